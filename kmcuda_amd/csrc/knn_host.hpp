// knn_host.hpp -- host pieces the k-NN entry points share: knn_cuda()'s KnnJob (kmcuda_api.cpp) and the prepared
// corpus of kmamd_knn_index_* (knn_index.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "../../include/kmcuda.h"
#include "engine.hpp"

namespace kmx {

// One GPU's copy of the corpus (and, in knn_cuda(), its slice of the queries): device buffers it owns, freed with it.
struct KnnShard {
  int dev = 0;
  hipStream_t stream = nullptr;
  const float *samples = nullptr, *centroids = nullptr;
  const uint32_t *assignments = nullptr;
  float *xs = nullptr, *n2s = nullptr, *mydist = nullptr, *rdist = nullptr, *R = nullptr, *C = nullptr, *heaps = nullptr;
  float *mu = nullptr, *mux = nullptr, *kbias = nullptr;
  uint16_t *xs16 = nullptr;
  uint32_t *inv = nullptr, *offsets = nullptr, *keys_tmp = nullptr, *vals_tmp = nullptr, *keys_sorted = nullptr,
           *stats = nullptr, *blocks = nullptr, *out = nullptr;
  unsigned long long *calced = nullptr;
  void *sort_temp = nullptr;
  uint32_t first_block = 0, nblocks = 0, p_base = 0, p_end = 0;
  std::vector<void *> owned;
  ~KnnShard() {
    (void)hipSetDevice(dev);
    for (void *p : owned) (void)hipFree(p);
    pooled_stream_release(dev, stream);
  }
  template <typename T>
  int alloc(T **p, size_t count) {
    void *q = nullptr;
    if (hipMalloc(&q, count ? count * sizeof(T) : sizeof(T)) != hipSuccess) return kmcudaMemoryAllocationFailure;
    owned.push_back(q);
    *p = static_cast<T *>(q);
    return 0;
  }
  // frees one buffer of alloc() early (a no-op for anything else, e.g. a caller's buffer used in place)
  void release(const void *p) {
    for (size_t i = 0; i < owned.size(); i++)
      if (owned[i] == p) {
        (void)hipFree(owned[i]);
        owned.erase(owned.begin() + i);
        return;
      }
  }
  // brings `count` elements of a caller buffer onto this device (or uses it in place)
  template <typename T>
  int stage_in(const T *src, size_t count, int32_t device_ptrs, const T **dst) {
    if (device_ptrs >= 0 && device_ptrs == dev) {
      *dst = src;
      return 0;
    }
    T *buf = nullptr;
    int rc = alloc(&buf, count);
    if (rc) return rc;
    hipError_t e = device_ptrs < 0
                       ? hipMemcpyAsync(buf, src, count * sizeof(T), hipMemcpyHostToDevice, stream)
                       : hipMemcpyPeerAsync(buf, dev, src, device_ptrs, count * sizeof(T), stream);
    if (e != hipSuccess) return kmcudaMemoryCopyError;
    *dst = buf;
    return 0;
  }
};

// brings `count` halves of a caller buffer onto the shard's device and widens them to fp32
inline int stage_in_half(KnnShard &sh, const void *src, size_t count, int32_t device_ptrs, const float **dst) {
  float *buf = nullptr;
  int rc = sh.alloc(&buf, count);
  if (rc) return rc;
  const uint16_t *dev_half = reinterpret_cast<const uint16_t *>(src);
  uint16_t *tmp = nullptr;
  if (!(device_ptrs >= 0 && device_ptrs == sh.dev)) {
    if ((rc = sh.alloc(&tmp, count))) return rc;
    hipError_t e = device_ptrs < 0 ? hipMemcpyAsync(tmp, src, count * sizeof(uint16_t), hipMemcpyHostToDevice, sh.stream)
                                   : hipMemcpyPeerAsync(tmp, sh.dev, src, device_ptrs, count * sizeof(uint16_t), sh.stream);
    if (e != hipSuccess) return kmcudaMemoryCopyError;
    dev_half = tmp;
  }
  if (launch_half_to_float(dev_half, count, buf, sh.stream) != hipSuccess) return kmcudaRuntimeError;
  *dst = buf;
  return 0;
}

// Which search runs: dp_filter = the padded width of the matrix-core filter (0: every candidate evaluated exactly), DP
// = the row stride of the sorted copies, use_f16 = the f16 filter (else the f32 one), strict_h2 = the reference's half2
// arithmetic.  The half range can still send a call from the f16 filter to another one.
struct KnnPath {
  uint32_t dp_filter = 0, DP = 0;
  bool use_f16 = false, strict_h2 = false;
};
inline KnnPath knn_choose_path(uint32_t D, bool fp16, int verbosity) {
  KnnPath p;
  const char *force_exact = getenv("KMCUDA_AMD_KNN_EXACT");
  // KMCUDA_AMD_FP16_STRICT (fp16x2 only): radii, centroid distances and every candidate distance in the reference's
  // half2 arithmetic (knn.hip, half2_ops.hpp) -- the verification mode of half2_strict.hip for this entry point;
  // no matrix-core filter (its bound is stated against the fp32 arithmetic)
  const char *strict_env = getenv("KMCUDA_AMD_FP16_STRICT");
  p.strict_h2 = fp16 && strict_env && atoi(strict_env) != 0;
  if (p.strict_h2 && verbosity > 0) printf("k-NN: the reference's half2 arithmetic (KMCUDA_AMD_FP16_STRICT)\n");
  const char *fenv = getenv("KMCUDA_AMD_FILTER");
  const bool want_f32 = fenv && strcmp(fenv, "f32") == 0;
  p.dp_filter = ((force_exact && atoi(force_exact)) || p.strict_h2) ? 0 : filter_dp_for(D);
  // 256 < D <= 1024: the f16 filter's one-operand-set instantiations (knn_f16.hip: 512 with two blocks per CU;
  // 768 / 1024 with one -- the queries' operands alone are 192 / 256 registers; the f32 filter stops at 256)
  if (!p.dp_filter && !(force_exact && atoi(force_exact)) && !p.strict_h2 && !want_f32 && D > 256 && D <= 1024)
    p.dp_filter = D <= 512 ? 512u : (D <= 768 ? 768u : 1024u);
  p.DP = p.dp_filter ? p.dp_filter : D;
  if (!p.dp_filter && verbosity > 0) printf("k-NN: every candidate is evaluated with the exact arithmetic (no matrix-core filter)\n");
  // which matrix-core instruction filters the candidates: f16 on centred hi/lo-split rows (default,
  // needs DP >= 16) or f32 (KMCUDA_AMD_FILTER=f32)
  p.use_f16 = p.dp_filter >= 16 && !want_f32;
  return p;
}

// The f16 filter's centre: mu = mean of the finite centroid rows (any vector works: distances are translation
// invariant), mu_host[0, D) (the rest of it stays as it is: zeros), *mu2 = ||mu||^2 rounded up
inline int knn_centroid_mean(const void *centroids, uint32_t K, uint32_t D, bool fp16, int32_t device_ptrs,
                             std::vector<float> &mu_host, float *mu2) {
  std::vector<float> cen((size_t)K * D);
  if (fp16) {
    std::vector<uint16_t> raw((size_t)K * D);
    if (device_ptrs < 0) memcpy(raw.data(), centroids, raw.size() * sizeof(uint16_t));
    else if (hipMemcpy(raw.data(), centroids, raw.size() * sizeof(uint16_t), hipMemcpyDeviceToHost) != hipSuccess)
      return kmcudaMemoryCopyError;
    for (size_t i = 0; i < raw.size(); i++) {  // half -> float on the host
      const uint32_t hbits = raw[i], sign = (hbits & 0x8000u) << 16, ex = (hbits >> 10) & 0x1Fu, man = hbits & 0x3FFu;
      float v;
      if (ex == 0) v = ldexpf((float)man, -24);
      else if (ex == 31) v = man ? NAN : INFINITY;
      else v = ldexpf((float)(man | 0x400u), (int)ex - 25);
      cen[i] = sign ? -v : v;
    }
  } else if (device_ptrs < 0) {
    memcpy(cen.data(), centroids, cen.size() * sizeof(float));
  } else if (hipMemcpy(cen.data(), centroids, cen.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
    return kmcudaMemoryCopyError;
  }
  std::vector<double> acc(D, 0.0);
  uint32_t nfin = 0;
  for (uint32_t c = 0; c < K; c++) {
    bool fin = true;
    for (uint32_t f = 0; f < D && fin; f++) fin = std::isfinite(cen[(size_t)c * D + f]);
    if (!fin) continue;
    for (uint32_t f = 0; f < D; f++) acc[f] += cen[(size_t)c * D + f];
    nfin++;
  }
  float m2 = 0.f;
  for (uint32_t f = 0; f < D; f++) {
    mu_host[f] = nfin ? (float)(acc[f] / nfin) : 0.f;
    m2 += mu_host[f] * mu_host[f];
  }
  *mu2 = m2 * 1.0001f;
  return 0;
}

// The corpus in cluster-sorted order: the CSR of the assignments (inv, offsets), the DP-padded fp32 copy xs, its
// plain squared norms and their maximum (stats[0]); with the f16 filter (mu) also the half-range flag stats[1]
inline int knn_sort_and_gather(KnnShard &s, uint32_t N, uint32_t D, uint32_t DP, uint32_t K, bool use_f16,
                               size_t sort_bytes) {
  if (hipMemsetAsync(s.calced, 0, KNN_STATS * sizeof(unsigned long long), s.stream) != hipSuccess) return kmcudaRuntimeError;
  if (launch_inverse_assignments(s.assignments, N, K, s.keys_tmp, s.vals_tmp, s.keys_sorted, s.inv, s.offsets,
                                 s.sort_temp, sort_bytes, s.stream) != hipSuccess)
    return kmcudaRuntimeError;
  if (launch_knn_gather(s.samples, N, D, DP, s.inv, s.xs, s.n2s, s.stats, use_f16 ? s.mu : nullptr, s.offsets, K,
                        s.stream) != hipSuccess)
    return kmcudaRuntimeError;
  return 0;
}

}  // namespace kmx
