// pq_scan.hip -- top-k search over product-quantiser codes by asymmetric distance computation (kmamd_pq_search,
// pq_job.cpp).  L2, fp32 tables, uint8 codes, 1 <= M <= 64 sub-spaces, k <= 256.
//
//   pq_tables  grid = (sub-space, group of 64 queries).  A block stages the codeword panel of its sub-space in LDS (row
//              stride dsub | 1: no bank conflict at any dsub), thread c owns codeword c and builds, query by query,
//              T[q][m][c] = sum_j fl(fl(x_j - y_j)^2), j ascending from the j = 0 term, +inf for c >= ksub.  Plain
//              VALU arithmetic: the definition is term by term and the phase is Q * 256 * M * dsub operations, nothing
//              beside the scan.  The tables are written as the scan reads them: [query tile][m][code][q in tile].
//   pq_scan    grid = (row chunk, query tile), the row chunk running fastest.  Table-stationary: a block copies the QT
//              tables of its query tile into LDS once (QT * M KB) and streams the code rows of its chunk, one row per
//              lane and step (16-byte loads where M and the base allow, else 4-byte, else bytes), the row's bytes in
//              VGPRs (the next step's already in flight).  For every byte ONE LDS
//              read fetches the QT adjacent entries T[m][code][0..QT) -- ds_read_b128 per four queries -- and feeds QT
//              independent add chains, m ascending from the m = 0 term.
//              Selection (pq_select.hpp, shared with ivfpq_scan.hip):
//              per query an LDS buffer of `cap` >= 2k keys (bits(d) << 32 | row, NaN canonical), a count and
//              a threshold key that every lane holds in registers.  A lane appends a key only below the threshold (one
//              LDS integer atomic per wave and query, by ballot); a buffer that fills is sorted by the block (bitonic),
//              cut to its k smallest keys and lowers the threshold; lanes that found no room try again against the new
//              threshold.  The compare is on the whole 64-bit key, so what is kept is the k smallest keys of the chunk
//              whatever order the lanes arrived in.  The block writes k sorted keys per (query, chunk).
//   pq_merge   one block per query: the chunks' keys, 256 at a time, through a 512-key bitonic sort whose lower half
//              carries the best so far; writes the k indices and distances.
#include <float.h>
#include <math.h>

#include "kernels.hpp"
#include "pq_select.hpp"

namespace kmx {

namespace {

constexpr uint32_t kPqTableQueries = 64;         // pq_tables: queries per block, a multiple of every query tile

__global__ __launch_bounds__(kPqThreads) void pq_tables_kernel(const float *__restrict__ queries, uint32_t Qc,
                                                               const float *__restrict__ codebooks, uint32_t M,
                                                               uint32_t dsub, uint32_t ksub, uint32_t QT,
                                                               float *__restrict__ tables) {
  extern __shared__ float pq_panel[];   // ksub x (dsub | 1)
  const uint32_t m = blockIdx.x, c = threadIdx.x, ld = dsub | 1u;
  const float *book = codebooks + (size_t)m * ksub * dsub;
  for (uint32_t i = c; i < ksub * dsub; i += kPqThreads) pq_panel[(i / dsub) * ld + i % dsub] = book[i];
  __syncthreads();
  const float *y = pq_panel + c * ld;
  const uint32_t q0 = blockIdx.y * kPqTableQueries, q_pad = (Qc + QT - 1) / QT * QT;
  for (uint32_t q = q0; q < q0 + kPqTableQueries && q < q_pad; q++) {
    float d = INFINITY;   // a code byte that names no codeword, and the queries that pad the last tile
    if (q < Qc && c < ksub) {
      const float *x = queries + (size_t)q * M * dsub + (size_t)m * dsub;
      const float t0 = x[0] - y[0];
      d = t0 * t0;
      for (uint32_t j = 1; j < dsub; j++) {
        const float t = x[j] - y[j];
        d = d + t * t;
      }
    }
    tables[(((size_t)(q / QT) * M + m) * 256 + c) * QT + q % QT] = d;
  }
}

template <int QT, bool VEC>
__global__ __launch_bounds__(kPqThreads) void pq_scan_kernel(PqGeom g, const float *__restrict__ tables,
                                                             uint32_t queries, uint64_t *__restrict__ part) {
  extern __shared__ float4 pq_lds4[];
  const uint32_t M = g.M, k = g.k, cap = g.cap, t = threadIdx.x;
  const uint32_t chunk = blockIdx.x % g.G, tile = blockIdx.x / g.G;
  float *T = reinterpret_cast<float *>(pq_lds4);                          // M x 256 x QT
  uint64_t *buf = reinterpret_cast<uint64_t *>(T + (size_t)QT * M * 256);   // QT x cap
  uint64_t *thr = buf + (size_t)QT * cap;                                 // QT
  uint32_t *cnt = reinterpret_cast<uint32_t *>(thr + QT);                 // QT
  uint32_t *full = cnt + QT;                                              // the round in which a buffer last filled
  {
    const float4 *src = reinterpret_cast<const float4 *>(tables + (size_t)tile * QT * M * 256);
    for (uint32_t i = t; i < (uint32_t)QT * M * 64; i += kPqThreads) pq_lds4[i] = src[i];
    if (t < (uint32_t)QT) { thr[t] = kPqNoKey; cnt[t] = 0; }
    if (t == 0) *full = 0;
  }
  __syncthreads();

  const bool dwords = (M & 3u) == 0 && (reinterpret_cast<uintptr_t>(g.codes) & 3u) == 0;
  const uint64_t r0 = (uint64_t)chunk * g.R, r1 = r0 + g.R < g.N ? r0 + g.R : g.N;
  uint64_t limit[QT];   // every lane's copy of thr[]
#pragma unroll
  for (int q = 0; q < QT; q++) limit[q] = kPqNoKey;
  uint32_t round = 0, w[16], wn[16];
  pq_load_codes<VEC>(g.codes, r0 + t, r0 + t < r1, M, dwords, wn);
  for (uint64_t base = r0; base < r1; base += kPqThreads) {
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = wn[i];
    const uint64_t row = base + t, next = row + kPqThreads;
    pq_load_codes<VEC>(g.codes, next, next < r1, M, dwords, wn);

    float acc[QT];
    pq_score<QT, VEC>(T, w, M, acc);

    uint64_t key[QT];
    uint32_t todo = 0;
#pragma unroll
    for (int q = 0; q < QT; q++) {
      const uint32_t bits = acc[q] != acc[q] ? kPqNanBits : __float_as_uint(acc[q]);
      key[q] = (uint64_t)bits << 32 | (uint32_t)row;
      if (row < r1 && key[q] < limit[q]) todo |= 1u << q;
    }
    pq_append<QT>(buf, thr, cnt, full, cap, k, t, key, todo, limit, round);
  }
  pq_reduce<QT>(buf, thr, cnt, cap, k, (1u << QT) - 1u, t);
#pragma unroll
  for (int q = 0; q < QT; q++) {
    const uint32_t query = tile * QT + q;
    if (query < queries && t < k)
      part[((size_t)query * g.G + chunk) * k + t] = t < cnt[q] ? buf[q * cap + t] : kPqNoKey;
  }
}

__global__ __launch_bounds__(kPqThreads) void pq_merge_kernel(const uint64_t *__restrict__ part, uint32_t G, uint32_t k,
                                                              uint32_t *__restrict__ indices,
                                                              float *__restrict__ distances) {
  __shared__ uint64_t s[2 * kPqThreads];   // [0, 256): the best so far; [256, 512): the next 256 keys
  const uint32_t q = blockIdx.x, t = threadIdx.x;
  const uint64_t total = (uint64_t)G * k;
  const uint64_t *mine = part + (size_t)q * total;
  s[t] = kPqNoKey;
  for (uint64_t at = 0; at < total; at += kPqThreads) {
    s[kPqThreads + t] = at + t < total ? mine[at + t] : kPqNoKey;
    __syncthreads();
    for (uint32_t size = 2; size <= 2 * kPqThreads; size <<= 1)
      for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
        const uint32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const uint64_t a = s[lo], b = s[hi];
        if ((a > b) == ((lo & size) == 0)) {
          s[lo] = b;
          s[hi] = a;
        }
        __syncthreads();
      }
  }
  if (t < k) {
    indices[(size_t)q * k + t] = (uint32_t)s[t];
    distances[(size_t)q * k + t] = __uint_as_float((uint32_t)(s[t] >> 32));
  }
}

template <int QT>
hipError_t pq_scan_launch(const PqGeom &g, bool vec, const float *tables, uint32_t queries, uint64_t *part,
                          hipStream_t st) {
  const size_t lds = pq_scan_lds_bytes(g.M, g.k, QT);
  const uint32_t tiles = (queries + QT - 1) / QT;
  // M a multiple of 16 has a tile of at most 4: the larger tiles have no 16-byte variant
  return with_flag(vec && QT <= 4, [&](auto V16) {
    using V = std::integral_constant<bool, decltype(V16)::value && QT <= 4>;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&pq_scan_kernel<QT, V::value>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((pq_scan_kernel<QT, V::value>), dim3(g.G * tiles), dim3(kPqThreads), lds, st, g, tables, queries,
                       part);
    return hipGetLastError();
  });
}

}  // namespace

uint32_t pq_candidate_cap(uint32_t k) {
  uint32_t cap = 64;
  while (cap < 2 * k) cap <<= 1;
  return cap;
}

size_t pq_scan_lds_bytes(uint32_t M, uint32_t k, uint32_t QT) {
  return (size_t)QT * ((size_t)M * 1024 + (size_t)pq_candidate_cap(k) * 8 + 16) + 16;
}

uint32_t pq_query_tile(uint32_t M, uint32_t k) {
  if (M == 0 || M > 64 || k == 0 || k > 256) return 0;
  for (uint32_t qt : {16u, 8u, 4u})   // two blocks per CU
    if (pq_scan_lds_bytes(M, k, qt) <= kPqLdsPerCu / 2) return qt;
  for (uint32_t qt : {4u, 2u})        // one
    if (pq_scan_lds_bytes(M, k, qt) <= kPqLdsPerCu) return qt;
  return 0;
}

hipError_t launch_pq_tables(const float *queries, uint32_t Qc, const float *codebooks, uint32_t M, uint32_t dsub,
                            uint32_t ksub, uint32_t QT, float *tables, hipStream_t st) {
  const size_t lds = (size_t)ksub * (dsub | 1u) * sizeof(float);
  const uint32_t q_pad = (Qc + QT - 1) / QT * QT;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&pq_tables_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pq_tables_kernel, dim3(M, (q_pad + kPqTableQueries - 1) / kPqTableQueries), dim3(kPqThreads), lds,
                     st, queries, Qc, codebooks, M, dsub, ksub, QT, tables);
  return hipGetLastError();
}

hipError_t launch_pq_scan(const PqGeom &g, const float *tables, uint32_t queries, uint64_t *part, hipStream_t st) {
  const bool vec = (g.M & 15u) == 0 && (((uintptr_t)g.codes) & 15u) == 0;
  switch (g.QT) {
    case 2: return pq_scan_launch<2>(g, vec, tables, queries, part, st);
    case 4: return pq_scan_launch<4>(g, vec, tables, queries, part, st);
    case 8: return pq_scan_launch<8>(g, vec, tables, queries, part, st);
    case 16: return pq_scan_launch<16>(g, vec, tables, queries, part, st);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_pq_merge(const uint64_t *part, uint32_t queries, uint32_t G, uint32_t k, uint32_t *indices,
                           float *distances, hipStream_t st) {
  hipLaunchKernelGGL(pq_merge_kernel, dim3(queries), dim3(kPqThreads), 0, st, part, G, k, indices, distances);
  return hipGetLastError();
}

}  // namespace kmx
