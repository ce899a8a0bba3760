// knn_rerank_job.cpp -- kmamd_knn_rerank of include/kmcuda_amd.h: exact re-ranking of per-query candidate lists
// (DESIGN.md 4.23).  The kernel is knn_rerank.hip's; nothing here goes through an Engine.
//
// Every operand goes to the device whole -- a host call stages the whole row matrix; the intended use is
// device-resident -- and the call is one launch and one stream sync.
#include <stdio.h>

#include "../../include/kmcuda_amd.h"
#include "host_job.hpp"

using namespace kmx;

extern "C" {

int kmamd_knn_rerank(uint32_t queries_size, uint64_t samples_size, uint32_t features_size, uint32_t candidates_size,
                     uint32_t k, int metric, int32_t fp16x2, int device, int32_t device_ptrs, int32_t verbosity,
                     const float *queries, const float *samples, const uint32_t *candidates, uint32_t *indices,
                     float *distances) {
  const uint32_t Q = queries_size, D = features_size, R = candidates_size;
  const uint64_t N = samples_size;
  // everything that is refused, before any device work
  if (metric != 0 || fp16x2 != 0 || D == 0) return kmcudaInvalidArguments;
  if (N == 0 || N > 0xFFFFFFFEull) return kmcudaInvalidArguments;
  if (k == 0 || k > 256 || R > 1024 || k > R) return kmcudaInvalidArguments;
  if (device < 0 || (device_ptrs >= 0 && device_ptrs != device)) return kmcudaInvalidArguments;
  if (!samples) return kmcudaInvalidArguments;
  if (Q != 0 && (!queries || !candidates || !indices || !distances)) return kmcudaInvalidArguments;
  if (Q == 0) return kmcudaSuccess;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) return kmcudaNoSuchDevice;
  if (hipSetDevice(device) != hipSuccess) return kmcudaNoSuchDevice;
  g_verbosity = verbosity;
  const bool host = device_ptrs < 0;
  if (!host) (void)hipDeviceSynchronize();   // the caller's writes, as kmamd_kmeans_assign

  DeviceArena w;
  w.dev = device;
  w.stream = pooled_stream_acquire(device);
  if (!w.stream) return kmcudaRuntimeError;
  const hipStream_t st = w.stream;
  const float *qry = nullptr, *x = nullptr;
  const uint32_t *cand = nullptr;
  KNN_TRY(w.stage_in(queries, (size_t)Q * D, device_ptrs, &qry));
  KNN_TRY(w.stage_in(samples, (size_t)N * D, device_ptrs, &x));
  KNN_TRY(w.stage_in(candidates, (size_t)Q * R, device_ptrs, &cand));
  uint32_t *idx = indices;
  float *dist = distances;
  if (host) {
    KNN_TRY(w.alloc(&idx, (size_t)Q * k));
    KNN_TRY(w.alloc(&dist, (size_t)Q * k));
  }
  if (verbosity > 1)
    printf("knn_rerank: %u queries x %u candidates, %u queries per block step, %zu bytes of LDS\n", Q, R,
           knn_rerank_query_block(R), knn_rerank_lds_bytes(R));
  KMX_HIPRT(launch_knn_rerank(qry, Q, x, (uint32_t)N, D, cand, R, k, idx, dist, st));
  if (host) {
    KMX_HIPCP(hipMemcpyAsync(indices, idx, (size_t)Q * k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    KMX_HIPCP(hipMemcpyAsync(distances, dist, (size_t)Q * k * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  if (hipStreamSynchronize(st) != hipSuccess) {
    if (verbosity > 0) printf("kmamd_knn_rerank failed: %s\n", hipGetErrorString(hipGetLastError()));
    return kmcudaRuntimeError;
  }
  return kmcudaSuccess;
}

}  // extern "C"
