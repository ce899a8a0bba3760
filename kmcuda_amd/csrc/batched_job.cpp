// batched_job.cpp -- kmamd_kmeans_batched and kmamd_kmeans_assign_batched of include/kmcuda_amd.h: K-means over many
// small independent problems.  The kernels are lloyd_batched.hip's; nothing here goes through an Engine.
//
// The whole run is enqueued on one stream without a host round trip: per pass the assignment kernel, the partial sums
// and the finish kernel, which decides every problem's stop on the device (stop[b] = the pass it stopped at).  The
// blocks of a stopped problem return at once, so the passes enqueued behind the last stop cost a launch each and leave
// everything as it is; the host reads stop[] -- the iterations -- once, at the end.
#include <stdio.h>
#include <string.h>

#include <unordered_set>
#include <vector>

#include "../../include/kmcuda_amd.h"
#include "hash_draw.hpp"
#include "host_job.hpp"
#include "launch_dispatch.hpp"

using namespace kmx;

namespace {

constexpr uint32_t kBatchedPanelCells = 16384;   // K8 * DP: 64 KB of fp32 panel, 128 KB of fp64 update cells
constexpr uint32_t kBatchedBlocks = 2048;        // the grid the row chunks of all problems together aim at

// everything that is refused, before any device work
int batched_check(uint32_t B, uint32_t D, uint32_t K, int32_t layout, int metric, int32_t fp16x2, int device,
                  int32_t device_ptrs) {
  if (B == 0 || B > 65535u || (layout != 0 && layout != 1)) return kmcudaInvalidArguments;
  if (metric != 0 || fp16x2 != 0) return kmcudaInvalidArguments;
  const uint32_t kmax = kmamd_batched_max_clusters(D);
  if (kmax == 0 || K == 0 || K > kmax) return kmcudaInvalidArguments;
  if (device < 0 || (device_ptrs >= 0 && device_ptrs != device)) return kmcudaInvalidArguments;
  return kmcudaSuccess;
}

int batched_device(int device, int32_t device_ptrs, int32_t verbosity) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) return kmcudaNoSuchDevice;
  if (hipSetDevice(device) != hipSuccess) return kmcudaNoSuchDevice;
  g_verbosity = verbosity;
  if (device_ptrs >= 0) (void)hipDeviceSynchronize();   // the caller's writes, as kmamd_kmeans_assign
  return kmcudaSuccess;
}

BatchedGeom batched_geom(const float *rows, uint32_t B, uint32_t N, uint32_t D, uint32_t K, int32_t layout) {
  BatchedGeom g;
  g.rows = rows; g.B = B; g.N = N; g.D = D; g.K = K;
  if (layout == 0) {
    g.row_stride = D; g.prob_stride = (uint64_t)N * D; g.out_row_stride = 1; g.out_prob_stride = N;
  } else {
    g.row_stride = (uint64_t)B * D; g.prob_stride = D; g.out_row_stride = B; g.out_prob_stride = 1;
  }
  // row chunks: whole 256-row tiles, about kBatchedBlocks blocks over all problems, every chunk with a row in it
  const uint64_t tiles = ((uint64_t)N + 255) / 256;
  uint64_t want = kBatchedBlocks / B ? kBatchedBlocks / B : 1;
  if (want > tiles) want = tiles;
  if (want == 0) want = 1;
  const uint64_t R = (tiles + want - 1) / want * 256;
  g.R = (uint32_t)(R > 0xFFFFFF00ull ? 0xFFFFFF00ull : R);
  g.G = N ? (uint32_t)(((uint64_t)N + g.R - 1) / g.R) : 1;
  return g;
}

// K distinct rows of [0, N) for problem b: the draws t = 0, 1, ... of h(seed, b, t) in order, repeats skipped
void batched_random_rows(uint32_t seed, uint32_t b, uint32_t N, uint32_t K, uint32_t *out) {
  std::unordered_set<uint32_t> seen;
  uint32_t got = 0;
  for (uint32_t t = 0; got < K; t++) {
    const uint32_t row = (uint32_t)draw_row(hash_draw(seed, b, t), N);
    if (seen.insert(row).second) out[got++] = row;
  }
}

}  // namespace

extern "C" {

uint32_t kmamd_batched_max_clusters(uint32_t features_size) {
  const uint32_t dp = features_size ? batched_dp_for(features_size) : 0;
  return dp ? kBatchedPanelCells / dp : 0;
}

int kmamd_kmeans_assign_batched(uint32_t problems, uint32_t samples_size, uint16_t features_size,
                                uint32_t clusters_size, int32_t layout, int metric, int32_t fp16x2, int device,
                                int32_t device_ptrs, int32_t verbosity, int32_t codes_u8, const float *samples,
                                const float *centroids, void *assignments, float *distances) {
  const uint32_t B = problems, N = samples_size, D = features_size, K = clusters_size;
  KNN_TRY(batched_check(B, D, K, layout, metric, fp16x2, device, device_ptrs));
  if (codes_u8 && K > 256) return kmcudaInvalidArguments;
  if (!centroids || (N != 0 && (!samples || !assignments))) return kmcudaInvalidArguments;
  KNN_TRY(batched_device(device, device_ptrs, verbosity));
  if (N == 0) return kmcudaSuccess;
  const bool host = device_ptrs < 0;
  DeviceArena w;
  w.dev = device;
  w.stream = pooled_stream_acquire(device);
  if (!w.stream) return kmcudaRuntimeError;
  const hipStream_t st = w.stream;
  const size_t cells = (size_t)B * N, asg_bytes = cells * (codes_u8 ? 1 : sizeof(uint32_t));
  const float *rows = nullptr, *cen = nullptr;
  KNN_TRY(w.stage_in(samples, cells * D, device_ptrs, &rows));
  KNN_TRY(w.stage_in(centroids, (size_t)B * K * D, device_ptrs, &cen));
  char *asg = static_cast<char *>(assignments);
  float *dist = distances;
  if (host) {
    KNN_TRY(w.alloc(&asg, asg_bytes));
    if (distances) KNN_TRY(w.alloc(&dist, cells));
  }
  const BatchedGeom g = batched_geom(rows, B, N, D, K, layout);
  KMX_HIPRT(launch_batched_assign(g, cen, asg, codes_u8 != 0, dist, nullptr, nullptr, 0, st));
  if (host) {
    KMX_HIPCP(hipMemcpyAsync(assignments, asg, asg_bytes, hipMemcpyDeviceToHost, st));
    if (distances) KMX_HIPCP(hipMemcpyAsync(distances, dist, cells * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  if (hipStreamSynchronize(st) != hipSuccess) {
    if (verbosity > 0) printf("kmamd_kmeans_assign_batched failed: %s\n", hipGetErrorString(hipGetLastError()));
    return kmcudaRuntimeError;
  }
  return kmcudaSuccess;
}

int kmamd_kmeans_batched(uint32_t problems, uint32_t samples_size, uint16_t features_size, uint32_t clusters_size,
                         int32_t layout, int metric, int32_t fp16x2, int32_t init, float tolerance, uint32_t max_iter,
                         uint32_t seed, int device, int32_t device_ptrs, int32_t verbosity, const float *samples,
                         const float *weights, float *centroids, uint32_t *assignments, uint32_t *iterations) {
  const uint32_t B = problems, N = samples_size, D = features_size, K = clusters_size;
  KNN_TRY(batched_check(B, D, K, layout, metric, fp16x2, device, device_ptrs));
  if (weights || K > N || (init != 0 && init != 1) || max_iter == 0) return kmcudaInvalidArguments;
  if (!(tolerance >= 0.f && tolerance <= 1.f)) return kmcudaInvalidArguments;
  if (!samples || !centroids || !assignments || !iterations) return kmcudaInvalidArguments;
  KNN_TRY(batched_device(device, device_ptrs, verbosity));
  const bool host = device_ptrs < 0;
  DeviceArena w;
  w.dev = device;
  w.stream = pooled_stream_acquire(device);
  if (!w.stream) return kmcudaRuntimeError;
  const hipStream_t st = w.stream;
  const size_t cells = (size_t)B * N, cen_count = (size_t)B * K * D;
  const float *rows = nullptr;
  KNN_TRY(w.stage_in(samples, cells * D, device_ptrs, &rows));
  float *cen = centroids;
  uint32_t *asg = assignments, *stop = iterations, *changed = nullptr;
  if (host) {
    KNN_TRY(w.alloc(&cen, cen_count));
    KNN_TRY(w.alloc(&asg, cells));
    KNN_TRY(w.alloc(&stop, B));
  }
  KNN_TRY(w.alloc(&changed, B));
  const BatchedGeom g = batched_geom(rows, B, N, D, K, layout);

  // ---- the initial centroids ----
  if (init == 1) {
    std::vector<uint32_t> picks((size_t)B * K);
    for (uint32_t b = 0; b < B; b++) batched_random_rows(seed, b, N, K, picks.data() + (size_t)b * K);
    uint32_t *picks_dev = nullptr;
    KNN_TRY(w.alloc(&picks_dev, picks.size()));
    KMX_HIPCP(hipMemcpyAsync(picks_dev, picks.data(), picks.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    KMX_HIPRT(launch_batched_gather(g, picks_dev, cen, st));
    KMX_HIPRT(hipStreamSynchronize(st));   // picks goes out of scope
  } else if (host) {
    KMX_HIPCP(hipMemcpyAsync(cen, centroids, cen_count * sizeof(float), hipMemcpyHostToDevice, st));
  }

  // ---- the state of the run: no assignment yet, nothing changed, nobody stopped ----
  const uint32_t DP = batched_dp_for(D), K8 = (K + 7u) & ~7u;
  double *psum = nullptr;
  uint32_t *pcnt = nullptr;
  KNN_TRY(w.alloc(&psum, (size_t)B * g.G * K8 * DP));
  KNN_TRY(w.alloc(&pcnt, (size_t)B * g.G * K8));
  KMX_HIPRT(launch_batched_fill(asg, cells, 0xFFFFFFFFu, st));
  KMX_HIPRT(launch_batched_fill(changed, B, 0, st));
  KMX_HIPRT(launch_batched_fill(stop, B, 0, st));

  for (uint32_t pass = 1; pass <= max_iter; pass++) {
    KMX_HIPRT(launch_batched_assign(g, cen, asg, false, nullptr, changed, stop, pass, st));
    KMX_HIPRT(launch_batched_update(g, asg, psum, pcnt, cen, changed, stop, pass, max_iter, tolerance, st));
  }
  if (host) {
    KMX_HIPCP(hipMemcpyAsync(centroids, cen, cen_count * sizeof(float), hipMemcpyDeviceToHost, st));
    KMX_HIPCP(hipMemcpyAsync(assignments, asg, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    KMX_HIPCP(hipMemcpyAsync(iterations, stop, (size_t)B * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  }
  if (hipStreamSynchronize(st) != hipSuccess) {
    if (verbosity > 0) printf("kmamd_kmeans_batched failed: %s\n", hipGetErrorString(hipGetLastError()));
    return kmcudaRuntimeError;
  }
  return kmcudaSuccess;
}

}  // extern "C"
