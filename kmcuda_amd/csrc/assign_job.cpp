// assign_job.cpp -- kmamd_kmeans_assign of include/kmcuda_amd.h: new rows assigned to given centroids (the "predict"
// of a trained K-means), with the distance of every row to its centroid and per-cluster statistics.
//
// The rows go through in chunks (host_job.hpp: assign_chunk_rows, RowStage): assignments <- K, ONE assignment pass of
// the engine (the filtered, bit-exact kmamd_lloyd_assign; no row cache, no carried bounds: a chunk is seen once), the
// distance kernel, the cluster statistics, copy out.  A shorter last chunk gets an ENGINE OF ITS OWN, sized for it
// (EngineSlot): the assignment pass then covers exactly the chunk's rows, nothing is read behind a
// caller's device buffer and no padding row is assigned or counted.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/kmcuda_amd.h"
#include "host_job.hpp"

using namespace kmx;

namespace {

// KMCUDA_AMD_ASSIGN_DIST=member: the distance pass on member_distances_kernel (the A/B)
bool assign_dist_member() {
  const char *v = getenv("KMCUDA_AMD_ASSIGN_DIST");
  return v && strcmp(v, "member") == 0;
}

hipError_t distance_pass(bool member, int metric, const float *rows, uint32_t n, uint32_t D, const float *centroids,
                         const uint32_t *assignments, uint32_t K, float *dists, hipStream_t st) {
  return member ? launch_member_distances(metric, rows, n, D, centroids, assignments, K, dists, st, true)
                : launch_assigned_distances(metric, rows, n, D, centroids, assignments, K, dists, st);
}

struct AssignJob {
  int metric = 0, device = 0, verbosity = 0;
  bool fp16 = false, host = true;
  uint32_t N = 0, D = 0, K = 0;
  const void *samples = nullptr, *centroids_in = nullptr;
  uint32_t *assignments = nullptr, *counts = nullptr;
  float *distances = nullptr;
  double *sums = nullptr;

  int run() {
    const bool member = assign_dist_member();
    DeviceArena w;   // owns the call's buffers and its pooled stream (destroyed after the engine below)
    w.dev = device;
    w.stream = pooled_stream_acquire(device);
    if (!w.stream) return kmcudaRuntimeError;
    const hipStream_t st = w.stream;
    const bool want_stats = counts || sums, want_dist = distances || sums;

    // ---- the statistics accumulate over the chunks: zeroed first (also what an empty call returns) ----
    uint32_t *counts_dev = host ? nullptr : counts;
    double *sums_dev = host ? nullptr : sums;
    if (host && counts) KNN_TRY(w.alloc(&counts_dev, K));
    if (host && sums) KNN_TRY(w.alloc(&sums_dev, K));
    if (counts_dev) KMX_HIPRT(hipMemsetAsync(counts_dev, 0, (size_t)K * sizeof(uint32_t), st));
    if (sums_dev) KMX_HIPRT(hipMemsetAsync(sums_dev, 0, (size_t)K * sizeof(double), st));

    if (N != 0) {
      // ---- the centroids, fp32 on this device ----
      RowStage cstage, rstage;
      const float *cen = nullptr;
      KNN_TRY(cstage.reserve(w, K, D, fp16, host));
      KNN_TRY(cstage.stage(centroids_in, 0, K, &cen));

      // ---- one chunk's buffers, reused by every chunk ----
      const size_t chunk = assign_chunk_rows(D);
      const uint32_t Nc = (uint32_t)(chunk < N ? chunk : N);
      float *dist_buf = nullptr;
      uint32_t *asg_buf = nullptr, *prev = nullptr, *inv = nullptr, *offsets = nullptr, *keys_tmp = nullptr,
               *vals_tmp = nullptr, *keys_sorted = nullptr;
      char *sort_temp = nullptr;
      size_t sort_bytes = 0;
      KNN_TRY(rstage.reserve(w, Nc, D, fp16, host));
      if (host) KNN_TRY(w.alloc(&asg_buf, Nc));
      KNN_TRY(w.alloc(&prev, Nc));
      if (want_dist && (host || !distances)) KNN_TRY(w.alloc(&dist_buf, Nc));
      if (want_stats) {
        KNN_TRY(w.alloc(&inv, Nc));
        KNN_TRY(w.alloc(&offsets, (size_t)K + 2));
        KNN_TRY(w.alloc(&keys_tmp, Nc));
        KNN_TRY(w.alloc(&vals_tmp, Nc));
        KNN_TRY(w.alloc(&keys_sorted, Nc));
        sort_bytes = sort_temp_bytes(Nc, K);
        KNN_TRY(w.alloc(&sort_temp, sort_bytes + 16));
      }

      EngineSlot slot;   // sized for the chunk at hand: Nc rows, then the shorter last chunk's
      for (uint32_t q0 = 0; q0 < N; q0 += Nc) {
        const uint32_t n = N - q0 < Nc ? N - q0 : Nc;
        // ---- the engine, then the chunk's rows, fp32 on this device (+ the halves for the filter) ----
        const float *rows = nullptr;
        Engine *eng = nullptr;
        KNN_TRY(slot.get(device, n, D, K, metric, st, rstage.halves_at(samples, q0), &eng));
        KNN_TRY(rstage.stage(samples, q0, n, &rows));
        // ---- assignments <- K ("no cluster"), then one pass: a row without a nearest centroid keeps K ----
        uint32_t *asg = host ? asg_buf : assignments + q0;
        KMX_HIPRT(hipMemsetD32Async((hipDeviceptr_t)asg, (int)K, n, st));
        KNN_TRY(eng->lloyd_assign(rows, cen, asg, prev, false));
        // ---- distances and statistics ----
        float *dist = nullptr;
        if (want_dist) {
          dist = (!host && distances) ? distances + q0 : dist_buf;
          KMX_HIPRT(distance_pass(member, metric, rows, n, D, cen, asg, K, dist, st));
        }
        if (want_stats) {
          KMX_HIPRT(launch_inverse_assignments(asg, n, K, keys_tmp, vals_tmp, keys_sorted, inv, offsets, sort_temp,
                                               sort_bytes, st));
          KMX_HIPRT(launch_cluster_stats(dist, inv, offsets, K, counts_dev, sums_dev, st));
        }
        if (host) {
          KMX_HIPCP(hipMemcpyAsync(assignments + q0, asg, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
          if (distances)
            KMX_HIPCP(hipMemcpyAsync(distances + q0, dist, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
        }
        // (the next chunk overwrites these buffers: the stream orders it behind this one's kernels and copies)
      }
      if (hipStreamSynchronize(st) != hipSuccess) {
        if (verbosity > 0) printf("kmamd_kmeans_assign failed: %s\n", hipGetErrorString(hipGetLastError()));
        return kmcudaRuntimeError;
      }
    }
    if (host && counts)
      KMX_HIPCP(hipMemcpyAsync(counts, counts_dev, (size_t)K * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (host && sums)
      KMX_HIPCP(hipMemcpyAsync(sums, sums_dev, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, st));
    KMX_HIPRT(hipStreamSynchronize(st));
    return kmcudaSuccess;
  }
};

}  // namespace

extern "C" {

int kmamd_kmeans_assign(int metric, uint32_t samples_size, uint16_t features_size, uint32_t clusters_size, int device,
                        int32_t device_ptrs, int32_t fp16x2, int32_t verbosity, const void *samples,
                        const void *centroids, uint32_t *assignments, float *distances, uint32_t *cluster_counts,
                        double *cluster_distance_sums) {
  // ---- everything that is refused is refused here, before any device work, with the outputs untouched ----
  if (clusters_size < 2 || clusters_size >= 0x7FFFFFFFu) return kmcudaInvalidArguments;
  if (!centroids || (samples_size != 0 && (!samples || !assignments))) return kmcudaInvalidArguments;
  KNN_TRY(rows_call_begin(metric, features_size, fp16x2, device, device_ptrs, verbosity));
  if (device_ptrs >= 0) (void)hipDeviceSynchronize();   // the caller's writes, as the k-NN index's calls
  AssignJob job;
  job.metric = metric; job.device = device; job.verbosity = verbosity;
  job.fp16 = fp16x2 != 0; job.host = device_ptrs < 0;
  job.N = samples_size; job.D = features_size; job.K = clusters_size;
  job.samples = samples; job.centroids_in = centroids;
  job.assignments = assignments; job.distances = distances; job.counts = cluster_counts;
  job.sums = cluster_distance_sums;
  return job.run();
}

int kmamd_assigned_distances(int metric, uint32_t n_rows, uint32_t features, uint32_t clusters, int device,
                             const float *samples, const float *centroids, const uint32_t *assignments,
                             float *distances, void *hip_stream) {
  if ((metric != 0 && metric != 1) || features == 0 || clusters == 0) return kmcudaInvalidArguments;
  if (n_rows == 0) return kmcudaSuccess;
  if (!samples || !centroids || !assignments || !distances) return kmcudaInvalidArguments;
  if (hipSetDevice(device) != hipSuccess) return kmcudaNoSuchDevice;
  KMX_HIPRT(distance_pass(assign_dist_member(), metric, samples, n_rows, features, centroids, assignments,
                          clusters, distances, (hipStream_t)hip_stream));
  return kmcudaSuccess;
}

}  // extern "C"
