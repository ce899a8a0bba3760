// seed_par_job.cpp -- kmamd_kmeans_seed_parallel of include/kmcuda_amd.h: k-means|| seeding (Bahmani et al., "Scalable
// K-Means++").  A handful of rounds draw about `oversampling` rows each, every row on its own by a hash
// of (seed, round, row); the few thousand candidates are weighted by the rows they attract and reclustered to K seeds
// by this library's weighted k-means++.
//
// The rows stay on the device for the whole call (host_job.hpp: one RowStage of all N rows).  A round is what
// kmamd_kmeans_assign does with a chunk, against the round's NEW candidates -- assignments <- M, one assignment pass of
// the engine (EngineSlot), the distance kernel -- followed by the kernels of seed_par.hip: the term update with
// its block sums, phi, the draw's count / prefix / fill.  The host reads one word per round: the number of drawn rows.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/kmcuda_amd.h"
#include "host_job.hpp"

using namespace kmx;

namespace {

// h(seed, r, s) of include/kmcuda_amd.h (seed_par.hip holds the device's copy)
uint64_t seed_par_hash(uint32_t seed, uint32_t r, uint32_t s) {
  uint64_t z = (((uint64_t)r << 32) | s) + ((uint64_t)seed + 1ull) * 0x9E3779B97F4A7C15ull;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

struct SeedParJob {
  int metric = 0, device = 0, verbosity = 0;
  bool fp16 = false, host = true;
  uint32_t N = 0, D = 0, K = 0, rounds = 0, seed = 0, capacity = 0;
  float ell = 0.f;
  const void *samples = nullptr;
  void *centroids = nullptr;
  uint32_t *cand_rows = nullptr, *cand_counts = nullptr, *n_candidates = nullptr, *round_ends = nullptr;
  int32_t *fell_back = nullptr;

  // one round's new candidates on the device: the row ids (ascending) and the rows, fp32
  struct Batch {
    uint32_t M = 0;
    uint32_t *ids = nullptr;
    float *rows = nullptr;
  };

  int run() {
    DeviceArena w;   // owns the call's buffers and its pooled stream (destroyed after the engine below)
    w.dev = device;
    w.stream = pooled_stream_acquire(device);
    if (!w.stream) return kmcudaRuntimeError;
    const hipStream_t st = w.stream;
    // KMCUDA_AMD_TIMING=1: wall-clock laps of the call's phases on stderr, as kmeans_cuda() (each lap waits for the GPU)
    PhaseClock clock(getenv("KMCUDA_AMD_TIMING") != nullptr, [st] { (void)hipStreamSynchronize(st); });

    // ---- the rows: fp32 on this device, and the halves they were widened from ----
    RowStage stage;
    const float *rows32 = nullptr;
    const void *rows16 = nullptr;
    KNN_TRY(stage.reserve(w, N, D, fp16, host));
    KNN_TRY(stage.stage(samples, 0, N, &rows32, &rows16));

    // ---- per-row and per-block state ----
    const size_t nb = seed_par_block_count(N), nchunks = seed_par_chunk_count(N);
    float *term = nullptr, *dist = nullptr;
    uint32_t *asg = nullptr, *prev = nullptr, *bcount = nullptr, *boff = nullptr, *aux = nullptr, *carry = nullptr;
    double *bsum = nullptr, *phi = nullptr;
    unsigned long long *best = nullptr;
    KNN_TRY(w.alloc(&term, N));
    KNN_TRY(w.alloc(&dist, N));
    KNN_TRY(w.alloc(&asg, N));
    KNN_TRY(w.alloc(&prev, N));
    KNN_TRY(w.alloc(&bcount, nb));
    KNN_TRY(w.alloc(&boff, nb));
    KNN_TRY(w.alloc(&aux, nchunks));
    KNN_TRY(w.alloc(&carry, nchunks + 1));
    KNN_TRY(w.alloc(&bsum, nb));
    KNN_TRY(w.alloc(&phi, 1));
    KNN_TRY(w.alloc(&best, 1));

    // ---- round 0: the first row at or cyclically after h(seed, 0, 0) % N whose first feature is not NaN ----
    uint32_t first = (uint32_t)(seed_par_hash(seed, 0, 0) % N);
    {
      float x0 = 0.f;
      KMX_HIPCP(hipMemcpyAsync(&x0, rows32 + (size_t)first * D, sizeof(float), hipMemcpyDeviceToHost, st));
      KMX_HIPRT(hipStreamSynchronize(st));
      if (x0 != x0) {
        unsigned long long off = ~0ull;
        KMX_HIPRT(hipMemsetAsync(best, 0xFF, sizeof(unsigned long long), st));
        KMX_HIPRT(launch_seed_par_first_valid(rows32, N, D, first, best, st));
        KMX_HIPCP(hipMemcpyAsync(&off, best, sizeof(off), hipMemcpyDeviceToHost, st));
        KMX_HIPRT(hipStreamSynchronize(st));
        if (off == ~0ull) {
          if (verbosity > 0) printf("k-means||: every row's first feature is NaN\n");
          return kmcudaInvalidArguments;
        }
        first = (uint32_t)(((uint64_t)first + off) % N);
      }
    }
    std::vector<Batch> batches;
    std::vector<uint32_t> ends;   // candidates after round 0 .. R
    uint32_t total = 0;
    EngineSlot slot;   // sized for (N rows, the round's M candidates); re-created when M changes
    Engine *eng = nullptr;
    // dist[s] = the distance of row s to its nearest of the batch's candidates, as kmeans_predict gives it (one
    // candidate: to that row, no engine); then the term update
    auto absorb = [&](const Batch &b, bool is_first, uint32_t r) -> int {
      if (b.M >= 2) {
        KNN_TRY(slot.get(device, N, D, b.M, metric, st, rows16, &eng));
        KMX_HIPRT(hipMemsetD32Async((hipDeviceptr_t)asg, (int)b.M, N, st));
        KNN_TRY(eng->lloyd_assign(rows32, b.rows, asg, prev, false));
        clock.lap("k-means|| round %u assignment", r);
      } else {
        KMX_HIPRT(hipMemsetD32Async((hipDeviceptr_t)asg, 0, N, st));
      }
      KMX_HIPRT(launch_assigned_distances(metric, rows32, N, D, b.rows, asg, b.M, dist, st));
      clock.lap("k-means|| round %u distance", r);
      KMX_HIPRT(launch_seed_par_update(term, dist, N, is_first ? rows32 : nullptr, D, bsum, phi, st));
      return 0;
    };
    {
      Batch b;
      b.M = 1;
      KNN_TRY(w.alloc(&b.ids, 1));
      KNN_TRY(w.alloc(&b.rows, D));
      KMX_HIPCP(hipMemcpyAsync(b.ids, &first, sizeof(uint32_t), hipMemcpyHostToDevice, st));
      KMX_HIPCP(hipMemcpyAsync(b.rows, rows32 + (size_t)first * D, (size_t)D * sizeof(float), hipMemcpyDeviceToDevice,
                               st));
      KNN_TRY(absorb(b, true, 0));
      KMX_HIPRT(hipStreamSynchronize(st));   // (`first` is read by the copy)
      batches.push_back(b);
      total = 1;
      ends.push_back(total);
      clock.lap("k-means|| round %u term update", 0u);
    }

    // ---- rounds 1 .. R (phi == 0 draws nothing: the remaining rounds add no candidate) ----
    for (uint32_t r = 1; r <= rounds; r++) {
      KMX_HIPRT(launch_seed_par_draw(term, N, seed, r, phi, ell, bcount, boff, aux, carry, st));
      uint32_t M = 0;
      KMX_HIPCP(hipMemcpyAsync(&M, carry + nchunks, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      KMX_HIPRT(hipStreamSynchronize(st));
      if (verbosity > 0) printf("k-means||: round %u draws %u rows\n", r, M);
      if (M != 0) {
        Batch b;
        b.M = M;
        KNN_TRY(w.alloc(&b.ids, M));
        KNN_TRY(w.alloc(&b.rows, (size_t)M * D));
        KMX_HIPRT(launch_seed_par_fill(term, N, seed, r, phi, ell, boff, carry, M, rows32, D, b.ids, b.rows, st));
        clock.lap("k-means|| round %u draw (count, prefix, fill)", r);
        KNN_TRY(absorb(b, false, r));
        clock.lap("k-means|| round %u term update", r);
        batches.push_back(b);
        total += M;
      }
      ends.push_back(total);
    }

    // ---- the weights: one assignment pass against ALL candidates; counts[j] = the rows candidate j attracts ----
    uint32_t *ids_all = nullptr, *counts_dev = nullptr;
    float *cand_all = nullptr;
    KNN_TRY(w.alloc(&ids_all, total));
    KNN_TRY(w.alloc(&cand_all, (size_t)total * D));
    KNN_TRY(w.alloc(&counts_dev, total));
    {
      size_t at = 0;
      for (const Batch &b : batches) {
        KMX_HIPCP(hipMemcpyAsync(ids_all + at, b.ids, (size_t)b.M * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        KMX_HIPCP(hipMemcpyAsync(cand_all + at * D, b.rows, (size_t)b.M * D * sizeof(float), hipMemcpyDeviceToDevice,
                                 st));
        at += b.M;
      }
    }
    std::vector<uint32_t> ids_host(total), counts_host(total);
    if (total >= 2) {
      KNN_TRY(slot.get(device, N, D, total, metric, st, rows16, &eng));
      KMX_HIPRT(hipMemsetD32Async((hipDeviceptr_t)asg, (int)total, N, st));
      KNN_TRY(eng->lloyd_assign(rows32, cand_all, asg, prev, false));
      KMX_HIPRT(hipMemsetAsync(counts_dev, 0, (size_t)total * sizeof(uint32_t), st));
      KMX_HIPRT(launch_seed_par_weights(asg, N, total, counts_dev, st));
      KMX_HIPCP(hipMemcpyAsync(counts_host.data(), counts_dev, (size_t)total * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, st));
    } else {
      counts_host[0] = N;   // a lone candidate (no predict form with one centroid; K >= 2: the call falls back)
    }
    KMX_HIPCP(hipMemcpyAsync(ids_host.data(), ids_all, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    KMX_HIPRT(hipStreamSynchronize(st));
    slot.reset();
    clock.lap("k-means|| round %u weighting pass", rounds);

    // ---- the live candidates, in order ----
    std::vector<uint32_t> live_rows;
    std::vector<float> live_w;
    for (uint32_t j = 0; j < total; j++)
      if (counts_host[j] != 0) {
        live_rows.push_back(ids_host[j]);
        live_w.push_back((float)counts_host[j]);
      }
    const bool fall = live_rows.size() < K;
    if (verbosity > 0)
      printf("k-means||: %u candidates, %zu live%s\n", total, live_rows.size(),
             fall ? " -- fewer than the clusters: plain k-means++ on the rows" : "");

    // ---- the K seeds: the library's weighted k-means++ over the live candidates (tolerance 1: no Lloyd iteration runs
    //      on them), or plain k-means++ over the rows.  Either way one public call on device buffers of the rows' dtype.
    const size_t esz = fp16 ? sizeof(uint16_t) : sizeof(float);
    void *cen_dev = centroids;
    if (host) {
      char *c = nullptr;
      KNN_TRY(w.alloc(&c, (size_t)K * D * esz));
      cen_dev = c;
    }
    const uint16_t feat = (uint16_t)(fp16 ? D / 2 : D);   // kmeans_cuda counts half2 pairs
    int rc;
    if (!fall) {
      const uint32_t L = (uint32_t)live_rows.size();
      uint32_t *live_dev = nullptr, *asg_l = nullptr;
      float *w_dev = nullptr;
      char *rows_l = nullptr;
      KNN_TRY(w.alloc(&live_dev, L));
      KNN_TRY(w.alloc(&asg_l, L));
      KNN_TRY(w.alloc(&w_dev, L));
      KNN_TRY(w.alloc(&rows_l, (size_t)L * D * esz));
      KMX_HIPCP(hipMemcpyAsync(live_dev, live_rows.data(), (size_t)L * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      KMX_HIPCP(hipMemcpyAsync(w_dev, live_w.data(), (size_t)L * sizeof(float), hipMemcpyHostToDevice, st));
      KMX_HIPRT(launch_seed_par_gather(fp16 ? nullptr : rows32, rows16, live_dev, L, D,
                                       fp16 ? nullptr : reinterpret_cast<float *>(rows_l), fp16 ? rows_l : nullptr, st));
      KMX_HIPRT(hipStreamSynchronize(st));
      rc = kmamd_kmeans_weighted(kmcudaInitMethodPlusPlus, nullptr, 1.f, 0.f, metric, L, feat, K, seed, 1u << device,
                                 device, fp16 ? 1 : 0, verbosity, reinterpret_cast<const float *>(rows_l),
                                 static_cast<float *>(cen_dev), asg_l, nullptr, w_dev);
    } else {
      KMX_HIPRT(hipStreamSynchronize(st));
      rc = kmamd_kmeans_weighted(kmcudaInitMethodPlusPlus, nullptr, 1.f, 0.f, metric, N, feat, K, seed, 1u << device,
                                 device, fp16 ? 1 : 0, verbosity,
                                 fp16 ? reinterpret_cast<const float *>(rows16) : rows32,
                                 static_cast<float *>(cen_dev), asg, nullptr, nullptr);
    }
    g_verbosity = verbosity;
    if (rc != 0) return rc;
    (void)hipSetDevice(device);
    if (host) {
      KMX_HIPCP(hipMemcpyAsync(centroids, cen_dev, (size_t)K * D * esz, hipMemcpyDeviceToHost, st));
      KMX_HIPRT(hipStreamSynchronize(st));
    }
    clock.lap("k-means|| round %u %s", rounds, fall ? "k-means++ on the rows" : "recluster");

    // ---- the optional reports (host memory, whatever device_ptrs says) ----
    const uint32_t ncopy = total < capacity ? total : capacity;
    if (cand_rows) memcpy(cand_rows, ids_host.data(), (size_t)ncopy * sizeof(uint32_t));
    if (cand_counts) memcpy(cand_counts, counts_host.data(), (size_t)ncopy * sizeof(uint32_t));
    if (n_candidates) *n_candidates = total;
    if (round_ends) memcpy(round_ends, ends.data(), ends.size() * sizeof(uint32_t));
    if (fell_back) *fell_back = fall ? 1 : 0;
    return kmcudaSuccess;
  }
};

}  // namespace

extern "C" {

int kmamd_kmeans_seed_parallel(int metric, uint32_t samples_size, uint16_t features_size, uint32_t clusters_size,
                               uint32_t rounds, float oversampling, uint32_t seed, int device, int32_t device_ptrs,
                               int32_t fp16x2, int32_t verbosity, const void *samples, void *centroids,
                               uint32_t *candidate_rows, uint32_t *candidate_counts, uint32_t candidate_capacity,
                               uint32_t *n_candidates, uint32_t *round_ends, int32_t *fell_back) {
  // ---- everything that is refused is refused here, before any device work, with the outputs untouched ----
  if (samples_size == 0 || clusters_size < 2 || clusters_size > samples_size) return kmcudaInvalidArguments;
  if (rounds > 64) return kmcudaInvalidArguments;
  if (!(oversampling >= 0.f) || isinf(oversampling)) return kmcudaInvalidArguments;   // (NaN fails the first test)
  if (!samples || !centroids) return kmcudaInvalidArguments;
  KNN_TRY(rows_call_begin(metric, features_size, fp16x2, device, device_ptrs, verbosity, 31));
  if (device_ptrs >= 0) (void)hipDeviceSynchronize();   // the caller's writes, as kmamd_kmeans_assign
  SeedParJob job;
  job.metric = metric; job.device = device; job.verbosity = verbosity;
  job.fp16 = fp16x2 != 0; job.host = device_ptrs < 0;
  job.N = samples_size; job.D = features_size; job.K = clusters_size;
  job.rounds = rounds ? rounds : 5u;
  job.ell = oversampling != 0.f ? oversampling : 2.f * (float)clusters_size;
  job.seed = seed;
  job.samples = samples; job.centroids = centroids;
  job.cand_rows = candidate_rows; job.cand_counts = candidate_counts; job.capacity = candidate_capacity;
  job.n_candidates = n_candidates; job.round_ends = round_ends; job.fell_back = fell_back;
  return job.run();
}

}  // extern "C"
