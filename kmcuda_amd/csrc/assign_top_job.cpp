// assign_top_job.cpp -- kmamd_kmeans_assign_top of include/kmcuda_amd.h: for every row its m nearest centroids in the
// order one assignment pass would find them, with the reference's distances.
//
// The rows go through in chunks (host_job.hpp: assign_chunk_rows, RowStage): the kernels of assign_top.hip, copy out.
// The centroids are prepared once per call (launch_centroid_prep: exact squared norms, the transposed panel, the centred
// panel and its bound).  Rows of up to 256 features take the filtered path, a sub-chunk's score matrix at a time
// (budgeted like the k-NN search's bound matrix); wider rows, KMCUDA_AMD_ASSIGN_TOP=exact and the rows the filter hands
// over take the exhaustive kernel.
// The centroid preparation and the per-chunk ranking are AssignTopRanker's two halves (knn_host.hpp): the k-NN index
// prepares once and ranks the chunks of its probed queries with them (knn_index.cpp).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

#include "../../include/kmcuda_amd.h"
#include "knn_host.hpp"

using namespace kmx;

namespace {
constexpr size_t kTopScoreBytes = (size_t)256 << 20;   // a sub-chunk's score matrix
}  // namespace

namespace kmx {

bool assign_top_exact_only() {
  const char *v = getenv("KMCUDA_AMD_ASSIGN_TOP");
  return v && strcmp(v, "exact") == 0;
}

int AssignTopRanker::prepare(DeviceArena &w, int metric_, const float *cen_, uint32_t K_, uint32_t D_, bool exact_only) {
  metric = metric_; cen = cen_; K = K_; D = D_;
  const hipStream_t st = w.stream;
  K_pad = (K + 31) / 32 * 32; Kt = (K + 63) / 64 * 64;
  DP = exact_only ? 0 : filter_dp_for(D);
  // (128 rows of scores are the least a launch writes: a panel too wide for the budget takes the exact kernel)
  if ((size_t)K_pad * sizeof(float) * 128 > kTopScoreBytes) DP = 0;
  KNN_TRY(w.alloc(&csqr, K));
  KNN_TRY(w.alloc(&ct, (size_t)D * Kt));
  KNN_TRY(w.alloc(&evaluated, 1));
  KMX_HIPRT(hipMemsetAsync(evaluated, 0, sizeof(unsigned long long), st));
  fa = AssignTopFilter{};
  if (DP) {
    float *bias = nullptr, *bias2 = nullptr, *cfil = nullptr, *mu = nullptr;
    uint32_t *finite = nullptr, *stats = nullptr;
    KNN_TRY(w.alloc(&bias, K_pad));
    KNN_TRY(w.alloc(&bias2, K_pad));
    KNN_TRY(w.alloc(&cfil, (size_t)K_pad * DP));
    KNN_TRY(w.alloc(&mu, DP));
    KNN_TRY(w.alloc(&finite, Kt));
    KNN_TRY(w.alloc(&stats, 16));
    KMX_HIPRT(hipMemsetAsync(stats, 0, 16 * sizeof(uint32_t), st));
    KMX_HIPRT(launch_centroid_prep(metric, cen, K, D, K_pad, DP, Kt, csqr, bias, bias2, cfil, ct, mu, false, finite,
                                   stats, nullptr, nullptr, nullptr, st));
    fa.metric = metric; fa.D = D; fa.DP = DP; fa.K = K; fa.K_pad = K_pad;
    fa.centroids = cen; fa.csqr = csqr; fa.cfil = cfil; fa.bias = bias; fa.mu = mu; fa.stats = stats;
    // the coefficient of the filter bound, as the engine's
    fa.eps = (float)(1.02 * ((double)D + 12.0) * ldexp(1.0, -24));
    fa.evaluated = evaluated;
  } else {
    KMX_HIPRT(launch_centroid_rows(metric, cen, K, D, Kt, csqr, ct, st));
  }
  return 0;
}

int AssignTopRanker::reserve(DeviceArena &w, uint32_t Nc) {
  sub = 0;   // rows per score matrix: a multiple of the score kernel's 128-row blocks
  if (!DP) return 0;
  size_t r = kTopScoreBytes / ((size_t)K_pad * sizeof(float)) / 128 * 128;
  if (const char *v = getenv("KMCUDA_AMD_ASSIGN_TOP_ROWS")) {   // (tests: several score matrices per chunk)
    const long long n = atoll(v);
    if (n > 0 && ((size_t)n + 127) / 128 * 128 < r) r = ((size_t)n + 127) / 128 * 128;
  }
  if (r > Nc) r = ((size_t)Nc + 127) / 128 * 128;
  sub = (uint32_t)r;
  KNN_TRY(w.alloc(&fa.scores, (size_t)sub * K_pad));
  KNN_TRY(w.alloc(&fa.meta, sub));
  KNN_TRY(w.alloc(&fa.fb_rows, Nc));
  KNN_TRY(w.alloc(&fa.fb_count, 1));
  return 0;
}

int AssignTopRanker::rank(const float *rows, uint32_t n, uint32_t m, uint32_t *top, bool exact_only, hipStream_t st) {
  if (DP && !exact_only) {
    fa.m = m;
    KMX_HIPRT(hipMemsetAsync(fa.fb_count, 0, sizeof(uint32_t), st));
    for (uint32_t r0 = 0; r0 < n; r0 += sub) {
      const uint32_t nr = n - r0 < sub ? n - r0 : sub;
      KMX_HIPRT(launch_assign_top_filter(fa, rows + (size_t)r0 * D, nr, r0, top + (size_t)r0 * m, st));
    }
    KMX_HIPRT(launch_assign_top_exact(metric, rows, n, D, ct, csqr, K, Kt, m, fa.fb_rows, fa.fb_count, top, evaluated, st));
  } else {
    KMX_HIPRT(launch_assign_top_exact(metric, rows, n, D, ct, csqr, K, Kt, m, nullptr, nullptr, top, evaluated, st));
  }
  return 0;
}

}  // namespace kmx

namespace {

std::mutex g_top_stats_mutex;
uint64_t g_top_pairs_exact = 0, g_top_pairs_total = 0;

struct AssignTopJob {
  int metric = 0, device = 0, verbosity = 0;
  bool fp16 = false, host = true;
  uint32_t N = 0, D = 0, K = 0, m = 0;
  const void *samples = nullptr, *centroids_in = nullptr;
  uint32_t *top = nullptr;
  float *distances = nullptr;
  uint64_t evaluated_host = 0;

  int run() {
    const size_t chunk = assign_chunk_rows(D);
    const bool exact_only = assign_top_exact_only();

    DeviceArena w;   // owns the call's buffers and its pooled stream
    w.dev = device;
    w.stream = pooled_stream_acquire(device);
    if (!w.stream) return kmcudaRuntimeError;
    const hipStream_t st = w.stream;

    // ---- the centroids, fp32 on this device ----
    RowStage cstage, rstage;
    const float *cen = nullptr;
    KNN_TRY(cstage.reserve(w, K, D, fp16, host));
    KNN_TRY(cstage.stage(centroids_in, 0, K, &cen));

    // ---- their preparation: csqr and the transposed panel for the exact keys, the centred panel for the filter ----
    AssignTopRanker r;
    KNN_TRY(r.prepare(w, metric, cen, K, D, exact_only));
    unsigned long long *evaluated = r.evaluated;
    const uint32_t DP = r.DP;

    // ---- one chunk's buffers, reused by every chunk ----
    const uint32_t Nc = (uint32_t)(chunk < N ? chunk : N);
    float *dist_buf = nullptr;
    uint32_t *top_buf = nullptr;
    KNN_TRY(rstage.reserve(w, Nc, D, fp16, host));
    if (host) KNN_TRY(w.alloc(&top_buf, (size_t)Nc * m));
    if (host && distances) KNN_TRY(w.alloc(&dist_buf, (size_t)Nc * m));
    KNN_TRY(r.reserve(w, Nc));

    for (uint32_t q0 = 0; q0 < N; q0 += Nc) {
      const uint32_t n = N - q0 < Nc ? N - q0 : Nc;
      // ---- the chunk's rows, fp32 on this device ----
      const float *rows = nullptr;
      KNN_TRY(rstage.stage(samples, q0, n, &rows));
      uint32_t *t = host ? top_buf : top + (size_t)q0 * m;
      KNN_TRY(r.rank(rows, n, m, t, false, st));
      float *dist = nullptr;
      if (distances) {
        dist = host ? dist_buf : distances + (size_t)q0 * m;
        KMX_HIPRT(launch_assign_top_distances(metric, rows, n, D, cen, K, m, t, dist, st));
      }
      if (host) {
        KMX_HIPCP(hipMemcpyAsync(top + (size_t)q0 * m, t, (size_t)n * m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (distances)
          KMX_HIPCP(hipMemcpyAsync(distances + (size_t)q0 * m, dist, (size_t)n * m * sizeof(float),
                                   hipMemcpyDeviceToHost, st));
      }
      // (the next chunk overwrites these buffers: the stream orders it behind this one's kernels and copies)
    }
    unsigned long long ev = 0;
    KMX_HIPCP(hipMemcpyAsync(&ev, evaluated, sizeof(ev), hipMemcpyDeviceToHost, st));
    if (hipStreamSynchronize(st) != hipSuccess) {
      if (verbosity > 0) printf("kmamd_kmeans_assign_top failed: %s\n", hipGetErrorString(hipGetLastError()));
      return kmcudaRuntimeError;
    }
    evaluated_host = ev;
    if (verbosity > 1)
      printf("kmamd_kmeans_assign_top: %s path, %llu exact keys of %llu pairs\n", DP ? "filtered" : "exact", ev,
             (unsigned long long)N * K);
    return kmcudaSuccess;
  }
};

}  // namespace

extern "C" {

int kmamd_kmeans_assign_top(int metric, uint32_t samples_size, uint16_t features_size, uint32_t clusters_size,
                            uint32_t m, int device, int32_t device_ptrs, int32_t fp16x2, int32_t verbosity,
                            const void *samples, const void *centroids, uint32_t *top_assignments,
                            float *top_distances) {
  // ---- everything that is refused is refused here, before any device work, with the outputs untouched ----
  if (clusters_size < 2 || clusters_size >= 0x7FFFFFFFu) return kmcudaInvalidArguments;
  if (m < 1 || m > 64 || m > clusters_size) return kmcudaInvalidArguments;
  if (!centroids || (samples_size != 0 && (!samples || !top_assignments))) return kmcudaInvalidArguments;
  KNN_TRY(rows_call_begin(metric, features_size, fp16x2, device, device_ptrs, verbosity));
  uint64_t evaluated = 0;
  if (samples_size != 0) {
    if (device_ptrs >= 0) (void)hipDeviceSynchronize();   // the caller's writes, as kmamd_kmeans_assign
    AssignTopJob job;
    job.metric = metric; job.device = device; job.verbosity = verbosity;
    job.fp16 = fp16x2 != 0; job.host = device_ptrs < 0;
    job.N = samples_size; job.D = features_size; job.K = clusters_size; job.m = m;
    job.samples = samples; job.centroids_in = centroids;
    job.top = top_assignments; job.distances = top_distances;
    const int rc = job.run();
    if (rc != kmcudaSuccess) return rc;
    evaluated = job.evaluated_host;
  }
  std::lock_guard<std::mutex> lock(g_top_stats_mutex);
  g_top_pairs_exact = evaluated;
  g_top_pairs_total = (uint64_t)samples_size * clusters_size;
  return kmcudaSuccess;
}

int kmamd_assign_top_stats(uint64_t *pairs_exact, uint64_t *pairs_total) {
  std::lock_guard<std::mutex> lock(g_top_stats_mutex);
  if (pairs_exact) *pairs_exact = g_top_pairs_exact;
  if (pairs_total) *pairs_total = g_top_pairs_total;
  return kmcudaSuccess;
}

}  // extern "C"
