// knn_host.cpp -- the host pipeline both k-NN entry points run (knn_host.hpp): knn_cuda()'s self-join (knn_job.cpp)
// and the query batches of kmamd_knn_index_* (knn_index.cpp) differ in their query side only.
#include "knn_host.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>

namespace kmx {

KnnSwitches knn_switches() {
  KnnSwitches sw;
  auto on = [](const char *v) { return v && atoi(v) != 0; };
  sw.exact = on(getenv("KMCUDA_AMD_KNN_EXACT"));
  sw.fp16_strict = fp16_strict_requested();
  const char *filter = getenv("KMCUDA_AMD_FILTER");
  sw.filter_f32 = filter && strcmp(filter, "f32") == 0;
  const char *tight = getenv("KMCUDA_AMD_KNN_TIGHT");
  sw.tight = !(tight && atoi(tight) == 0);
  if (const char *order = getenv("KMCUDA_AMD_KNN_ORDER")) sw.order = atoi(order);
  sw.xcd = on(getenv("KMCUDA_AMD_KNN_XCD"));
  sw.stats = getenv("KMCUDA_AMD_KNN_STATS") != nullptr;
  if (const char *only = getenv("KMCUDA_AMD_KNN_SHARD")) {
    unsigned i = 0, n = 0;
    if (sscanf(only, "%u/%u", &i, &n) == 2 && n >= 1 && i < n) {
      sw.shard_i = i;
      sw.shard_n = n;
    }
  }
  if (const char *chunk = getenv("KMCUDA_AMD_KNN_QUERY_CHUNK")) {
    const long v = atol(chunk);
    if (v > 0) sw.query_chunk = (size_t)v;
  }
  if (const char *chunk = getenv("KMCUDA_AMD_KNN_ADD_CHUNK")) {
    const long v = atol(chunk);
    if (v > 0) sw.add_chunk = (size_t)v;
  }
  sw.add_time = on(getenv("KMCUDA_AMD_KNN_ADD_TIME"));
  sw.remove_time = on(getenv("KMCUDA_AMD_KNN_REMOVE_TIME"));
  return sw;
}

KnnPath knn_choose_path(uint32_t D, bool fp16, int verbosity, const KnnSwitches &sw) {
  KnnPath p;
  // KMCUDA_AMD_FP16_STRICT (fp16x2 only): radii, centroid distances and every candidate distance in the reference's
  // half2 arithmetic (knn.hip, half2_ops.hpp) -- the verification mode of half2_strict.hip for this entry point;
  // no matrix-core filter (its bound is stated against the fp32 arithmetic)
  p.strict_h2 = fp16 && sw.fp16_strict;
  if (p.strict_h2 && verbosity > 0) printf("k-NN: the reference's half2 arithmetic (KMCUDA_AMD_FP16_STRICT)\n");
  const bool exact = sw.exact || p.strict_h2;
  p.dp_filter = exact ? 0 : filter_dp_for(D);
  // 256 < D <= 1024: the f16 filter's one-operand-set instantiations (knn_f16.hip: 512 with two blocks per CU;
  // 768 / 1024 with one -- the queries' operands alone are 192 / 256 registers; the f32 filter stops at 256)
  if (!p.dp_filter && !exact && !sw.filter_f32) p.dp_filter = KnnF16Widths::fit(D);
  p.DP = p.dp_filter ? p.dp_filter : D;
  if (!p.dp_filter && verbosity > 0) printf("k-NN: every candidate is evaluated with the exact arithmetic (no matrix-core filter)\n");
  // which matrix-core instruction filters the candidates: f16 on centred hi/lo-split rows (default,
  // needs DP >= 16) or f32 (KMCUDA_AMD_FILTER=f32)
  p.use_f16 = p.dp_filter >= 16 && !sw.filter_f32;
  return p;
}

bool knn_leaves_half_range(bool *use_f16, uint32_t *dp_filter, uint32_t D, uint32_t flag) {
  if (!*use_f16 || !flag) return false;
  *use_f16 = false;
  if (D > 256) *dp_filter = 0;   // (the f32 filter stops at 256 features)
  return true;
}

namespace {

// brings `count` halves of a caller buffer onto the shard's device and widens them to fp32
int stage_in_half(KnnShard &sh, const void *src, size_t count, int32_t device_ptrs, const float **dst) {
  float *buf = nullptr;
  KNN_TRY(sh.alloc(&buf, count));
  const uint16_t *dev_half = nullptr;
  KNN_TRY(sh.stage_in(static_cast<const uint16_t *>(src), count, device_ptrs, &dev_half));
  KMX_HIPRT(launch_half_to_float(dev_half, count, buf, sh.stream));
  *dst = buf;
  return 0;
}

// The f16 filter's centre: mu = mean of the finite centroid rows (any vector works: distances are translation
// invariant), mu_host[0, D) (the rest of it stays as it is: zeros), *mu2 = ||mu||^2 rounded up
int centroid_mean(const KnnCorpus &c, std::vector<float> &mu_host, float *mu2) {
  const uint32_t K = c.K, D = c.D;
  const size_t count = (size_t)K * D, bytes = count * (c.fp16 ? sizeof(uint16_t) : sizeof(float));
  std::vector<float> cen(count);
  std::vector<_Float16> raw(c.fp16 ? count : 0);
  void *dst = c.fp16 ? static_cast<void *>(raw.data()) : static_cast<void *>(cen.data());
  if (c.device_ptrs < 0) memcpy(dst, c.centroids, bytes);
  else KMX_HIPCP(hipMemcpy(dst, c.centroids, bytes, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < raw.size(); i++) cen[i] = (float)raw[i];
  std::vector<double> acc(D, 0.0);
  uint32_t nfin = 0;
  for (uint32_t r = 0; r < K; r++) {
    bool fin = true;
    for (uint32_t f = 0; f < D && fin; f++) fin = std::isfinite(cen[(size_t)r * D + f]);
    if (!fin) continue;
    for (uint32_t f = 0; f < D; f++) acc[f] += cen[(size_t)r * D + f];
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

// one shard's stream, its copy of the caller's buffers and everything the preparation writes
int stage_and_alloc(KnnShard &s, const KnnCorpus &c, const KnnPath &path, bool keep_plain,
                    const std::vector<float> &mu_host, float mu2) {
  const uint32_t N = c.N, D = c.D, K = c.K, DP = path.DP;
  s.metric = c.metric; s.N = N; s.D = D; s.DP = DP; s.K = K; s.mu2 = mu2;
  if (hipSetDevice(s.dev) != hipSuccess) return kmcudaNoSuchDevice;
  if (!(s.stream = pooled_stream_acquire(s.dev))) return kmcudaRuntimeError;
  if (c.fp16) {  // half buffers -> fp32 working copies (fp32 arithmetic on the half values)
    KNN_TRY(stage_in_half(s, c.samples, (size_t)N * D, c.device_ptrs, &s.samples));
    KNN_TRY(stage_in_half(s, c.centroids, (size_t)K * D, c.device_ptrs, &s.centroids));
  } else {
    KNN_TRY(s.stage_in(static_cast<const float *>(c.samples), (size_t)N * D, c.device_ptrs, &s.samples));
    KNN_TRY(s.stage_in(static_cast<const float *>(c.centroids), (size_t)K * D, c.device_ptrs, &s.centroids));
  }
  KNN_TRY(s.stage_in(c.assignments, (size_t)N, c.device_ptrs, &s.assignments));
  KNN_TRY(s.alloc(&s.xs, (size_t)N * DP));
  KNN_TRY(s.alloc(&s.n2s, N));
  KNN_TRY(s.alloc(&s.mydist, N));
  KNN_TRY(s.alloc(&s.rdist, N));
  KNN_TRY(s.alloc(&s.R, K));
  KNN_TRY(s.alloc(&s.C, (size_t)K * K));
  KNN_TRY(s.alloc(&s.inv, N));
  KNN_TRY(s.alloc(&s.offsets, (size_t)K + 2));
  KNN_TRY(s.alloc(&s.scratch.keys_tmp, N));
  KNN_TRY(s.alloc(&s.scratch.vals_tmp, N));
  KNN_TRY(s.alloc(&s.scratch.keys_sorted, N));
  KNN_TRY(s.alloc(&s.stats, 4));
  KNN_TRY(s.alloc(&s.calced, KNN_STATS));
  if (path.use_f16) {
    KNN_TRY(s.alloc(&s.xs16, ((size_t)N + KNN16_PAD_ROWS) * DP));
    KNN_TRY(s.alloc(&s.kbias, (size_t)N + KNN16_PAD_ROWS));
    KNN_TRY(s.alloc(&s.mu, DP));
    KNN_TRY(s.alloc(&s.mux, N));
    s.n2c = s.n2s;
    s.stats_c = s.stats;
    if (keep_plain) {
      KNN_TRY(s.alloc(&s.n2c, N));
      KNN_TRY(s.alloc(&s.stats_c, 4));   // (only word 0, the maximum, is ever written or read: the flag stays stats[1])
    }
    KMX_HIPCP(hipMemcpyAsync(s.mu, mu_host.data(), DP * sizeof(float), hipMemcpyHostToDevice, s.stream));
  }
  s.scratch.sort_bytes = sort_temp_bytes(N, K);
  char *t = nullptr;
  KNN_TRY(s.alloc(&t, s.scratch.sort_bytes + 16));
  s.scratch.sort_temp = t;
  return 0;
}

}  // namespace

int knn_prepare_corpus(KnnShard *const *shards, size_t nshards, const KnnCorpus &c, bool keep_plain, KnnPath *path,
                       bool *left_half_range, uint32_t *offsets_host) {
  const uint32_t N = c.N, D = c.D, K = c.K, DP = path->DP;
  const bool f16 = path->use_f16;
  std::vector<float> mu_host(DP, 0.f);
  float mu2 = 0.f;
  if (f16) KNN_TRY(centroid_mean(c, mu_host, &mu2));
  for (size_t i = 0; i < nshards; i++) KNN_TRY(stage_and_alloc(*shards[i], c, *path, keep_plain, mu_host, mu2));
  // The corpus in cluster-sorted order: the CSR of the assignments (inv, offsets), the DP-padded fp32 copy xs, its
  // plain squared norms and their maximum (stats[0]); with the f16 filter (mu) also the half-range flag stats[1]
  for (size_t i = 0; i < nshards; i++) {
    KnnShard &s = *shards[i];
    (void)hipSetDevice(s.dev);
    KMX_HIPRT(hipMemsetAsync(s.calced, 0, KNN_STATS * sizeof(unsigned long long), s.stream));
    const KnnScratch &x = s.scratch;
    KMX_HIPRT(launch_inverse_assignments(s.assignments, N, K, x.keys_tmp, x.vals_tmp, x.keys_sorted, s.inv, s.offsets,
                                         x.sort_temp, x.sort_bytes, s.stream));
    KMX_HIPRT(launch_knn_gather(s.samples, N, D, DP, s.inv, s.xs, s.n2s, s.stats, f16 ? s.mu : nullptr, s.offsets, K,
                                s.stream));
    // radii, member distances, centroid distances
    KMX_HIPRT(launch_knn_prep(c.metric, s.xs, N, D, DP, s.offsets, K, s.centroids, s.mydist, s.rdist, s.R, s.C,
                              path->strict_h2, s.stream));
  }
  // every shard holds the same corpus: the first one's flag and offsets speak for all
  uint32_t flag = 0;
  if (f16 || offsets_host) {
    KnnShard &s = *shards[0];
    (void)hipSetDevice(s.dev);
    if (offsets_host)
      KMX_HIPCP(hipMemcpyAsync(offsets_host, s.offsets, ((size_t)K + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
    if (f16) KMX_HIPCP(hipMemcpyAsync(&flag, s.stats + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
    KMX_HIPRT(hipStreamSynchronize(s.stream));
  }
  *left_half_range = knn_leaves_half_range(&path->use_f16, &path->dp_filter, D, flag);
  if (path->use_f16) {  // after the radii / member distances, which read the plain norms
    for (size_t i = 0; i < nshards; i++) {
      KnnShard &s = *shards[i];
      (void)hipSetDevice(s.dev);
      KMX_HIPRT(launch_knn_split(c.metric, s.xs, N, D, DP, s.mu, s.xs16, s.n2c, s.mux, s.kbias, s.stats_c, s.stream));
    }
  }
  return 0;
}

void knn_block_plan(const uint32_t *offsets, uint32_t K, uint32_t qpb, std::vector<uint32_t> *plan) {
  plan->clear();
  for (uint32_t c = 0; c < K; c++)
    for (uint32_t p = offsets[c]; p < offsets[c + 1]; p += qpb) {
      plan->push_back(c);
      plan->push_back(p);
    }
}

// An experiment that lost, off by default: the blocks of one query cluster -- which visit the same candidate clusters
// in the same order, 512 bytes per candidate and block: 4.3 TB of fetches for config D's share -- dispatched to ONE
// XCD (workgroup indices congruent mod 8), cluster after cluster, so that an XCD's L2 holds two or three such streams
// instead of sixteen and a stream's followers hit the tiles its leader has just fetched.  Measured: FETCH_SIZE 4.17 TB
// against 4.27, knn_cuda 1.13-1.15 s against 1.11-1.13 (profiles/r5d_knn_dispatch_order_ab.log): the blocks of a
// stream drift further apart than an L2 holds (a cluster's slab alone is 4 MB).  Slots a shorter list leaves empty
// carry the marker 0xFFFFFFFF (the kernel returns at once).  Only the order of independent blocks changes: the lists
// are the same.
std::vector<uint32_t> knn_xcd_plan(const std::vector<uint32_t> &plan) {
  constexpr uint32_t kXcds = 8;
  const uint32_t nblocks = (uint32_t)(plan.size() / 2);
  std::vector<std::vector<uint32_t>> lists(kXcds);   // block numbers (into plan) per XCD
  uint32_t b = 0;
  while (b < nblocks) {
    uint32_t e = b;
    while (e < nblocks && plan[2 * (size_t)e] == plan[2 * (size_t)b]) e++;   // one cluster's blocks
    uint32_t best = 0;
    for (uint32_t x = 1; x < kXcds; x++)
      if (lists[x].size() < lists[best].size()) best = x;
    for (uint32_t q = b; q < e; q++) lists[best].push_back(q);
    b = e;
  }
  size_t longest = 0;
  for (auto &l : lists) longest = l.size() > longest ? l.size() : longest;
  std::vector<uint32_t> ordered(2 * kXcds * longest, 0xFFFFFFFFu);
  for (uint32_t x = 0; x < kXcds; x++)
    for (size_t i = 0; i < lists[x].size(); i++) {
      ordered[2 * (kXcds * i + x)] = plan[2 * (size_t)lists[x][i]];
      ordered[2 * (kXcds * i + x) + 1] = plan[2 * (size_t)lists[x][i] + 1];
    }
  return ordered;
}

void knn_corpus_args(const KnnShard &s, bool f16, const float *R, KnnArgs *a) {
  a->xs = s.xs; a->n2s = f16 ? s.n2c : s.n2s; a->inv = s.inv; a->offsets = s.offsets; a->mydist = s.mydist; a->R = R;
  a->C = s.C; a->stats = f16 ? s.stats_c : s.stats; a->N = s.N; a->D = s.D; a->DP = s.DP; a->K = s.K;
  a->eps = (float)(1.02 * ((double)s.D + 12.0) * ldexp(1.0, -24));  // the filters' slack, as the Lloyd filter
  a->calced = s.calced;
  a->xs16 = s.xs16; a->mux = s.mux; a->kbias = s.kbias; a->mu2 = s.mu2;
}

int knn_bound_queries(const KnnShard &s, const KnnScratch &x, const float *qxs, const uint32_t *qoffsets,
                      const float *qmydist, uint32_t p_base, uint32_t p_end, const float *R, int order, KnnArgs *a) {
  const uint32_t len = p_end - p_base;
  KMX_HIPRT(launch_knn_centroid_bounds(qxs, s.D, s.DP, p_base, p_end, s.centroids, s.K, R, x.lb, len, s.stream));
  a->lb = x.lb;
  a->lb_stride = len;
  // queries that want the same clusters into the same waves (update.hip: launch_knn_query_order): by the other
  // cluster that can come closest, then by their distance to their own centroid (mode 3); KMCUDA_AMD_KNN_ORDER=0:
  // sorted-position order, 1: the closest other cluster alone, 2: the distance alone
  // (A/B: 1.911 / 1.882 / 1.860 / 1.839e12 pairs scored for config D's share, profiles/r6aj_*)
  if (order != 0 && x.qperm) {
    if (launch_knn_query_order(x.lb, len, qoffsets, s.K, p_base, p_end, x.keys_tmp, x.vals_tmp, x.keys_sorted, x.qperm,
                               x.sort_temp, x.sort_bytes, s.stream, order, qmydist, R))
      a->qperm = x.qperm;
    else
      (void)hipGetLastError();
  }
  return 0;
}

int knn_search(const KnnShard &s, KnnScratch &x, KnnArgs a, const KnnPath &path, const KnnSwitches &sw,
               uint32_t nblocks, bool self, int verbosity, const KnnProbeOrder *probe_order) {
  const bool f16 = path.use_f16;
  const bool probe = a.plist != nullptr;
  const bool mask = a.allow_bits != nullptr;   // (the caller's a.R then: the radii over the allowed rows)
  const hipStream_t st = s.stream;
  if ((probe || mask) && (self || (path.dp_filter && !f16))) return kmcudaInvalidArguments;
  if (mask && (!a.allow_count || !a.R)) return kmcudaInvalidArguments;
  const float *const R = mask ? a.R : s.R;
  knn_corpus_args(s, f16, R, &a);
  const uint32_t len = a.p_end - a.p_base;
  // (the query order is an optimisation: sorted-position order without its buffer)
  auto want_qperm = [&]() {
    if (sw.order != 0 && !x.qperm && hipMalloc((void **)&x.qperm, x.rows * sizeof(uint32_t)) != hipSuccess) {
      x.qperm = nullptr;
      (void)hipGetLastError();
    }
    return sw.order != 0 && x.qperm;
  };
  if (probe) {
    // Probe mode: no second cluster test -- the probed clusters are the nearest ones, where it rarely
    // fires, and its table is K floats per query.  The queries of a cluster go into waves by the second entry of their
    // raw lists instead.
    if (f16 && len != 0 && probe_order && a.pw >= 2 && want_qperm()) {
      if (launch_knn_probe_order(probe_order->raw, a.pw, probe_order->qinv, a.qoffsets, s.K, a.p_base, a.p_end, x.keys_tmp,
                                 x.vals_tmp, x.keys_sorted, x.qperm, x.sort_temp, x.sort_bytes, st))
        a.qperm = x.qperm;
      else
        (void)hipGetLastError();
    }
  } else if (f16 && s.metric == 0 && s.D <= 1024 && len != 0 && sw.tight) {
    // The tighter cluster test of the f16 search (knn_f16.hip: the query's own distance to every centroid instead of
    // the triangle bound for it).  4 K bytes per query; without that memory, or with KMCUDA_AMD_KNN_TIGHT=0, the
    // reference's prune test decides alone.  Same neighbour lists either way.
    if (!x.lb && hipMalloc((void **)&x.lb, (size_t)s.K * x.rows * sizeof(float)) != hipSuccess) {
      x.lb = nullptr;
      (void)hipGetLastError();
      if (verbosity > 1) printf("k-NN: no memory for the per-query centroid bounds, the reference's prune test alone\n");
    } else {
      KNN_TRY(knn_bound_queries(s, x, self ? s.xs : a.qxs, self ? s.offsets : a.qoffsets, self ? s.mydist : a.qmydist,
                                a.p_base, a.p_end, R, want_qperm() ? sw.order : 0, &a));
    }
  }
  KMX_HIPRT(!path.dp_filter ? launch_knn_exact(s.metric, a, path.strict_h2, st, self, probe, mask)
            : f16           ? launch_knn_filter_f16(s.metric, a, nblocks, st, self, probe, mask)
                            : launch_knn_filter(s.metric, a, nblocks, st, self));
  return 0;
}

int knn_scatter_on(int dev, int src_dev, const uint32_t *out, const uint32_t *inv, uint32_t N, uint32_t p_base,
                   uint32_t p_end, uint32_t k, uint32_t *neighbors) {
  struct Tmp {   // a copy on `dev`, freed on every way out
    uint32_t *p = nullptr;
    ~Tmp() { if (p) (void)hipFree(p); }
  } tmp_out, tmp_inv;
  const size_t out_bytes = (size_t)(p_end - p_base) * k * sizeof(uint32_t), inv_bytes = (size_t)N * sizeof(uint32_t);
  (void)hipSetDevice(dev);
  if (!out || src_dev != dev) {
    if (hipMalloc((void **)&tmp_out.p, out_bytes) != hipSuccess) return kmcudaMemoryAllocationFailure;
    if (!out) KMX_HIPRT(hipMemset(tmp_out.p, 0xFF, out_bytes));
    else KMX_HIPCP(hipMemcpyPeer(tmp_out.p, dev, out, src_dev, out_bytes));
    out = tmp_out.p;
  }
  if (src_dev != dev) {
    if (hipMalloc((void **)&tmp_inv.p, inv_bytes) != hipSuccess) return kmcudaMemoryAllocationFailure;
    KMX_HIPCP(hipMemcpyPeer(tmp_inv.p, dev, inv, src_dev, inv_bytes));
    inv = tmp_inv.p;
  }
  KMX_HIPRT(launch_knn_scatter(out, inv, p_base, p_end, k, neighbors, nullptr));
  KMX_HIPRT(hipDeviceSynchronize());
  return 0;
}

}  // namespace kmx
