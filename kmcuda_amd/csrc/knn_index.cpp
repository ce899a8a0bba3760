// knn_index.cpp -- k nearest neighbours of NEW rows (queries) among a clustered corpus: kmamd_knn_index_* of
// include/kmcuda_amd.h.
//
// knn_cuda() answers the self-join only (every corpus row against the others, the row itself skipped: knn.cu:204-206).
// Here the corpus is prepared ONCE per index -- the cluster-sorted fp32 copy, the f16 split, radii, the K x K centroid
// distances, mu and the stats, exactly as knn_cuda() prepares it (knn_host.hpp) -- and every query batch runs the same
// search kernels in their query mode (SELF = false: the query side from its own buffers, KnnArgs::q*).  A query's list
// is what the reference's procedure gives for it as one more row of its cluster c_q, without the self-skip (DESIGN.md
// 4.8): own cluster in ascending corpus order, then the other clusters in ascending id under the triangle prune, push
// iff distance <= kth, output popped from the heap.  c_q is its nearest centroid (kmamd_lloyd_assign's arithmetic and
// tie rule) unless the caller passes one; any cluster id gives the same lists (the prune is rigorous), only the work
// differs.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../include/kmcuda.h"
#include "../../include/kmcuda_amd.h"
#include "engine.hpp"
#include "knn_host.hpp"

using namespace kmx;

#define RETERR(call) do { int rc__ = (call); if (rc__ != 0) return rc__; } while (false)
#define KMX_HIPRT(call) do { if ((call) != hipSuccess) return kmcudaRuntimeError; } while (false)
#define KMX_HIPCP(call) do { if ((call) != hipSuccess) return kmcudaMemoryCopyError; } while (false)

namespace {

// lb (K floats per query) and the heaps (2k floats per query) of one chunk of queries stay within this budget
constexpr size_t kQueryChunkBytes = (size_t)4 << 30;

class KnnIndex {
 public:
  KnnShard s;   // the prepared corpus (its buffers and stream)
  KnnPath path;
  int metric = 0, verbosity = 0;
  bool fp16 = false;
  uint32_t N = 0, D = 0, K = 0;
  float mu2 = 0.f;
  float *n2c = nullptr;           // centred squared norms (f16 filter); s.n2s keeps the plain ones (f32 filter)
  uint32_t *stats_plain = nullptr;   // [0] max plain squared norm (the f32 filter's bound); s.stats[0]: the centred one

  int build(int device, int metric_, int fp16x2, uint32_t N_, uint32_t D_, uint32_t K_, const void *samples,
            const void *centroids, const uint32_t *assignments, int32_t device_ptrs, int verbosity_) {
    metric = metric_; fp16 = fp16x2 != 0; N = N_; D = D_; K = K_; verbosity = verbosity_;
    path = knn_choose_path(D, fp16, verbosity);
    const uint32_t DP = path.DP;
    std::vector<float> mu_host(DP, 0.f);
    if (path.use_f16) RETERR(knn_centroid_mean(centroids, K, D, fp16, device_ptrs, mu_host, &mu2));
    s.dev = device;
    if (hipSetDevice(device) != hipSuccess) return kmcudaNoSuchDevice;
    if (!(s.stream = pooled_stream_acquire(device))) return kmcudaRuntimeError;
    if (fp16) {
      RETERR(stage_in_half(s, samples, (size_t)N * D, device_ptrs, &s.samples));
      RETERR(stage_in_half(s, centroids, (size_t)K * D, device_ptrs, &s.centroids));
    } else {
      RETERR(s.stage_in(static_cast<const float *>(samples), (size_t)N * D, device_ptrs, &s.samples));
      RETERR(s.stage_in(static_cast<const float *>(centroids), (size_t)K * D, device_ptrs, &s.centroids));
    }
    if (!fp16 && device_ptrs == device) {   // the caller's centroids may change after this call: the index keeps a copy
      float *cen = nullptr;
      RETERR(s.alloc(&cen, (size_t)K * D));
      KMX_HIPCP(hipMemcpyAsync(cen, s.centroids, (size_t)K * D * sizeof(float), hipMemcpyDeviceToDevice, s.stream));
      s.centroids = cen;
    }
    RETERR(s.stage_in(assignments, (size_t)N, device_ptrs, &s.assignments));
    RETERR(s.alloc(&s.xs, (size_t)N * DP));
    RETERR(s.alloc(&s.n2s, N));
    RETERR(s.alloc(&s.mydist, N));
    RETERR(s.alloc(&s.rdist, N));
    RETERR(s.alloc(&s.R, K));
    RETERR(s.alloc(&s.C, (size_t)K * K));
    RETERR(s.alloc(&s.inv, N));
    RETERR(s.alloc(&s.offsets, (size_t)K + 2));
    RETERR(s.alloc(&s.keys_tmp, N));
    RETERR(s.alloc(&s.vals_tmp, N));
    RETERR(s.alloc(&s.keys_sorted, N));
    RETERR(s.alloc(&s.stats, 4));
    RETERR(s.alloc(&stats_plain, 4));
    RETERR(s.alloc(&s.calced, KNN_STATS));
    if (path.use_f16) {
      RETERR(s.alloc(&s.xs16, ((size_t)N + KNN16_PAD_ROWS) * DP));
      RETERR(s.alloc(&s.kbias, (size_t)N + KNN16_PAD_ROWS));
      RETERR(s.alloc(&s.mu, DP));
      RETERR(s.alloc(&s.mux, N));
      RETERR(s.alloc(&n2c, N));
      KMX_HIPCP(hipMemcpyAsync(s.mu, mu_host.data(), DP * sizeof(float), hipMemcpyHostToDevice, s.stream));
    }
    const size_t sort_bytes = sort_temp_bytes(N, K);
    char *t = nullptr;
    RETERR(s.alloc(&t, sort_bytes + 16));
    s.sort_temp = t;
    RETERR(knn_sort_and_gather(s, N, D, DP, K, path.use_f16, sort_bytes));
    KMX_HIPRT(launch_knn_prep(metric, s.xs, N, D, DP, s.offsets, K, s.centroids, s.mydist, s.rdist, s.R, s.C,
                              path.strict_h2, s.stream));
    KMX_HIPCP(hipMemcpyAsync(stats_plain, s.stats, 2 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s.stream));
    uint32_t overflow = 0;
    if (path.use_f16) {
      KMX_HIPCP(hipMemcpyAsync(&overflow, s.stats + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
      KMX_HIPRT(hipStreamSynchronize(s.stream));
    }
    if (overflow) {   // a centred corpus row leaves the half range -- no f16 filter for this index
      path.use_f16 = false;
      if (D > 256) path.dp_filter = 0;
      if (verbosity > 0)
        printf("k-NN index: a centred row leaves the half range, %s\n",
               path.dp_filter ? "the f32 matrix-core filter instead of the f16 one" : "every candidate is evaluated exactly");
    } else if (path.use_f16) {
      KMX_HIPRT(launch_knn_split(metric, s.xs, N, D, DP, s.mu, s.xs16, n2c, s.mux, s.kbias, s.stats, s.stream));
    }
    KMX_HIPRT(hipStreamSynchronize(s.stream));
    // what the searches no longer read
    s.release(s.samples);
    s.release(s.assignments);
    s.release(s.rdist);
    s.release(s.keys_tmp);
    s.release(s.vals_tmp);
    s.release(s.keys_sorted);
    s.release(s.sort_temp);
    s.samples = nullptr; s.assignments = nullptr; s.rdist = nullptr; s.keys_tmp = s.vals_tmp = s.keys_sorted = nullptr;
    s.sort_temp = nullptr;
    return 0;
  }

  int query(uint32_t k, uint32_t Q, const void *queries, const uint32_t *qassign_in, uint32_t *neighbors,
            float *distances, uint32_t *qassign_out, int32_t device_ptrs);
};

// One query batch, in chunks of at most `chunk` queries; every buffer is sized for one chunk and reused.
int KnnIndex::query(uint32_t k, uint32_t Q, const void *queries, const uint32_t *qassign_in, uint32_t *neighbors,
                    float *distances, uint32_t *qassign_out, int32_t device_ptrs) {
  if (Q == 0) return 0;
  if (hipSetDevice(s.dev) != hipSuccess) return kmcudaNoSuchDevice;
  const uint32_t DP = path.DP;
  const hipStream_t st = s.stream;
  size_t chunk = kQueryChunkBytes / (4 * ((size_t)K + 2 * (size_t)k));
  if (const char *ce = getenv("KMCUDA_AMD_KNN_QUERY_CHUNK")) {   // test hook: queries per chunk
    const long v = atol(ce);
    if (v > 0) chunk = (size_t)v;
  }
  if (chunk < 1) chunk = 1;
  const uint32_t Qc = (uint32_t)(chunk < Q ? chunk : Q);
  const bool host = device_ptrs < 0;
  const bool tight_ok = metric == 0 && D <= 1024 && !(getenv("KMCUDA_AMD_KNN_TIGHT") && atoi(getenv("KMCUDA_AMD_KNN_TIGHT")) == 0);
  const char *ord = getenv("KMCUDA_AMD_KNN_ORDER");
  const int ord_mode = ord ? atoi(ord) : 3;

  // per-call buffers (freed with `w`)
  KnnShard w;
  w.dev = s.dev;
  w.stream = nullptr;   // (enqueues on the index's stream; nothing to release)
  float *qrows = nullptr, *qxs = nullptr, *qn2p = nullptr, *qn2c = nullptr, *qmydist = nullptr, *qrdist = nullptr,
        *qmux = nullptr, *qkbias = nullptr, *heaps = nullptr, *outd = nullptr, *lb = nullptr, *dist_dev = nullptr;
  uint16_t *qhalf = nullptr, *qxs16 = nullptr;
  uint32_t *qassign = nullptr, *qprev = nullptr, *qeff = nullptr, *qinv = nullptr, *qoffsets = nullptr, *keys_tmp = nullptr,
           *vals_tmp = nullptr, *keys_sorted = nullptr, *qstats = nullptr, *blocks = nullptr, *out = nullptr, *qperm = nullptr,
           *nb_dev = nullptr;
  RETERR(w.alloc(&qrows, (size_t)Qc * D));
  if (fp16) RETERR(w.alloc(&qhalf, (size_t)Qc * D));
  RETERR(w.alloc(&qassign, Qc));
  RETERR(w.alloc(&qprev, Qc));
  RETERR(w.alloc(&qeff, Qc));
  RETERR(w.alloc(&qinv, Qc));
  RETERR(w.alloc(&qoffsets, (size_t)K + 2));
  RETERR(w.alloc(&keys_tmp, Qc));
  RETERR(w.alloc(&vals_tmp, Qc));
  RETERR(w.alloc(&keys_sorted, Qc));
  RETERR(w.alloc(&qstats, 4));
  RETERR(w.alloc(&qxs, (size_t)Qc * DP));
  RETERR(w.alloc(&qn2p, Qc));
  RETERR(w.alloc(&qmydist, Qc));
  RETERR(w.alloc(&qrdist, Qc));
  if (path.use_f16) {
    RETERR(w.alloc(&qxs16, ((size_t)Qc + KNN16_PAD_ROWS) * DP));
    RETERR(w.alloc(&qn2c, Qc));
    RETERR(w.alloc(&qmux, Qc));
    RETERR(w.alloc(&qkbias, (size_t)Qc + KNN16_PAD_ROWS));
  }
  RETERR(w.alloc(&heaps, (size_t)Qc * 2 * k));
  RETERR(w.alloc(&out, (size_t)Qc * k));
  RETERR(w.alloc(&outd, (size_t)Qc * k));
  const size_t max_blocks = (size_t)Qc / 32 + K + 1;   // (every plan packs >= 32 queries per block but one per cluster)
  RETERR(w.alloc(&blocks, 2 * max_blocks));
  if (host) {
    RETERR(w.alloc(&nb_dev, (size_t)Qc * k));
    if (distances) RETERR(w.alloc(&dist_dev, (size_t)Qc * k));
  }
  // radix sorts: the CSR of the chunk (keys <= K) and the query order (keys of up to 32 bits)
  const size_t sort_bytes = sort_temp_bytes(Qc, 0xFFFFFFFFu);
  char *sort_temp = nullptr;
  RETERR(w.alloc(&sort_temp, sort_bytes + 16));
  // the queries' clusters: the engine's assignment pass (kmamd_lloyd_assign; D > 256 through lloyd_wide), on fp32 rows
  std::unique_ptr<Engine> eng;
  if (!qassign_in) {
    eng.reset(new Engine());
    RETERR(eng->init(s.dev, Qc, D, K, metric, 0, st));
  }
  std::vector<uint32_t> offs(K + 1), plan;
  for (uint32_t q0 = 0; q0 < Q; q0 += Qc) {
    const uint32_t n = Q - q0 < Qc ? Q - q0 : Qc;
    // ---- the chunk's rows, fp32 on this device ----
    if (fp16) {
      const uint16_t *src = static_cast<const uint16_t *>(queries) + (size_t)q0 * D;
      KMX_HIPCP(hipMemcpyAsync(qhalf, src, (size_t)n * D * sizeof(uint16_t), host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
      KMX_HIPRT(launch_half_to_float(qhalf, (size_t)n * D, qrows, st));
    } else {
      const float *src = static_cast<const float *>(queries) + (size_t)q0 * D;
      KMX_HIPCP(hipMemcpyAsync(qrows, src, (size_t)n * D * sizeof(float), host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    }
    // ---- their clusters ----
    if (qassign_in) {
      KMX_HIPCP(hipMemcpyAsync(qassign, qassign_in + q0, (size_t)n * sizeof(uint32_t),
                               host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    } else {
      // (rows [n, Qc) of a last, shorter chunk hold the previous chunk's rows: assigned and ignored)
      KMX_HIPRT(hipMemsetAsync(qassign, 0, (size_t)Qc * sizeof(uint32_t), st));
      RETERR(eng->lloyd_assign(qrows, s.centroids, qassign, qprev, false));
    }
    if (qassign_out)
      KMX_HIPCP(hipMemcpyAsync(qassign_out + q0, qassign, (size_t)n * sizeof(uint32_t),
                               host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    // ---- the chunk in cluster-sorted order: rows, norms, distances to the own centroid ----
    KMX_HIPRT(hipMemsetAsync(qstats, 0, 4 * sizeof(uint32_t), st));
    KMX_HIPRT(launch_knn_query_clusters(qrows, n, D, qassign, K, s.centroids, qeff, qstats + 2, st));
    KMX_HIPRT(launch_inverse_assignments(qeff, n, K, keys_tmp, vals_tmp, keys_sorted, qinv, qoffsets, sort_temp, sort_bytes, st));
    // (with mu: the queries raise the half-range flag qstats[1] as the corpus rows do)
    KMX_HIPRT(launch_knn_gather(qrows, n, D, DP, qinv, qxs, qn2p, qstats, path.use_f16 ? s.mu : nullptr, qoffsets, K, st));
    KMX_HIPRT(launch_knn_member(metric, qxs, n, D, DP, qoffsets, K, s.centroids, qmydist, qrdist, path.strict_h2, st));
    uint32_t flags[4] = {0, 0, 0, 0};
    KMX_HIPCP(hipMemcpyAsync(offs.data(), qoffsets, (K + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    KMX_HIPCP(hipMemcpyAsync(flags, qstats, sizeof(flags), hipMemcpyDeviceToHost, st));
    KMX_HIPRT(hipStreamSynchronize(st));
    if (flags[2]) return kmcudaInvalidArguments;   // a caller-supplied cluster id >= K or with a non-finite centroid
    // which search this chunk takes: a query that leaves the half range sends it from the f16 filter to the f32 one
    // (D <= 256) or to the exact search, as a corpus row sends knn_cuda()
    bool f16 = path.use_f16;
    uint32_t dp_filter = path.dp_filter;
    if (f16 && flags[1]) {
      f16 = false;
      if (D > 256) dp_filter = 0;
      if (verbosity > 0) printf("k-NN query: a centred query leaves the half range, %s\n",
                                dp_filter ? "the f32 matrix-core filter" : "the exact search");
    }
    if (f16) KMX_HIPRT(launch_knn_split(metric, qxs, n, D, DP, s.mu, qxs16, qn2c, qmux, qkbias, qstats + 3, st));
    const uint32_t assigned = offs[K];   // positions >= assigned: queries without a cluster (NaN / inf features)
    const uint32_t qpb = f16 ? knn_qpb_f16(DP) : KNN_QPB_F32;
    plan.clear();
    for (uint32_t c = 0; c < K; c++)
      for (uint32_t p = offs[c]; p < offs[c + 1]; p += qpb) {
        plan.push_back(c);
        plan.push_back(p);
      }
    const uint32_t nblocks = (uint32_t)(plan.size() / 2);
    if (!plan.empty())
      KMX_HIPCP(hipMemcpyAsync(blocks, plan.data(), plan.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    // unassigned queries: indices 0xFFFFFFFF, distances NaN (the filters leave their slots alone)
    KMX_HIPRT(hipMemsetAsync(out, 0xFF, (size_t)n * k * sizeof(uint32_t), st));
    KMX_HIPRT(hipMemsetAsync(outd, 0xFF, (size_t)n * k * sizeof(float), st));
    KnnArgs a;
    a.xs = s.xs; a.n2s = f16 ? n2c : s.n2s; a.inv = s.inv; a.offsets = s.offsets; a.mydist = s.mydist; a.R = s.R;
    a.C = s.C; a.blocks = blocks; a.stats = f16 ? s.stats : stats_plain; a.N = N; a.D = D; a.DP = DP; a.K = K; a.k = k;
    a.p_base = 0; a.p_end = dp_filter ? assigned : n;   // (the exact kernel also fills the unassigned queries)
    a.eps = (float)(1.02 * ((double)D + 12.0) * ldexp(1.0, -24));  // as knn_cuda()
    a.heaps = heaps; a.out = out; a.calced = s.calced;
    a.xs16 = s.xs16; a.mux = s.mux; a.kbias = s.kbias; a.mu2 = mu2;
    a.qxs = qxs; a.qn2s = f16 ? qn2c : qn2p; a.qmux = qmux; a.qmydist = qmydist; a.qxs16 = qxs16; a.qoffsets = qoffsets;
    a.outd = outd;
    // the second cluster test and the query order of the f16 search (as knn_cuda(): kmcuda_api.cpp)
    if (f16 && tight_ok && assigned != 0) {
      if (!lb) RETERR(w.alloc(&lb, (size_t)K * Qc));
      KMX_HIPRT(launch_knn_centroid_bounds(qxs, D, DP, 0, assigned, s.centroids, K, s.R, lb, assigned, st));
      a.lb = lb;
      a.lb_stride = assigned;
      if (ord_mode != 0) {
        if (!qperm) RETERR(w.alloc(&qperm, Qc));
        if (launch_knn_query_order(lb, assigned, qoffsets, K, 0, assigned, keys_tmp, vals_tmp, keys_sorted, qperm,
                                   sort_temp, sort_bytes, st, ord_mode, qmydist, s.R))
          a.qperm = qperm;
        else
          (void)hipGetLastError();
      }
    }
    const hipError_t e = !dp_filter ? launch_knn_exact(metric, a, path.strict_h2, st, false)
                         : f16 ? launch_knn_filter_f16(metric, a, nblocks, st, false)
                               : launch_knn_filter(metric, a, nblocks, st, false);
    if (e != hipSuccess) return kmcudaRuntimeError;
    // ---- back in query order ----
    uint32_t *nb = host ? nb_dev : neighbors + (size_t)q0 * k;
    KMX_HIPRT(launch_knn_scatter(out, qinv, 0, n, k, nb, st));
    if (distances) {
      float *dd = host ? dist_dev : distances + (size_t)q0 * k;
      KMX_HIPRT(launch_knn_scatter(reinterpret_cast<const uint32_t *>(outd), qinv, 0, n, k, reinterpret_cast<uint32_t *>(dd), st));
    }
    if (host) {
      KMX_HIPCP(hipMemcpyAsync(neighbors + (size_t)q0 * k, nb_dev, (size_t)n * k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      if (distances)
        KMX_HIPCP(hipMemcpyAsync(distances + (size_t)q0 * k, dist_dev, (size_t)n * k * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    // (the next chunk overwrites these buffers: the stream orders it behind this one's scatter and copies)
  }
  if (hipStreamSynchronize(st) != hipSuccess) {
    if (verbosity > 0) printf("k-NN query failed: %s\n", hipGetErrorString(hipGetLastError()));
    return kmcudaRuntimeError;
  }
  return 0;
}

}  // namespace

struct kmamd_knn_index {
  KnnIndex ix;
};

extern "C" {

int kmamd_knn_index_create(kmamd_knn_index **out, int device, int metric, int fp16x2, uint32_t n_rows,
                           uint32_t features, uint32_t clusters, const void *samples, const void *centroids,
                           const uint32_t *assignments, int32_t device_ptrs, int verbosity) {
  if (!out) return kmcudaInvalidArguments;
  *out = nullptr;
  if (metric != 0 && metric != 1) return kmcudaInvalidArguments;
  if (n_rows == 0 || features == 0 || clusters == 0 || clusters == UINT32_MAX) return kmcudaInvalidArguments;
  if (fp16x2 && (features & 1u)) return kmcudaInvalidArguments;
  if (!samples || !centroids || !assignments) return kmcudaInvalidArguments;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return kmcudaNoSuchDevice;
  if (device_ptrs >= 0 && device_ptrs != device) return kmcudaInvalidArguments;   // one device per index
  g_verbosity = verbosity;
  if (device_ptrs >= 0 && hipSetDevice(device_ptrs) == hipSuccess) (void)hipDeviceSynchronize();  // as knn_cuda()
  kmamd_knn_index *h = new kmamd_knn_index();
  const int rc = h->ix.build(device, metric, fp16x2, n_rows, features, clusters, samples, centroids, assignments,
                             device_ptrs, verbosity);
  if (rc != 0) {
    delete h;
    return rc;
  }
  *out = h;
  return kmcudaSuccess;
}

int kmamd_knn_index_query(kmamd_knn_index *h, uint32_t k, uint32_t n_queries, const void *queries,
                          const uint32_t *query_assignments, uint32_t *neighbors, float *distances,
                          uint32_t *query_assignments_out, int32_t device_ptrs) {
  if (!h) return kmcudaInvalidArguments;
  KnnIndex &ix = h->ix;
  if (k == 0 || k > 65535u || k > ix.N) return kmcudaInvalidArguments;
  if (device_ptrs >= 0 && device_ptrs != ix.s.dev) return kmcudaInvalidArguments;
  if (n_queries == 0) return kmcudaSuccess;
  if (!queries || !neighbors) return kmcudaInvalidArguments;
  if (device_ptrs >= 0 && hipSetDevice(device_ptrs) == hipSuccess) (void)hipDeviceSynchronize();  // the caller's writes
  return ix.query(k, n_queries, queries, query_assignments, neighbors, distances, query_assignments_out, device_ptrs);
}

void kmamd_knn_index_destroy(kmamd_knn_index *h) { delete h; }

}  // extern "C"
