// knn_index.cpp -- k nearest neighbours of NEW rows (queries) among a clustered corpus: kmamd_knn_index_* of
// include/kmcuda_amd.h.
//
// knn_cuda() answers the self-join only (every corpus row against the others, the row itself skipped: knn.cu:204-206).
// Here the corpus is prepared ONCE per index -- the cluster-sorted fp32 copy, the f16 split, radii, the K x K centroid
// distances, mu and the stats, by the preparation knn_cuda() runs (knn_host.cpp: knn_prepare_corpus) -- and every
// query batch goes through the same search launch (knn_search) with the kernels in their query mode (SELF = false: the
// query side from its own buffers, KnnArgs::q*).  A query's list is what the reference's procedure gives for it as one
// more row of its cluster c_q, without the self-skip: own cluster in ascending corpus order, then the
// other clusters in ascending id under the triangle prune, push iff distance <= kth, output popped from the heap.  c_q
// is its nearest centroid (kmamd_lloyd_assign's arithmetic and tie rule) unless the caller passes one; any cluster id
// gives the same lists (the prune is rigorous), only the work differs.
#include <stdio.h>

#include <memory>

#include "../../include/kmcuda_amd.h"
#include "knn_host.hpp"

using namespace kmx;

namespace {

// lb (K floats per query) and the heaps (2k floats per query) of one chunk of queries stay within this budget
constexpr size_t kQueryChunkBytes = (size_t)4 << 30;

class KnnIndex {
 public:
  KnnShard s;   // the prepared corpus (its buffers and stream); plain and centred norms both kept
  KnnPath path;
  int verbosity = 0;
  bool fp16 = false;

  int build(int device, const KnnCorpus &c, int verbosity_) {
    fp16 = c.fp16; verbosity = verbosity_;
    path = knn_choose_path(c.D, fp16, verbosity, knn_switches());
    s.dev = device;
    KnnShard *one = &s;
    bool left_half_range = false;
    KNN_TRY(knn_prepare_corpus(&one, 1, c, true, &path, &left_half_range, nullptr));
    if (left_half_range && verbosity > 0)   // no f16 filter for this index
      printf("k-NN index: a centred row leaves the half range, %s\n",
             path.dp_filter ? "the f32 matrix-core filter instead of the f16 one" : "every candidate is evaluated exactly");
    if (s.centroids == c.centroids) {   // the caller's centroids may change after this call: the index keeps a copy
      float *cen = nullptr;
      KNN_TRY(s.alloc(&cen, (size_t)c.K * c.D));
      KMX_HIPCP(hipMemcpyAsync(cen, s.centroids, (size_t)c.K * c.D * sizeof(float), hipMemcpyDeviceToDevice, s.stream));
      s.centroids = cen;
    }
    KMX_HIPRT(hipStreamSynchronize(s.stream));
    // what the searches no longer read
    s.release(s.samples);
    s.release(s.assignments);
    s.release(s.rdist);
    s.release(s.scratch.keys_tmp);
    s.release(s.scratch.vals_tmp);
    s.release(s.scratch.keys_sorted);
    s.release(s.scratch.sort_temp);
    s.samples = nullptr; s.assignments = nullptr; s.rdist = nullptr; s.scratch.keys_tmp = s.scratch.vals_tmp = s.scratch.keys_sorted = nullptr;
    s.scratch.sort_temp = nullptr;
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
  const uint32_t D = s.D, DP = s.DP, K = s.K;
  const int metric = s.metric;
  const hipStream_t st = s.stream;
  const KnnSwitches sw = knn_switches();
  size_t chunk = kQueryChunkBytes / (4 * ((size_t)K + 2 * (size_t)k));
  if (sw.query_chunk) chunk = sw.query_chunk;   // test hook: queries per chunk
  if (chunk < 1) chunk = 1;
  const uint32_t Qc = (uint32_t)(chunk < Q ? chunk : Q);
  const bool host = device_ptrs < 0;

  // per-call buffers (freed with `w`), among them the sort scratch and the optional buffers of knn_search
  KnnShard w;
  w.dev = s.dev;
  w.stream = nullptr;   // (enqueues on the index's stream; nothing to release)
  float *qrows = nullptr, *qxs = nullptr, *qn2p = nullptr, *qn2c = nullptr, *qmydist = nullptr, *qrdist = nullptr,
        *qmux = nullptr, *qkbias = nullptr, *heaps = nullptr, *outd = nullptr, *dist_dev = nullptr;
  uint16_t *qhalf = nullptr, *qxs16 = nullptr;
  uint32_t *qassign = nullptr, *qprev = nullptr, *qeff = nullptr, *qinv = nullptr, *qoffsets = nullptr,
           *qstats = nullptr, *blocks = nullptr, *out = nullptr, *nb_dev = nullptr;
  KNN_TRY(w.alloc(&qrows, (size_t)Qc * D));
  if (fp16) KNN_TRY(w.alloc(&qhalf, (size_t)Qc * D));
  KNN_TRY(w.alloc(&qassign, Qc));
  KNN_TRY(w.alloc(&qprev, Qc));
  KNN_TRY(w.alloc(&qeff, Qc));
  KNN_TRY(w.alloc(&qinv, Qc));
  KNN_TRY(w.alloc(&qoffsets, (size_t)K + 2));
  KNN_TRY(w.alloc(&w.scratch.keys_tmp, Qc));
  KNN_TRY(w.alloc(&w.scratch.vals_tmp, Qc));
  KNN_TRY(w.alloc(&w.scratch.keys_sorted, Qc));
  KNN_TRY(w.alloc(&qstats, 4));
  KNN_TRY(w.alloc(&qxs, (size_t)Qc * DP));
  KNN_TRY(w.alloc(&qn2p, Qc));
  KNN_TRY(w.alloc(&qmydist, Qc));
  KNN_TRY(w.alloc(&qrdist, Qc));
  if (path.use_f16) {
    KNN_TRY(w.alloc(&qxs16, ((size_t)Qc + KNN16_PAD_ROWS) * DP));
    KNN_TRY(w.alloc(&qn2c, Qc));
    KNN_TRY(w.alloc(&qmux, Qc));
    KNN_TRY(w.alloc(&qkbias, (size_t)Qc + KNN16_PAD_ROWS));
  }
  KNN_TRY(w.alloc(&heaps, (size_t)Qc * 2 * k));
  KNN_TRY(w.alloc(&out, (size_t)Qc * k));
  KNN_TRY(w.alloc(&outd, (size_t)Qc * k));
  const size_t max_blocks = (size_t)Qc / 32 + K + 1;   // (every plan packs >= 32 queries per block but one per cluster)
  KNN_TRY(w.alloc(&blocks, 2 * max_blocks));
  if (host) {
    KNN_TRY(w.alloc(&nb_dev, (size_t)Qc * k));
    if (distances) KNN_TRY(w.alloc(&dist_dev, (size_t)Qc * k));
  }
  // radix sorts: the CSR of the chunk (keys <= K) and the query order (keys of up to 32 bits)
  w.scratch.rows = Qc;
  w.scratch.sort_bytes = sort_temp_bytes(Qc, 0xFFFFFFFFu);
  char *sort_temp = nullptr;
  KNN_TRY(w.alloc(&sort_temp, w.scratch.sort_bytes + 16));
  w.scratch.sort_temp = sort_temp;
  // the queries' clusters: the engine's assignment pass (kmamd_lloyd_assign; D > 256 through lloyd_wide), on fp32 rows
  std::unique_ptr<Engine> eng;
  if (!qassign_in) {
    eng.reset(new Engine());
    KNN_TRY(eng->init(s.dev, Qc, D, K, metric, 0, st));
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
      KNN_TRY(eng->lloyd_assign(qrows, s.centroids, qassign, qprev, false));
    }
    if (qassign_out)
      KMX_HIPCP(hipMemcpyAsync(qassign_out + q0, qassign, (size_t)n * sizeof(uint32_t),
                               host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    // ---- the chunk in cluster-sorted order: rows, norms, distances to the own centroid ----
    KMX_HIPRT(hipMemsetAsync(qstats, 0, 4 * sizeof(uint32_t), st));
    KMX_HIPRT(launch_knn_query_clusters(qrows, n, D, qassign, K, s.centroids, qeff, qstats + 2, st));
    KMX_HIPRT(launch_inverse_assignments(qeff, n, K, w.scratch.keys_tmp, w.scratch.vals_tmp, w.scratch.keys_sorted, qinv, qoffsets, w.scratch.sort_temp,
                                         w.scratch.sort_bytes, st));
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
    KnnPath cp = path;
    if (knn_leaves_half_range(&cp.use_f16, &cp.dp_filter, D, flags[1]) && verbosity > 0)
      printf("k-NN query: a centred query leaves the half range, %s\n",
             cp.dp_filter ? "the f32 matrix-core filter" : "the exact search");
    const bool f16 = cp.use_f16;
    if (f16) KMX_HIPRT(launch_knn_split(metric, qxs, n, D, DP, s.mu, qxs16, qn2c, qmux, qkbias, qstats + 3, st));
    const uint32_t assigned = offs[K];   // positions >= assigned: queries without a cluster (NaN / inf features)
    knn_block_plan(offs.data(), K, knn_qpb(f16, DP), &plan);
    if (!plan.empty())
      KMX_HIPCP(hipMemcpyAsync(blocks, plan.data(), plan.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    // unassigned queries: indices 0xFFFFFFFF, distances NaN (the filters leave their slots alone)
    KMX_HIPRT(hipMemsetAsync(out, 0xFF, (size_t)n * k * sizeof(uint32_t), st));
    KMX_HIPRT(hipMemsetAsync(outd, 0xFF, (size_t)n * k * sizeof(float), st));
    KnnArgs a;
    a.blocks = blocks; a.k = k; a.heaps = heaps; a.out = out; a.outd = outd;
    a.p_base = 0; a.p_end = cp.dp_filter ? assigned : n;   // (the exact kernel also fills the unassigned queries)
    a.qxs = qxs; a.qn2s = f16 ? qn2c : qn2p; a.qmux = qmux; a.qmydist = qmydist; a.qxs16 = qxs16; a.qoffsets = qoffsets;
    KNN_TRY(knn_search(s, w.scratch, a, cp, sw, (uint32_t)(plan.size() / 2), false, verbosity));
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
  KnnCorpus c;
  c.metric = metric; c.fp16 = fp16x2 != 0; c.N = n_rows; c.D = features; c.K = clusters;
  c.samples = samples; c.centroids = centroids; c.assignments = assignments; c.device_ptrs = device_ptrs;
  kmamd_knn_index *h = new kmamd_knn_index();
  const int rc = h->ix.build(device, c, verbosity);
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
  if (k == 0 || k > 65535u || k > ix.s.N) return kmcudaInvalidArguments;
  if (device_ptrs >= 0 && device_ptrs != ix.s.dev) return kmcudaInvalidArguments;
  if (n_queries == 0) return kmcudaSuccess;
  if (!queries || !neighbors) return kmcudaInvalidArguments;
  if (device_ptrs >= 0 && hipSetDevice(device_ptrs) == hipSuccess) (void)hipDeviceSynchronize();  // the caller's writes
  return ix.query(k, n_queries, queries, query_assignments, neighbors, distances, query_assignments_out, device_ptrs);
}

void kmamd_knn_index_destroy(kmamd_knn_index *h) { delete h; }

}  // extern "C"
