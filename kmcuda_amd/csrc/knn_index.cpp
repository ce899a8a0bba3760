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
//
// Every top-k entry point is one call, topk(), of one request (TopkRequest).  With probe lists it is the approximate
// mode: the same procedure with one more skip rule -- a cluster that is not in the query's probe list
// is never visited.  The lists are the caller's, or the ranking of kmamd_kmeans_assign_top run here on the index's own
// centroids (AssignTopRanker, assign_top_job.cpp).
//
// add() takes more rows into the index: the new rows are prepared chunk by chunk with the launches a
// fresh index's rows go through and merged into new cluster-sorted copies (knn_merge.hip); the index's own buffers stay
// as they are until the whole batch has been enqueued without error.
//
// remove() takes rows out of every later search: their assignments become K ("no cluster"), the order a
// fresh index would give the patched assignments is made by its own sort, and one gather (knn_remove.hip) moves every
// row's values into a new state, whose member distances and radii the fresh index's kernels make again.
#include <math.h>
#include <stdio.h>

#include <memory>

#include "../../include/kmcuda_amd.h"
#include "knn_host.hpp"
#include "knn_merge_host.hpp"

using namespace kmx;

namespace {

// lb (K floats per query) and the heaps (2k floats per query) of one chunk of queries stay within this budget
constexpr size_t kQueryChunkBytes = (size_t)4 << 30;
// KnnArgs::cap of a search without a cap (FLT_MAX: the heap's own filler, so min(kth, cap) = kth)
constexpr float kNoCap = 3.402823466e+38f;

// The centred half copy of a state or chunk of N rows ends in KNN16_PAD_ROWS rows / biases of zeros (the filter's tile
// DMA reads whole tiles), as launch_knn_split leaves them
int zero_f16_pad(const KnnSortedRows &r, uint32_t N, uint32_t DP, hipStream_t st) {
  KMX_HIPRT(hipMemsetAsync(r.xs16 + (size_t)N * DP, 0, (size_t)KNN16_PAD_ROWS * DP * sizeof(uint16_t), st));
  KMX_HIPRT(hipMemsetAsync(r.kbias + N, 0, (size_t)KNN16_PAD_ROWS * sizeof(float), st));
  return 0;
}

// (`path`: what the index runs from now on)
void say_left_half_range(const KnnPath &path) {
  printf("k-NN index: a centred row leaves the half range, %s\n",
         path.dp_filter ? "the f32 matrix-core filter instead of the f16 one" : "every candidate is evaluated exactly");
}

// What an add replaces: the per-row copies of the index (the f16 filter's only while it runs), its CSR offsets (on the
// device and on the host: K + 2 entries, [K] the rows that have a cluster, [K + 1] all of them), radii and statistics.
struct IndexState {
  KnnSortedRows rows{};
  uint32_t *offsets = nullptr, *stats = nullptr, *stats_c = nullptr;
  float *R = nullptr;
  uint32_t N = 0;
  std::vector<uint32_t> off_host;
};

struct AddChunk;
struct ArenaScratch;

// One top-k call on the index: what the kmamd_knn_index_query* entry points ask of KnnIndex::topk
struct TopkRequest {
  uint32_t k = 0, Q = 0;
  float cap = kNoCap;   // the capped search, DESIGN.md 4.19 -- min(kth, cap) wherever the procedure reads kth
  const void *queries = nullptr;
  const uint32_t *qassign_in = nullptr;   // (neither of the two with probe lists: column 0 stands in)
  uint32_t *qassign_out = nullptr;
  uint32_t *neighbors = nullptr;
  float *distances = nullptr;
  const uint8_t *allow = nullptr;   // the masked search, DESIGN.md 4.17: one flag per row id on the side device_ptrs names
  int32_t device_ptrs = -1;
  const char *report = nullptr;   // what the KMCUDA_AMD_KNN_STATS line calls this call (null: it prints none)
  // the probed search, DESIGN.md 4.12 (pw = 0: none)
  uint32_t pw = 0;
  const uint32_t *probes_in = nullptr;   // the caller's lists, or null: ranked here
  uint32_t *probes_out = nullptr;        // optional
};

// One radius call: counts (fill = false), or the hits at the caller's CSR offsets
struct RadiusRequest {
  bool fill = false;
  float r = 0.f;
  uint32_t Q = 0;
  const void *queries = nullptr;
  const uint32_t *qassign_in = nullptr;
  uint32_t *qassign_out = nullptr;
  uint32_t *counts = nullptr;          // (count)
  const uint64_t *offsets = nullptr;   // (fill, as neighbors and the optional distances)
  uint32_t *neighbors = nullptr;
  float *distances = nullptr;
  const uint8_t *allow = nullptr;   // the masked radius search, DESIGN.md 4.18
  int32_t device_ptrs = -1;
};

// What a masked call prepares once, for all its query chunks: the caller's flags as one bit per sorted
// position, the allowed rows per cluster and the radii over them -- the radii of the index the call is defined by
struct QueryMask {
  uint32_t *bits = nullptr, *count = nullptr;
  float *R = nullptr;
  void fill_args(KnnArgs *a) const { a->allow_bits = bits; a->allow_count = count; a->R = R; }
};

class KnnIndex {
 public:
  KnnShard s;   // the prepared corpus (its buffers and stream); plain and centred norms both kept
  std::vector<uint32_t> off_host;   // IndexState::off_host of `s`
  KnnPath path;
  int verbosity = 0;
  bool fp16 = false;
  bool said_exact = false;   // the path's "no matrix-core filter" line has been printed (probe mode says it otherwise)

  int build(int device, const KnnCorpus &c, int verbosity_) {
    fp16 = c.fp16; verbosity = verbosity_;
    path = knn_choose_path(c.D, fp16, verbosity, knn_switches());
    said_exact = !path.dp_filter;
    s.dev = device;
    KnnShard *one = &s;
    bool left_half_range = false;
    off_host.assign((size_t)c.K + 2, c.N);
    KNN_TRY(knn_prepare_corpus(&one, 1, c, true, &path, &left_half_range, off_host.data()));
    if (left_half_range && verbosity > 0) say_left_half_range(path);   // no f16 filter for this index
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

  // probe mode: the centroid preparation of the ranking (kmamd_kmeans_assign_top's), made on the first probed query
  // that brings no lists of its own and kept until the index goes (its buffers belong to `s`)
  AssignTopRanker ranker;
  bool ranker_ready = false;

  int topk(const TopkRequest &rq);
  int prepare_mask(const uint8_t *allow, bool host, ArenaScratch &x, QueryMask *m);
  int radius(const RadiusRequest &rq);

  // ---- add ----
  int add(uint32_t n_rows, const void *rows, const uint32_t *assign_in, uint32_t *assign_out, int32_t device_ptrs);
  int add_chunks(uint32_t n_rows, const void *rows, const uint32_t *assign_in, uint32_t *assign_out, bool host);
  IndexState state() const {
    IndexState t;
    t.rows.xs = s.xs; t.rows.n2s = s.n2s; t.rows.mydist = s.mydist; t.rows.inv = s.inv;
    t.rows.xs16 = s.xs16; t.rows.n2c = s.n2c; t.rows.mux = s.mux; t.rows.kbias = s.kbias;
    t.offsets = s.offsets; t.stats = s.stats; t.stats_c = s.stats_c; t.R = s.R; t.N = s.N;
    t.off_host = off_host;
    return t;
  }
  void adopt(IndexState &t) {
    s.xs = t.rows.xs; s.n2s = t.rows.n2s; s.mydist = t.rows.mydist; s.inv = t.rows.inv;
    s.xs16 = t.rows.xs16; s.n2c = t.rows.n2c; s.mux = t.rows.mux; s.kbias = t.rows.kbias;
    s.offsets = t.offsets; s.stats = t.stats; s.stats_c = t.stats_c; s.R = t.R; s.N = t.N;
    off_host.swap(t.off_host);
  }
  // buffers for N rows (f16: the filter's too), owned by the shard's arena; whatever was allocated is released again
  // if one allocation fails
  int alloc_state(IndexState *t, uint32_t N, bool f16) {
    const uint32_t DP = s.DP, K = s.K;
    KnnSortedRows &r = t->rows;
    int rc = 0;
    auto get = [&](auto **p, size_t count) { if (!rc) rc = s.alloc(p, count); };
    get(&r.xs, (size_t)N * DP);
    get(&r.n2s, N);
    get(&r.mydist, N);
    get(&r.inv, N);
    get(&t->offsets, (size_t)K + 2);
    get(&t->stats, 4);
    get(&t->R, K);
    if (f16) {
      get(&r.xs16, ((size_t)N + KNN16_PAD_ROWS) * DP);
      get(&r.kbias, (size_t)N + KNN16_PAD_ROWS);
      get(&r.n2c, N);
      get(&r.mux, N);
      get(&t->stats_c, 4);
    }
    t->N = N;
    if (rc) {
      (void)hipGetLastError();
      release_state(*t);
    }
    return rc;
  }
  void release_f16(IndexState &t) {
    s.release(t.rows.xs16); s.release(t.rows.kbias); s.release(t.rows.n2c); s.release(t.rows.mux); s.release(t.stats_c);
    t.rows.xs16 = nullptr; t.rows.kbias = t.rows.n2c = t.rows.mux = nullptr; t.stats_c = nullptr;
  }
  void release_state(IndexState &t) {
    release_f16(t);
    s.release(t.rows.xs); s.release(t.rows.n2s); s.release(t.rows.mydist); s.release(t.rows.inv);
    s.release(t.offsets); s.release(t.stats); s.release(t.R);
    t = IndexState();
  }
  int merge(const IndexState &cur, const AddChunk &c, uint32_t n, IndexState *next);

  // ---- remove ----
  int remove(uint32_t n_ids, const uint32_t *ids, uint32_t *n_removed, int32_t device_ptrs);
  int radii(float *out, const uint8_t *allow = nullptr, int32_t device_ptrs = -1);
};

// n caller rows made cluster-sorted against this index: the buffers of one chunk of a query batch or of an add (sized
// for at most `cap` rows, reused by every chunk) and the steps both take on them.  Between upload() and sort() lies
// what differs: the rows' clusters (QueryChunk, AddChunk).
// stats: [0] the largest plain norm, [1] the half-range flag (both the gather's), [2] the largest centred norm (the
// split's; launch_knn_merge_radii reads it), [3] a flag of the cluster step
struct SortedChunk {
  DeviceArena w;   // owns the buffers; enqueues on the index's stream (nothing to release)
  KnnScratch scratch;   // the sort scratch (w's) and the optional buffers of knn_search
  uint32_t cap = 0;
  float *rows = nullptr, *rdist = nullptr;
  uint16_t *half = nullptr;
  uint32_t *asg = nullptr, *prev = nullptr, *offsets = nullptr, *stats = nullptr;
  KnnSortedRows b{};   // the chunk in cluster-sorted order (inv: sorted position -> row of the chunk)
  std::vector<uint32_t> offs;   // `offsets` on the host (K + 1)

  // sort_max_key: the largest key sort() or a search's query order will see; want_prev: an engine's assignment pass runs
  int init(const KnnIndex &ix, uint32_t cap_, uint32_t sort_max_key, bool want_prev) {
    const KnnShard &s = ix.s;
    const uint32_t D = s.D, DP = s.DP, K = s.K;
    cap = cap_;
    w.dev = s.dev;
    w.stream = nullptr;
    KNN_TRY(w.alloc(&rows, (size_t)cap * D));
    if (ix.fp16) KNN_TRY(w.alloc(&half, (size_t)cap * D));
    KNN_TRY(w.alloc(&asg, cap));
    if (want_prev) KNN_TRY(w.alloc(&prev, cap));
    KNN_TRY(w.alloc(&b.inv, cap));
    KNN_TRY(w.alloc(&offsets, (size_t)K + 2));
    KNN_TRY(w.alloc(&scratch.keys_tmp, cap));
    KNN_TRY(w.alloc(&scratch.vals_tmp, cap));
    KNN_TRY(w.alloc(&scratch.keys_sorted, cap));
    KNN_TRY(w.alloc(&stats, 4));
    KNN_TRY(w.alloc(&b.xs, (size_t)cap * DP));
    KNN_TRY(w.alloc(&b.n2s, cap));
    KNN_TRY(w.alloc(&b.mydist, cap));
    KNN_TRY(w.alloc(&rdist, cap));
    if (ix.path.use_f16) {
      KNN_TRY(w.alloc(&b.xs16, ((size_t)cap + KNN16_PAD_ROWS) * DP));
      KNN_TRY(w.alloc(&b.n2c, cap));
      KNN_TRY(w.alloc(&b.mux, cap));
      KNN_TRY(w.alloc(&b.kbias, (size_t)cap + KNN16_PAD_ROWS));
    }
    scratch.rows = cap;
    scratch.sort_bytes = sort_temp_bytes(cap, sort_max_key);
    char *sort_temp = nullptr;
    KNN_TRY(w.alloc(&sort_temp, scratch.sort_bytes + 16));
    scratch.sort_temp = sort_temp;
    offs.resize((size_t)K + 1);
    return 0;
  }

  // rows [r0, r0 + n) of the caller's row matrix, fp32 in `rows` (halves by way of `half`)
  int upload(const KnnIndex &ix, const void *src, size_t r0, size_t n, bool host) {
    const hipStream_t st = ix.s.stream;
    const uint32_t D = ix.s.D;
    const hipMemcpyKind kind = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    if (ix.fp16) {
      KMX_HIPCP(hipMemcpyAsync(half, static_cast<const uint16_t *>(src) + r0 * D, n * D * sizeof(uint16_t), kind, st));
      KMX_HIPRT(launch_half_to_float(half, n * D, rows, st));
    } else {
      KMX_HIPCP(hipMemcpyAsync(rows, static_cast<const float *>(src) + r0 * D, n * D * sizeof(float), kind, st));
    }
    return 0;
  }
  // the CSR of the chunk (b.inv, offsets) by a key per row (>= K: no cluster)
  int sort(const KnnIndex &ix, const uint32_t *keys, uint32_t n) {
    KMX_HIPRT(launch_inverse_assignments(keys, n, ix.s.K, scratch.keys_tmp, scratch.vals_tmp, scratch.keys_sorted, b.inv, offsets,
                                         scratch.sort_temp, scratch.sort_bytes, ix.s.stream));
    return 0;
  }
  // the rows in that order: the DP-padded copy, plain norms, their maximum and -- with mu, the f16 filter's centre --
  // the half-range flag, which the chunk's rows raise as the corpus rows do; distances to the own centroid
  int gather(const KnnIndex &ix, uint32_t n) {
    const KnnShard &s = ix.s;
    KMX_HIPRT(launch_knn_gather(rows, n, s.D, s.DP, b.inv, b.xs, b.n2s, stats, ix.path.use_f16 ? s.mu : nullptr, offsets, s.K, s.stream));
    KMX_HIPRT(launch_knn_member(s.metric, b.xs, n, s.D, s.DP, offsets, s.K, s.centroids, b.mydist, rdist, ix.path.strict_h2, s.stream));
    return 0;
  }
  // the f16 filter's side of the sorted rows
  int split(const KnnIndex &ix, uint32_t n) {
    const KnnShard &s = ix.s;
    KMX_HIPRT(launch_knn_split(s.metric, b.xs, n, s.D, s.DP, s.mu, b.xs16, b.n2c, b.mux, b.kbias, stats + 2, s.stream));
    return 0;
  }
  // the offsets and, where asked for, the four stat words on the host: the chunk's one wait for the stream
  int fetch(const KnnIndex &ix, uint32_t *stats_host) {
    const hipStream_t st = ix.s.stream;
    KMX_HIPCP(hipMemcpyAsync(offs.data(), offsets, ((size_t)ix.s.K + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (stats_host) KMX_HIPCP(hipMemcpyAsync(stats_host, stats, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    KMX_HIPRT(hipStreamSynchronize(st));
    return 0;
  }
};

// The probe side of a chunk: raw = the chunk's n x pw lists in query order (the caller's slice, or the
// ranking's), lists = what the PROBE kernels read, per sorted query position (launch_knn_probe_lists)
struct ProbeSide {
  uint32_t pw = 0;
  const uint32_t *probes_in = nullptr;   // the caller's lists (whole batch), or null: ranked here
  uint32_t *probes_out = nullptr;        // optional (whole batch)
  AssignTopRanker ranker;                // (computed lists, K >= 2)
  bool rank_exact = false;
  uint32_t *raw = nullptr, *lists = nullptr;

  // for chunks of at most Qc queries (buffers: w's); the ranking's centroid preparation is made on the index's first
  // probed call that brings no lists of its own
  int init(KnnIndex &ix, DeviceArena &w, uint32_t Qc, const TopkRequest &rq) {
    pw = rq.pw; probes_in = rq.probes_in; probes_out = rq.probes_out;
    KNN_TRY(w.alloc(&raw, (size_t)Qc * pw));
    KNN_TRY(w.alloc(&lists, (size_t)Qc * pw));
    if (probes_in || ix.s.K < 2) return 0;
    if (!ix.ranker_ready) {
      KNN_TRY(ix.ranker.prepare(ix.s, ix.s.metric, ix.s.centroids, ix.s.K, ix.s.D, false));
      ix.ranker_ready = true;
    }
    ranker = ix.ranker;
    rank_exact = assign_top_exact_only();
    return ranker.reserve(w, Qc);
  }
};

// What a chunk of queries is prepared for.  There is a matrix-core filter on f32 for the plain top-k search alone: a
// search with probe lists or a mask, and the radius search, take the f16 filter or the exact kernel.
enum class ChunkUse { topk, topk_subset, radius };   // (subset: probe lists and / or a mask)

// A chunk of queries, shared by the top-k and the radius calls: the queries' clusters, the sorted chunk and the block
// plan of its search.
struct QueryChunk : SortedChunk {
  uint32_t *qeff = nullptr, *blocks = nullptr;
  std::unique_ptr<Engine> eng;   // (a member of the derived type: it goes before the arena whose stream it uses)
  std::vector<uint32_t> plan;
  // what prepare() found out about the chunk
  KnnPath cp;
  uint32_t assigned = 0;   // sorted positions >= assigned: queries without a cluster (NaN / inf features)

  int init(const KnnIndex &ix, uint32_t Qc, bool assign) {
    const KnnShard &s = ix.s;
    // radix sorts: the CSR of the chunk (keys <= K) and the query order (keys of up to 32 bits)
    KNN_TRY(SortedChunk::init(ix, Qc, 0xFFFFFFFFu, true));
    KNN_TRY(w.alloc(&qeff, Qc));
    const size_t max_blocks = (size_t)Qc / 32 + s.K + 1;   // (every plan packs >= 32 queries per block but one per cluster)
    KNN_TRY(w.alloc(&blocks, 2 * max_blocks));
    // the queries' clusters: the engine's assignment pass (kmamd_lloyd_assign; D > 256 through lloyd_wide), on fp32 rows
    if (assign) {
      eng.reset(new Engine());
      KNN_TRY(eng->init(s.dev, Qc, s.D, s.K, s.metric, 0, s.stream));
    }
    return 0;
  }

  // queries [q0, q0 + n) of the batch; waits for the stream once (the CSR offsets and the flags reach the host)
  // pr: probe mode -- the chunk's lists are fetched or ranked, their column 0 stands in for qassign_in
  // Leaves in `cp` the search the chunk takes for `use` (the one place that decides it), split and planned for it.
  int prepare(const KnnIndex &ix, ChunkUse use, uint32_t q0, uint32_t n, const void *queries, const uint32_t *qassign_in,
              uint32_t *qassign_out, bool host, ProbeSide *pr = nullptr) {
    const KnnShard &s = ix.s;
    const uint32_t D = s.D, K = s.K;
    const hipStream_t st = s.stream;
    KNN_TRY(upload(ix, queries, q0, n, host));
    // ---- their clusters ----
    if (pr) {
      const size_t cnt = (size_t)n * pr->pw;
      if (pr->probes_in)
        KMX_HIPCP(hipMemcpyAsync(pr->raw, pr->probes_in + (size_t)q0 * pr->pw, cnt * sizeof(uint32_t),
                                 host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
      else if (K == 1)   // (the ranking kernels need two centroids: P = {0})
        KMX_HIPRT(hipMemsetAsync(pr->raw, 0, cnt * sizeof(uint32_t), st));
      else
        KNN_TRY(pr->ranker.rank(rows, n, pr->pw, pr->raw, pr->rank_exact, st));
      if (pr->probes_out)
        KMX_HIPCP(hipMemcpyAsync(pr->probes_out + (size_t)q0 * pr->pw, pr->raw, cnt * sizeof(uint32_t),
                                 host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
      KMX_HIPRT(launch_knn_probe_column0(pr->raw, pr->pw, n, asg, st));
    } else if (qassign_in) {
      KMX_HIPCP(hipMemcpyAsync(asg, qassign_in + q0, (size_t)n * sizeof(uint32_t),
                               host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    } else {
      // (rows [n, cap) of a shorter chunk hold an earlier chunk's rows, or radius()'s zeros: assigned and ignored)
      KMX_HIPRT(hipMemsetAsync(asg, 0, (size_t)cap * sizeof(uint32_t), st));
      KNN_TRY(eng->lloyd_assign(rows, s.centroids, asg, prev, false));
    }
    if (qassign_out)
      KMX_HIPCP(hipMemcpyAsync(qassign_out + q0, asg, (size_t)n * sizeof(uint32_t),
                               host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    // ---- the chunk in cluster-sorted order: rows, norms, distances to the own centroid ----
    KMX_HIPRT(hipMemsetAsync(stats, 0, 4 * sizeof(uint32_t), st));
    KMX_HIPRT(launch_knn_query_clusters(rows, n, D, asg, K, s.centroids, qeff, stats + 3, st));
    KNN_TRY(sort(ix, qeff, n));
    if (pr) KMX_HIPRT(launch_knn_probe_lists(pr->raw, pr->pw, n, b.inv, K, pr->lists, stats + 3, st));
    KNN_TRY(gather(ix, n));
    uint32_t flags[4] = {0, 0, 0, 0};
    KNN_TRY(fetch(ix, flags));
    // a caller-supplied cluster id >= K or with a non-finite centroid, or an entry > K in a caller's probe list (a row
    // the ranking fills with K has no cluster: no error)
    if (flags[3] && !(pr && !pr->probes_in)) return kmcudaInvalidArguments;
    // which search this chunk takes: a query that leaves the half range sends it from the f16 filter to the f32 one
    // (D <= 256) or to the exact search, as a corpus row sends knn_cuda()
    cp = ix.path;
    if (knn_leaves_half_range(&cp.use_f16, &cp.dp_filter, D, flags[1]) && ix.verbosity > 0)
      printf("k-NN query: a centred query leaves the half range, %s\n",
             cp.dp_filter && !pr ? "the f32 matrix-core filter" : "the exact search");
    // no f32 filter but the plain top-k search's: whatever is not the f16 filter there takes the exact kernel
    if (use != ChunkUse::topk && !cp.use_f16) cp.dp_filter = 0;
    // nor an f16 probe search at a K its visit map has no room for
    if (pr && K > KNN_PROBE_BITMAP_K) { cp.use_f16 = false; cp.dp_filter = 0; }
    if (cp.use_f16) KNN_TRY(split(ix, n));
    assigned = offs[K];
    knn_block_plan(offs.data(), K, knn_qpb(cp.use_f16, s.DP), &plan);
    if (!plan.empty())
      KMX_HIPCP(hipMemcpyAsync(blocks, plan.data(), plan.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    return 0;
  }

  // the query side of a search launch over this chunk of n queries
  void fill_args(KnnArgs *a, uint32_t n) const {
    a->blocks = blocks;
    a->p_base = 0;
    a->p_end = cp.dp_filter ? assigned : n;   // (the exact kernel also fills the unassigned queries)
    a->qxs = b.xs; a->qn2s = cp.use_f16 ? b.n2c : b.n2s; a->qmux = b.mux; a->qmydist = b.mydist; a->qxs16 = b.xs16; a->qoffsets = offsets;
  }
};

// HIP events on the index's stream at the stage boundaries of a call, where a switch asks for them
template <int N>
struct StageEvents {
  hipEvent_t ev[N] = {};
  bool on = false;
  ~StageEvents() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  void start(bool on_) {
    on = on_;
    for (hipEvent_t &e : ev)
      if (on && hipEventCreate(&e) != hipSuccess) on = false;
  }
  void mark(int i, hipStream_t st) const {
    if (on) (void)hipEventRecord(ev[i], st);
  }
  float elapsed(int from, int to) const {   // (after a wait for the stream)
    float t = 0.f;
    return on && hipEventElapsedTime(&t, ev[from], ev[to]) == hipSuccess ? t : 0.f;
  }
};

// KMCUDA_AMD_KNN_ADD_TIME: the three stages of every chunk of an add -- the rows' clusters (upload and assignment pass),
// the chunk's preparation (CSR, gather, member distances, split), the merge --, summed over the chunks and printed at
// the end of the call (scripts/knn_add_bench.py reads the line)
struct AddTimer : StageEvents<5> {   // (2 -> 3: the host's wait and allocations)
  float ms[3] = {0.f, 0.f, 0.f};
  unsigned long long merged_bytes = 0;
  void fold() {   // (after a wait for the stream)
    for (int i = 0; i < 3; i++) ms[i] += elapsed(i == 2 ? 3 : i, i == 2 ? 4 : i + 1);
  }
};

// A chunk of an add: what knn_prepare_corpus makes of a corpus's rows, by the same launches, with the index's
// centroids, mu and path.
struct AddChunk : SortedChunk {
  EngineSlot slot;   // (a member of the derived type: the engine goes before the arena whose stream it uses)

  int init(const KnnIndex &ix, uint32_t Cn, bool assign) { return SortedChunk::init(ix, Cn, ix.s.K, assign); }

  // rows [r0, r0 + n) of the batch; waits for the stream once (the chunk's offsets reach the host)
  int prepare(const KnnIndex &ix, uint32_t r0, uint32_t n, const void *src, const uint32_t *assign_in,
              uint32_t *assign_out, bool host, const AddTimer &tm) {
    const KnnShard &s = ix.s;
    const uint32_t D = s.D, K = s.K;
    const hipStream_t st = s.stream;
    tm.mark(0, st);
    KNN_TRY(upload(ix, src, r0, n, host));
    // ---- their clusters: the caller's (>= K: none, as create takes them), or kmamd_kmeans_assign's ----
    if (assign_in) {
      KMX_HIPCP(hipMemcpyAsync(asg, assign_in + r0, (size_t)n * sizeof(uint32_t),
                               host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    } else if (K == 1) {   // (the engine needs two centroids: a row of finite features has cluster 0)
      KMX_HIPRT(hipMemsetAsync(prev, 0, (size_t)n * sizeof(uint32_t), st));
      KMX_HIPRT(launch_knn_query_clusters(rows, n, D, prev, K, s.centroids, asg, stats + 3, st));
    } else {
      // assignments <- K ("no cluster"), then one pass of an engine sized for the chunk (assign_job.cpp)
      Engine *eng = nullptr;
      KNN_TRY(slot.get(s.dev, n, D, K, s.metric, st, half, &eng));
      KMX_HIPRT(hipMemsetD32Async((hipDeviceptr_t)asg, (int)K, n, st));
      KNN_TRY(eng->lloyd_assign(rows, s.centroids, asg, prev, false));
    }
    if (assign_out)
      KMX_HIPCP(hipMemcpyAsync(assign_out + r0, asg, (size_t)n * sizeof(uint32_t),
                               host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    tm.mark(1, st);
    // ---- the chunk in cluster-sorted order, with everything an index keeps per row ----
    KNN_TRY(sort(ix, asg, n));
    KNN_TRY(gather(ix, n));
    if (ix.path.use_f16) KNN_TRY(split(ix, n));
    tm.mark(2, st);
    return fetch(ix, nullptr);
  }
};

// KMCUDA_AMD_KNN_STATS: what the searches of a radius or probe call did (KnnArgs::calced), then the counters start over
int report_stats(const KnnIndex &ix, const char *what) {
  unsigned long long cs[KNN_STATS] = {0, 0, 0, 0, 0};
  KMX_HIPCP(hipMemcpy(cs, ix.s.calced, sizeof(cs), hipMemcpyDeviceToHost));
  printf("k-NN index %s: %llu pairs in visited clusters, %llu scored on the matrix cores (%llu of them live query x "
         "real candidate; %llu by operand sets with a visiting query), %llu exact chains\n", what, cs[0], cs[1], cs[2],
         cs[4], cs[3]);
  fflush(stdout);
  KMX_HIPRT(hipMemset(ix.s.calced, 0, sizeof(cs)));
  return 0;
}

// The top-k lists of a query batch on their way to the caller: the search's buffers for one chunk of at most Qc queries
// (heaps, and out / outd in sorted-position order) and, for a caller on the host, the chunk in query order
struct TopkResult {
  uint32_t k = 0;
  bool host = false;
  float *heaps = nullptr, *outd = nullptr, *dist_dev = nullptr;
  uint32_t *out = nullptr, *nb_dev = nullptr;

  int init(DeviceArena &w, uint32_t Qc, uint32_t k_, bool host_, bool want_distances) {
    k = k_; host = host_;
    KNN_TRY(w.alloc(&heaps, (size_t)Qc * 2 * k));
    KNN_TRY(w.alloc(&out, (size_t)Qc * k));
    KNN_TRY(w.alloc(&outd, (size_t)Qc * k));
    if (host) {
      KNN_TRY(w.alloc(&nb_dev, (size_t)Qc * k));
      if (want_distances) KNN_TRY(w.alloc(&dist_dev, (size_t)Qc * k));
    }
    return 0;
  }
  // unassigned queries: indices 0xFFFFFFFF, distances NaN (the filters leave their slots alone)
  int clear(uint32_t n, hipStream_t st) {
    KMX_HIPRT(hipMemsetAsync(out, 0xFF, (size_t)n * k * sizeof(uint32_t), st));
    KMX_HIPRT(hipMemsetAsync(outd, 0xFF, (size_t)n * k * sizeof(float), st));
    return 0;
  }
  void fill_args(KnnArgs *a) const { a->k = k; a->heaps = heaps; a->out = out; a->outd = outd; }
  // the chunk of n queries from q0 on, back in query order (qinv: sorted position -> query) and to the caller.  (The
  // next chunk overwrites these buffers: the stream orders it behind this one's scatter and copies.)
  int deliver(uint32_t q0, uint32_t n, const uint32_t *qinv, uint32_t *neighbors, float *distances, hipStream_t st) {
    const size_t at = (size_t)q0 * k, count = (size_t)n * k;
    KMX_HIPRT(launch_knn_scatter(out, qinv, 0, n, k, host ? nb_dev : neighbors + at, st));
    if (distances)
      KMX_HIPRT(launch_knn_scatter(reinterpret_cast<const uint32_t *>(outd), qinv, 0, n, k,
                                   reinterpret_cast<uint32_t *>(host ? dist_dev : distances + at), st));
    if (host) {
      KMX_HIPCP(hipMemcpyAsync(neighbors + at, nb_dev, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      if (distances) KMX_HIPCP(hipMemcpyAsync(distances + at, dist_dev, count * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    return 0;
  }
};

// The scratch of one call, taken from the index's arena and given back when the call ends, whichever way it ends
// (behind a wait for the stream: kernels may still read it)
struct ArenaScratch {
  DeviceArena &a;
  std::vector<void *> mine;
  explicit ArenaScratch(DeviceArena &a_) : a(a_) {}
  ~ArenaScratch() {
    (void)hipStreamSynchronize(a.stream);
    for (void *p : mine) a.release(p);
  }
  template <typename T>
  int get(T **p, size_t count) {
    const int rc = a.alloc(p, count);
    if (rc == 0) mine.push_back(*p);
    else (void)hipGetLastError();
    return rc;
  }
};

// the last wait of a query call (`what`: its name)
int finish_query(const KnnIndex &ix, const char *what) {
  if (hipStreamSynchronize(ix.s.stream) == hipSuccess) return 0;
  if (ix.verbosity > 0) printf("k-NN %s failed: %s\n", what, hipGetErrorString(hipGetLastError()));
  return kmcudaRuntimeError;
}

// The mask of one call, enqueued on the index's stream; the scratch -- the staged bytes of a host
// mask, N / 8 bytes of bits, the member distances -- is x's and goes with the call.  The radii are those of the index
// the call is defined by, KnnIndex(rows, centroids, assignments with the denied rows' set to K): the chunked distances
// by the member kernel a fresh index runs (the index keeps none: 4 bytes per row it would carry through every add and
// remove, against one more pass over the rows per masked call), reduced over the allowed rows.
int KnnIndex::prepare_mask(const uint8_t *allow, bool host, ArenaScratch &x, QueryMask *m) {
  const uint32_t N = s.N, K = s.K;
  const hipStream_t st = s.stream;
  if (host) {
    uint8_t *up = nullptr;
    KNN_TRY(x.get(&up, N));
    KMX_HIPCP(hipMemcpyAsync(up, allow, N, hipMemcpyHostToDevice, st));
    allow = up;
  }
  unsigned long long *bits = nullptr;
  float *mydist = nullptr, *rdist = nullptr;
  KNN_TRY(x.get(&bits, knn_mask_words64(N)));
  KNN_TRY(x.get(&mydist, N));
  KNN_TRY(x.get(&rdist, N));
  KNN_TRY(x.get(&m->R, K));
  KNN_TRY(x.get(&m->count, K));
  m->bits = reinterpret_cast<uint32_t *>(bits);
  KMX_HIPRT(launch_knn_mask_pack(allow, s.inv, N, s.offsets + K, bits, st));
  KMX_HIPRT(launch_knn_member(s.metric, s.xs, N, s.D, s.DP, s.offsets, K, s.centroids, mydist, rdist, path.strict_h2, st));
  KMX_HIPRT(launch_knn_masked_radii(rdist, s.offsets, K, m->bits, m->R, m->count, st));
  return 0;
}

// One query batch, in chunks of at most Qc queries; every buffer is sized for one chunk and reused.  With probe lists
//  the cluster loop of the search is driven by every query's list.
int KnnIndex::topk(const TopkRequest &rq) {
  if (rq.Q == 0) return 0;
  if (hipSetDevice(s.dev) != hipSuccess) return kmcudaNoSuchDevice;
  const hipStream_t st = s.stream;
  const KnnSwitches sw = knn_switches();
  const bool host = rq.device_ptrs < 0, probed = rq.pw != 0;
  const ChunkUse use = probed || rq.allow ? ChunkUse::topk_subset : ChunkUse::topk;
  const char *const what = probed ? "probe query" : "query";
  // what a chunk keeps per query besides its heaps (2k floats): the probe lists, else the lb table (K floats)
  const size_t query_bytes = 4 * ((probed ? (size_t)rq.pw : (size_t)s.K) + 2 * (size_t)rq.k);
  const uint32_t Qc = knn_chunk_rows(kQueryChunkBytes, query_bytes, sw.query_chunk, rq.Q);

  ArenaScratch x(s);   // (before `c`: it waits for the stream, then releases)
  QueryMask mask;
  if (rq.allow) KNN_TRY(prepare_mask(rq.allow, host, x, &mask));
  // per-call buffers (freed with `c`), among them the sort scratch and the optional buffers of knn_search
  QueryChunk c;
  KNN_TRY(c.init(*this, Qc, !probed && !rq.qassign_in));
  ProbeSide pr;
  if (probed) KNN_TRY(pr.init(*this, c.w, Qc, rq));
  const KnnProbeOrder probe_order{pr.raw, c.b.inv};
  TopkResult res;
  KNN_TRY(res.init(c.w, Qc, rq.k, host, rq.distances != nullptr));
  // the counters line, where the call has a name for it (the plain query prints what it always printed)
  const bool stats = rq.report && sw.stats;
  if (stats) KMX_HIPRT(hipMemsetAsync(s.calced, 0, KNN_STATS * sizeof(unsigned long long), st));
  bool said = said_exact || verbosity <= 0;
  for (uint32_t q0 = 0; q0 < rq.Q; q0 += Qc) {
    const uint32_t n = rq.Q - q0 < Qc ? rq.Q - q0 : Qc;
    KNN_TRY(c.prepare(*this, use, q0, n, rq.queries, rq.qassign_in, rq.qassign_out, host, probed ? &pr : nullptr));
    if (use == ChunkUse::topk_subset && !c.cp.use_f16 && !said) {
      printf(probed ? "k-NN probe query: every candidate is evaluated with the exact arithmetic (no f32-filtered probe search)\n"
                    : "k-NN masked query: every candidate is evaluated with the exact arithmetic (no f32-filtered masked search)\n");
      said = true;
    }
    KNN_TRY(res.clear(n, st));
    KnnArgs a;
    c.fill_args(&a, n);
    res.fill_args(&a);
    a.cap = rq.cap;
    if (probed) { a.plist = pr.lists; a.pw = rq.pw; }
    if (rq.allow) mask.fill_args(&a);
    KNN_TRY(knn_search(s, c.scratch, a, c.cp, sw, (uint32_t)(c.plan.size() / 2), false, verbosity,
                       probed ? &probe_order : nullptr));
    KNN_TRY(res.deliver(q0, n, c.b.inv, rq.neighbors, rq.distances, st));
  }
  KNN_TRY(finish_query(*this, what));
  if (stats) KNN_TRY(report_stats(*this, rq.report));
  return 0;
}

// The answer of a radius call on its way to the caller: counts, or the hits at the caller's CSR offsets.  A caller on
// the device is written in place; for one on the host a chunk's counts, or its CSR range, are staged on the device (a
// chunk is split until its range fits kQueryChunkBytes).
struct RadiusResult {
  const RadiusRequest &rq;
  bool host = false;
  hipStream_t st = nullptr;
  DeviceArena own;   // this call's own device buffers (nothing to release: the index's stream)
  uint32_t *flag = nullptr;   // raised by a fill in which a query's hit count differs from its range
  uint32_t *counts_dev = nullptr;
  uint64_t *offsets_dev = nullptr;
  struct Staging {
    void *nb = nullptr, *dist = nullptr;
    uint64_t cap = 0;
    ~Staging() { (void)hipFree(nb); (void)hipFree(dist); }
  } stage;
  uint64_t range = 0;   // the hits of the chunk begun last (a fill to the host)

  explicit RadiusResult(const RadiusRequest &rq_) : rq(rq_) {}

  int flag_raised(bool *raised) const {   // (waits for the stream)
    uint32_t f = 0;
    KMX_HIPCP(hipMemcpyAsync(&f, flag, sizeof(f), hipMemcpyDeviceToHost, st));
    KMX_HIPRT(hipStreamSynchronize(st));
    *raised = f != 0;
    return 0;
  }
  // for chunks of at most Qc queries.  A fill's offsets must not decrease: checked here, before anything is written
  int init(const KnnShard &s, uint32_t Qc) {
    host = rq.device_ptrs < 0;
    st = s.stream;
    own.dev = s.dev;
    own.stream = nullptr;
    KNN_TRY(own.alloc(&flag, 1));
    KMX_HIPRT(hipMemsetAsync(flag, 0, sizeof(uint32_t), st));
    if (!rq.fill) return host ? own.alloc(&counts_dev, Qc) : 0;
    if (host) {
      for (uint32_t i = 0; i < rq.Q; i++)
        if (rq.offsets[i] > rq.offsets[i + 1]) return kmcudaInvalidArguments;
      return own.alloc(&offsets_dev, (size_t)Qc + 1);
    }
    KMX_HIPRT(launch_knn_radius_offsets_check(rq.offsets, rq.Q, flag, st));
    bool raised = false;
    KNN_TRY(flag_raised(&raised));
    return raised ? kmcudaInvalidArguments : 0;
  }
  // the chunk from q0 on: of its *n queries as many as the staging budget holds, and a staging that holds their range
  int begin_chunk(uint32_t q0, uint32_t *n) {
    if (!rq.fill || !host) return 0;
    const size_t hit_bytes = sizeof(uint32_t) + (rq.distances ? sizeof(float) : 0);
    *n = knn_fill_chunk_rows(rq.offsets, q0, *n, kQueryChunkBytes / hit_bytes);
    range = rq.offsets[q0 + *n] - rq.offsets[q0];
    if (range <= stage.cap) return 0;
    (void)hipStreamSynchronize(st);   // (the copies out of the old buffers)
    (void)hipFree(stage.nb); (void)hipFree(stage.dist);
    stage.nb = stage.dist = nullptr;
    stage.cap = 0;
    if (hipMalloc(&stage.nb, range * sizeof(uint32_t)) != hipSuccess ||
        (rq.distances && hipMalloc(&stage.dist, range * sizeof(float)) != hipSuccess)) {
      (void)hipGetLastError();
      return kmcudaMemoryAllocationFailure;
    }
    stage.cap = range;
    return 0;
  }
  // where the search of the chunk begun last (n queries from q0 on) writes
  int fill_args(uint32_t q0, uint32_t n, KnnRadiusArgs *ra) const {
    ra->counts = host ? counts_dev : (rq.counts ? rq.counts + q0 : nullptr);
    ra->offsets = nullptr; ra->out_base = 0; ra->neighbors = nullptr; ra->distances = nullptr; ra->flag = flag;
    if (rq.fill && host) {
      KMX_HIPCP(hipMemcpyAsync(offsets_dev, rq.offsets + q0, ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      // (slots of a range the search does not fill -- the call then fails -- read 0xFF)
      if (range) KMX_HIPRT(hipMemsetAsync(stage.nb, 0xFF, range * sizeof(uint32_t), st));
      if (range && rq.distances) KMX_HIPRT(hipMemsetAsync(stage.dist, 0xFF, range * sizeof(float), st));
      ra->offsets = offsets_dev; ra->out_base = rq.offsets[q0];
      ra->neighbors = static_cast<uint32_t *>(stage.nb); ra->distances = static_cast<float *>(stage.dist);
    } else if (rq.fill) {
      ra->offsets = rq.offsets + q0;
      ra->neighbors = rq.neighbors; ra->distances = rq.distances;
    }
    return 0;
  }
  // that chunk to a caller on the host.  (The next chunk overwrites these buffers: the stream orders it behind this
  // one's kernels and copies.)
  int deliver(uint32_t q0, uint32_t n) const {
    if (!host) return 0;
    if (!rq.fill)
      KMX_HIPCP(hipMemcpyAsync(rq.counts + q0, counts_dev, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    else if (range) {
      const uint64_t at = rq.offsets[q0];
      KMX_HIPCP(hipMemcpyAsync(rq.neighbors + at, stage.nb, range * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      if (rq.distances)
        KMX_HIPCP(hipMemcpyAsync(rq.distances + at, stage.dist, range * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    return 0;
  }
};

// The margins of the radius search's cluster prune where no lb table decides: the triangle test with a
// margin for the rounding of its computed terms; the half2 arithmetic's distances carry half-precision errors no such
// margin covers: nothing is pruned there.
// (tests/test_radius_bound_model.py restates these constants and reads them back from this file: change both)
void radius_prune_margins(const KnnIndex &ix, KnnRadiusArgs *ra) {
  const uint32_t D = ix.s.D;
  const bool fp16 = ix.fp16;
  ra->prune_abs = ra->prune_rel = 0.f;
  if (ix.path.strict_h2) {
    ra->prune_abs = INFINITY;
  } else if (ix.s.metric == 0) {
    ra->prune_rel = (float)(1e-5 + 4e-9 * (double)D);
  } else {
    // four computed angles, each acos of a product that is off by at most dp: |acos(a) - acos(b)| <= sqrt(2 |a - b|) * 1.01
    const double dp = (fp16 ? 1.0e-3 : 1.0e-6) + 1.0e-8 * (double)D;
    ra->prune_abs = (float)(4.0 * 1.01 * sqrt(2.0 * dp));
  }
}

// Radius search of one query batch, chunked as topk(); a chunk's lb table (L2, up to 1024 features:
// the prune test) stays within kQueryChunkBytes.  allow: the masked search -- the mask is prepared
// once, behind the unmasked call's refusals, and every chunk prunes with the radii over the allowed rows and runs the
// MASK kernels.
int KnnIndex::radius(const RadiusRequest &rq) {
  if (hipSetDevice(s.dev) != hipSuccess) return kmcudaNoSuchDevice;
  const uint32_t D = s.D, K = s.K;
  const hipStream_t st = s.stream;
  const KnnSwitches sw = knn_switches();
  const bool host = rq.device_ptrs < 0, fill = rq.fill, masked = rq.allow != nullptr;
  const uint32_t Qc = knn_chunk_rows(kQueryChunkBytes, 4 * (size_t)K, sw.query_chunk, rq.Q);

  RadiusResult res(rq);
  KNN_TRY(res.init(s, Qc));
  ArenaScratch mx(s);   // (before `c`: it waits for the stream, then releases)
  QueryMask mask;
  if (masked) KNN_TRY(prepare_mask(rq.allow, host, mx, &mask));
  const float *R = masked ? mask.R : s.R;   // what the prune tests read: the radii over the rows that may be returned
  QueryChunk c;
  KNN_TRY(c.init(*this, Qc, !rq.qassign_in));
  // (a fill's first chunk may be shorter than Qc, and the assignment pass reads Qc rows: defined values for them)
  if (fill && host && !rq.qassign_in) KMX_HIPRT(hipMemsetAsync(c.rows, 0, (size_t)Qc * D * sizeof(float), st));
  // the cluster prune: the lb table (L2, D <= 1024, rows the bounds kernel can read four features at a time; the call
  // fails without its memory), else the triangle test with its margins
  const bool use_lb = s.metric == 0 && D <= 1024 && (s.DP & 3u) == 0 && !path.strict_h2;
  if (use_lb && hipMalloc((void **)&c.scratch.lb, (size_t)K * Qc * sizeof(float)) != hipSuccess) {
    c.scratch.lb = nullptr;
    (void)hipGetLastError();
    return kmcudaMemoryAllocationFailure;
  }
  if (use_lb && path.use_f16 && sw.order != 0 && hipMalloc((void **)&c.scratch.qperm, (size_t)Qc * sizeof(uint32_t)) != hipSuccess) {
    c.scratch.qperm = nullptr;   // (the query order is an optimisation: sorted-position order without it)
    (void)hipGetLastError();
  }
  if (sw.stats) KMX_HIPRT(hipMemsetAsync(s.calced, 0, KNN_STATS * sizeof(unsigned long long), st));

  uint32_t n = 0;
  for (uint32_t q0 = 0; q0 < rq.Q; q0 += n) {
    n = rq.Q - q0 < Qc ? rq.Q - q0 : Qc;
    KNN_TRY(res.begin_chunk(q0, &n));
    KNN_TRY(c.prepare(*this, ChunkUse::radius, q0, n, rq.queries, rq.qassign_in, rq.qassign_out, host));
    const bool f16 = c.cp.use_f16;
    KnnRadiusArgs ra;
    KnnArgs &a = ra.a;
    c.fill_args(&a, n);
    a.k = 0; a.heaps = nullptr; a.out = nullptr; a.outd = nullptr;
    knn_corpus_args(s, f16, R, &a);
    if (masked) mask.fill_args(&a);
    // the bounds of every assigned query, and (f16) the order that brings queries that want the same clusters into
    // the same waves
    if (use_lb && c.assigned)
      KNN_TRY(knn_bound_queries(s, c.scratch, c.b.xs, c.offsets, c.b.mydist, 0, c.assigned, R, f16 ? sw.order : 0, &a));
    ra.radius = rq.r;
    radius_prune_margins(*this, &ra);
    ra.qinv = c.b.inv;
    KNN_TRY(res.fill_args(q0, n, &ra));
    if (f16) {
      KMX_HIPRT(launch_knn_radius_f16(s.metric, ra, (uint32_t)(c.plan.size() / 2), fill, st, masked));
      KnnRadiusArgs rest = ra;
      rest.a.p_base = c.assigned; rest.a.p_end = n;
      KMX_HIPRT(launch_knn_radius_rest(rest, fill, st));
    } else {
      KMX_HIPRT(launch_knn_radius_exact(s.metric, ra, c.cp.strict_h2, fill, st, masked));
    }
    KNN_TRY(res.deliver(q0, n));
  }
  bool raised = false;
  if (res.flag_raised(&raised) != 0) {
    if (verbosity > 0) printf("k-NN radius search failed: %s\n", hipGetErrorString(hipGetLastError()));
    return kmcudaRuntimeError;
  }
  if (sw.stats) KNN_TRY(report_stats(*this, fill ? "radius fill" : "radius count"));
  return raised ? kmcudaInvalidArguments : 0;   // a query's hit count differs from its range
}

// A state under construction (none yet: nothing to do): released with the call, behind a wait for the stream, unless
// the index has adopted it
struct PendingState {
  KnnIndex &ix;
  IndexState t;
  bool adopted = false;
  explicit PendingState(KnnIndex &ix_) : ix(ix_) {}
  ~PendingState() {
    if (adopted || !t.rows.xs) return;
    (void)hipStreamSynchronize(ix.s.stream);
    ix.release_state(t);
  }
};

// One merge (knn_merge.hip): `cur` and the prepared chunk into the buffers of `next`, whose host offsets are made.
int KnnIndex::merge(const IndexState &cur, const AddChunk &c, uint32_t n, IndexState *next) {
  const uint32_t DP = s.DP, K = s.K;
  const hipStream_t st = s.stream;
  const bool f16 = path.use_f16;
  KMX_HIPCP(hipMemcpyAsync(next->offsets, next->off_host.data(), ((size_t)K + 2) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  KMX_HIPRT(hipMemsetAsync(next->stats, 0, 4 * sizeof(uint32_t), st));
  KnnMergeArgs a;
  a.old_rows = cur.rows; a.chunk = c.b; a.out = next->rows;
  a.off_old = cur.offsets; a.boffs = c.offsets; a.off_new = next->offsets;
  a.N_old = cur.N; a.n = n; a.K = K; a.DP = DP;
  KMX_HIPRT(launch_knn_merge_rows(a, st));
  if (f16) {
    KNN_TRY(zero_f16_pad(next->rows, next->N, DP, st));
    KMX_HIPRT(hipMemsetAsync(next->stats_c, 0, 4 * sizeof(uint32_t), st));
  }
  KMX_HIPRT(launch_knn_merge_radii(cur.R, c.rdist, c.offsets, K, next->R, cur.stats, f16 ? cur.stats_c : nullptr, c.stats,
                                   next->stats, f16 ? next->stats_c : nullptr, st));
  return 0;
}

// n_rows more rows, in chunks of one merge each.  Every merge writes a whole new state; the index's
// own buffers are read only, and replaced once the last chunk has been enqueued and the stream has drained without error.
int KnnIndex::add(uint32_t n_rows, const void *rows, const uint32_t *assign_in, uint32_t *assign_out, int32_t device_ptrs) {
  if (hipSetDevice(s.dev) != hipSuccess) return kmcudaNoSuchDevice;
  const int rc = add_chunks(n_rows, rows, assign_in, assign_out, device_ptrs < 0);
  if (rc != 0 && verbosity > 0) printf("k-NN index add failed: %s\n", hipGetErrorString(hipGetLastError()));
  return rc;
}

// (Every return before the adoption leaves the index as it was: the guards wait for the stream, then release the states
// under construction, then the chunk's buffers go.)
int KnnIndex::add_chunks(uint32_t n_rows, const void *rows, const uint32_t *assign_in, uint32_t *assign_out, bool host) {
  const hipStream_t st = s.stream;
  const bool f16 = path.use_f16;
  const uint32_t Cn = knn_add_chunk_rows(n_rows, s.D, s.DP, kQueryChunkBytes, knn_switches().add_chunk);
  AddTimer tm;
  tm.start(knn_switches().add_time);
  AddChunk c;
  KNN_TRY(c.init(*this, Cn, !assign_in));
  const IndexState own = state();
  PendingState cur(*this);   // what the merges so far have made (none before the first)
  for (uint32_t r0 = 0; r0 < n_rows; r0 += Cn) {
    const uint32_t n = n_rows - r0 < Cn ? n_rows - r0 : Cn;
    const bool first = r0 == 0;
    const IndexState &from = first ? own : cur.t;
    PendingState next(*this);
    if (!first && tm.on && hipStreamSynchronize(st) == hipSuccess) tm.fold();   // (the chunk before: its events are reused)
    KNN_TRY(c.prepare(*this, r0, n, rows, assign_in, assign_out, host, tm));
    KNN_TRY(alloc_state(&next.t, from.N + n, f16));
    if (!knn_merge_offsets(from.off_host, c.offs.data(), s.K, n, &next.t.off_host)) return kmcudaRuntimeError;
    tm.mark(3, st);
    KNN_TRY(merge(from, c, n, &next.t));
    tm.mark(4, st);
    // (read and written once: the fp32 rows, the halves and six words per row)
    tm.merged_bytes += 2ull * ((unsigned long long)from.N + n) * ((f16 ? 6ull : 4ull) * s.DP + (f16 ? 24ull : 12ull));
    if (!first) KMX_HIPRT(hipStreamSynchronize(st));   // (the merge reads `cur`, which goes with `next`'s guard)
    std::swap(cur.t, next.t);
  }
  // the half-range flag, once per add (create waits for it too); the chunk's buffers go behind this wait
  uint32_t flag = 0;
  if (f16) KMX_HIPCP(hipMemcpyAsync(&flag, cur.t.stats + 1, sizeof(flag), hipMemcpyDeviceToHost, st));
  KMX_HIPRT(hipStreamSynchronize(st));
  if (tm.on) {
    tm.fold();
    printf("k-NN index add: %u rows in chunks of %u: clusters %.3f ms, preparation %.3f ms, merge %.3f ms (%.3f GB moved, "
           "%.3f TB/s)\n", n_rows, Cn, tm.ms[0], tm.ms[1], tm.ms[2], 1e-9 * (double)tm.merged_bytes,
           tm.ms[2] > 0.f ? 1e-9 * (double)tm.merged_bytes / (double)tm.ms[2] : 0.0);
    fflush(stdout);
  }
  IndexState old = state();
  adopt(cur.t);
  cur.adopted = true;
  release_state(old);
  if (knn_leaves_half_range(&path.use_f16, &path.dp_filter, s.D, flag)) {   // no f16 filter for this index any more
    if (verbosity > 0) say_left_half_range(path);
    IndexState now = state();
    release_f16(now);
    adopt(now);
  }
  return 0;
}

// KMCUDA_AMD_KNN_REMOVE_TIME: the four stages of a remove -- the assignments (scatter and mark), the sort, the copy, the
// member distances and radii --, printed at the end of the call (scripts/knn_remove_bench.py reads the line)
using RemoveTimer = StageEvents<6>;   // (1 -> 2: the host's wait and allocations)

// The listed rows lose their cluster.  A whole new state is built beside the index's own, which is
// read only and replaced once everything has been enqueued and the stream has drained without error.
int KnnIndex::remove(uint32_t n_ids, const uint32_t *ids, uint32_t *n_removed, int32_t device_ptrs) {
  if (hipSetDevice(s.dev) != hipSuccess) return kmcudaNoSuchDevice;
  const hipStream_t st = s.stream;
  const bool host = device_ptrs < 0, f16 = path.use_f16;
  const uint32_t N = s.N, K = s.K, DP = s.DP;
  if (host)
    for (uint32_t i = 0; i < n_ids; i++)
      if (ids[i] >= N) return kmcudaInvalidArguments;
  if (n_ids == 0) {
    if (n_removed) *n_removed = 0;
    return 0;
  }
  RemoveTimer tm;
  tm.start(knn_switches().remove_time);
  ArenaScratch x(s);
  // ---- the ids on the device, every one a row of the index ----
  uint32_t *words = nullptr, *ids_up = nullptr;   // words: [0] the flag of the check, [1] the rows that lose a cluster
  KNN_TRY(x.get(&words, 2));
  KMX_HIPRT(hipMemsetAsync(words, 0, 2 * sizeof(uint32_t), st));
  uint32_t seen[2] = {0, 0};
  if (host) {
    KNN_TRY(x.get(&ids_up, n_ids));
    KMX_HIPCP(hipMemcpyAsync(ids_up, ids, (size_t)n_ids * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    ids = ids_up;
  } else {
    KMX_HIPRT(launch_knn_remove_ids_check(ids, n_ids, N, words, st));
    KMX_HIPCP(hipMemcpyAsync(seen, words, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    KMX_HIPRT(hipStreamSynchronize(st));
    if (seen[0]) return kmcudaInvalidArguments;
  }
  // ---- the assignments the index stands for, the listed rows' set to K ----
  uint32_t *asg = nullptr, *pos = nullptr;
  KNN_TRY(x.get(&asg, N));
  KNN_TRY(x.get(&pos, N));
  tm.mark(0, st);
  KMX_HIPRT(launch_knn_remove_scatter(s.offsets, K, s.inv, N, asg, pos, st));
  KMX_HIPRT(launch_knn_remove_mark(ids, n_ids, K, asg, words + 1, st));
  tm.mark(1, st);
  KMX_HIPCP(hipMemcpyAsync(seen + 1, words + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  KMX_HIPRT(hipStreamSynchronize(st));
  const uint32_t lost = seen[1];
  if (lost == 0) {   // nothing listed had a cluster: the index's buffers have not been touched
    if (n_removed) *n_removed = 0;
    return 0;
  }
  // ---- the new order: the stable sort a fresh index runs over the patched assignments ----
  PendingState next(*this);
  KNN_TRY(alloc_state(&next.t, N, f16));
  uint32_t *keys_tmp = nullptr, *vals_tmp = nullptr, *keys_sorted = nullptr;
  char *sort_temp = nullptr;
  float *rdist = nullptr;
  const size_t sort_bytes = sort_temp_bytes(N, K);
  KNN_TRY(x.get(&keys_tmp, N));
  KNN_TRY(x.get(&vals_tmp, N));
  KNN_TRY(x.get(&keys_sorted, N));
  KNN_TRY(x.get(&sort_temp, sort_bytes + 16));
  KNN_TRY(x.get(&rdist, N));
  KnnSortedRows &out = next.t.rows;
  tm.mark(2, st);
  KMX_HIPRT(launch_inverse_assignments(asg, N, K, keys_tmp, vals_tmp, keys_sorted, out.inv, next.t.offsets, sort_temp,
                                       sort_bytes, st));
  KMX_HIPRT(hipMemsetD32Async((hipDeviceptr_t)(next.t.offsets + K + 1), (int)N, 1, st));
  tm.mark(3, st);
  // ---- every row's own values into their new places ----
  KnnRemoveArgs a;
  a.old_rows = state().rows; a.out = out; a.pos = pos; a.N = N; a.DP = DP;
  KMX_HIPRT(launch_knn_remove_rows(a, st));
  if (f16) {
    KNN_TRY(zero_f16_pad(out, N, DP, st));
    KMX_HIPCP(hipMemcpyAsync(next.t.stats_c, s.stats_c, 4 * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  }
  // (maxima over all rows, and every row stays; the half-range flag cannot rise)
  KMX_HIPCP(hipMemcpyAsync(next.t.stats, s.stats, 4 * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  tm.mark(4, st);
  // ---- what depends on membership, by the kernels of a fresh index ----
  KMX_HIPRT(launch_knn_member(s.metric, out.xs, N, s.D, DP, next.t.offsets, K, s.centroids, out.mydist, rdist, path.strict_h2, st));
  KMX_HIPRT(launch_knn_radii(rdist, next.t.offsets, K, next.t.R, st));
  tm.mark(5, st);
  next.t.off_host.assign((size_t)K + 2, N);
  KMX_HIPCP(hipMemcpyAsync(next.t.off_host.data(), next.t.offsets, ((size_t)K + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (hipStreamSynchronize(st) != hipSuccess) {
    if (verbosity > 0) printf("k-NN index remove failed: %s\n", hipGetErrorString(hipGetLastError()));
    return kmcudaRuntimeError;
  }
  if (tm.on) {
    // (read and written once: the fp32 rows, the halves and one or four words per row)
    const double bytes = 2.0 * (double)N * ((f16 ? 6.0 : 4.0) * DP + (f16 ? 16.0 : 4.0));
    const float copy_ms = tm.elapsed(3, 4);
    printf("k-NN index remove: %u ids, %u rows lost a cluster of %u: assignments %.3f ms, sort %.3f ms, copy %.3f ms "
           "(%.3f GB moved, %.3f TB/s), member distances and radii %.3f ms\n", n_ids, lost, N, tm.elapsed(0, 1),
           tm.elapsed(2, 3), copy_ms, 1e-9 * bytes, copy_ms > 0.f ? 1e-9 * bytes / (double)copy_ms : 0.0, tm.elapsed(4, 5));
    fflush(stdout);
  }
  IndexState old = state();
  adopt(next.t);
  next.adopted = true;
  release_state(old);
  if (n_removed) *n_removed = lost;
  return 0;
}

// R on the host (a window for tests: the radii are otherwise invisible); allow: the radii a masked search prunes with
int KnnIndex::radii(float *out, const uint8_t *allow, int32_t device_ptrs) {
  if (hipSetDevice(s.dev) != hipSuccess) return kmcudaNoSuchDevice;
  ArenaScratch x(s);
  QueryMask mask;
  if (allow) KNN_TRY(prepare_mask(allow, device_ptrs < 0, x, &mask));
  KMX_HIPRT(hipStreamSynchronize(s.stream));
  KMX_HIPCP(hipMemcpy(out, allow ? mask.R : s.R, (size_t)s.K * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

struct kmamd_knn_index {
  KnnIndex ix;
};

// what the caller wrote on its device (device_ptrs >= 0) has to be there before the index's stream reads it
static void sync_callers_writes(int32_t device_ptrs) {
  if (device_ptrs >= 0 && hipSetDevice(device_ptrs) == hipSuccess) (void)hipDeviceSynchronize();
}

// max_distance of the capped calls: not NaN, >= 0; +inf (and whatever exceeds FLT_MAX) means FLT_MAX, no cap
static bool cap_ok(float *cap) {
  if (!(*cap >= 0.f)) return false;
  if (*cap > kNoCap) *cap = kNoCap;
  return true;
}

// Every top-k entry point behind its request: the refusals in their order, the empty batch, the call.  probed: rq.pw
// is the caller's nprobe, any value
static int topk_call(kmamd_knn_index *h, TopkRequest rq, bool probed) {
  if (!cap_ok(&rq.cap) || !h) return kmcudaInvalidArguments;
  KnnIndex &ix = h->ix;
  if (rq.k == 0 || rq.k > 65535u || rq.k > ix.s.N) return kmcudaInvalidArguments;
  if (rq.device_ptrs >= 0 && rq.device_ptrs != ix.s.dev) return kmcudaInvalidArguments;
  if (probed) {
    if (rq.pw < 1 || rq.pw > KNN_PROBE_MAX || rq.pw > ix.s.K) return kmcudaInvalidArguments;
    // the reference's half2 arithmetic has no ranking (kmamd_kmeans_assign_top refuses it likewise): the caller's lists only
    if (!rq.probes_in && ix.fp16 && (ix.path.strict_h2 || knn_switches().fp16_strict)) return kmcudaInvalidArguments;
  }
  if (rq.Q == 0) return kmcudaSuccess;
  if (!rq.queries || !rq.neighbors) return kmcudaInvalidArguments;
  sync_callers_writes(rq.device_ptrs);
  return ix.topk(rq);
}

// ... and every radius entry point
static int radius_call(kmamd_knn_index *h, const RadiusRequest &rq) {
  if (!h) return kmcudaInvalidArguments;
  if (!(rq.r >= 0.f) || rq.r > 3.402823466e+38f) return kmcudaInvalidArguments;   // NaN, negative or infinite
  if (rq.device_ptrs >= 0 && rq.device_ptrs != h->ix.s.dev) return kmcudaInvalidArguments;
  if (rq.Q == 0) return kmcudaSuccess;
  if (!rq.queries || (rq.fill ? !rq.offsets || !rq.neighbors : !rq.counts)) return kmcudaInvalidArguments;
  sync_callers_writes(rq.device_ptrs);
  return h->ix.radius(rq);
}

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
  sync_callers_writes(device_ptrs);   // as knn_cuda()
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

int kmamd_knn_index_query_capped(kmamd_knn_index *h, uint32_t k, float max_distance, uint32_t n_queries,
                                 const void *queries, const uint32_t *query_assignments, uint32_t *neighbors,
                                 float *distances, uint32_t *query_assignments_out, int32_t device_ptrs,
                                 const uint8_t *allow) {
  TopkRequest rq;
  rq.k = k; rq.cap = max_distance; rq.Q = n_queries; rq.queries = queries;
  rq.qassign_in = query_assignments; rq.qassign_out = query_assignments_out;
  rq.neighbors = neighbors; rq.distances = distances; rq.allow = allow; rq.device_ptrs = device_ptrs;
  rq.report = "capped query";
  return topk_call(h, rq, false);
}

int kmamd_knn_index_query(kmamd_knn_index *h, uint32_t k, uint32_t n_queries, const void *queries,
                          const uint32_t *query_assignments, uint32_t *neighbors, float *distances,
                          uint32_t *query_assignments_out, int32_t device_ptrs) {
  return kmamd_knn_index_query_allow(h, k, n_queries, queries, query_assignments, neighbors, distances,
                                     query_assignments_out, device_ptrs, nullptr);
}

int kmamd_knn_index_query_allow(kmamd_knn_index *h, uint32_t k, uint32_t n_queries, const void *queries,
                                const uint32_t *query_assignments, uint32_t *neighbors, float *distances,
                                uint32_t *query_assignments_out, int32_t device_ptrs, const uint8_t *allow) {
  TopkRequest rq;   // (no cap, and no counters line: the uncapped query prints what it always printed)
  rq.k = k; rq.Q = n_queries; rq.queries = queries;
  rq.qassign_in = query_assignments; rq.qassign_out = query_assignments_out;
  rq.neighbors = neighbors; rq.distances = distances; rq.allow = allow; rq.device_ptrs = device_ptrs;
  return topk_call(h, rq, false);
}

int kmamd_knn_index_query_probe_capped(kmamd_knn_index *h, uint32_t k, float max_distance, uint32_t nprobe,
                                       uint32_t n_queries, const void *queries, const uint32_t *probes,
                                       uint32_t *neighbors, float *distances, uint32_t *probes_out, int32_t device_ptrs,
                                       const uint8_t *allow) {
  TopkRequest rq;
  rq.k = k; rq.cap = max_distance; rq.Q = n_queries; rq.queries = queries;
  rq.pw = nprobe; rq.probes_in = probes; rq.probes_out = probes_out;
  rq.neighbors = neighbors; rq.distances = distances; rq.allow = allow; rq.device_ptrs = device_ptrs;
  rq.report = "probe query";
  return topk_call(h, rq, true);
}

int kmamd_knn_index_query_probe_allow(kmamd_knn_index *h, uint32_t k, uint32_t nprobe, uint32_t n_queries,
                                      const void *queries, const uint32_t *probes, uint32_t *neighbors, float *distances,
                                      uint32_t *probes_out, int32_t device_ptrs, const uint8_t *allow) {
  return kmamd_knn_index_query_probe_capped(h, k, kNoCap, nprobe, n_queries, queries, probes, neighbors, distances,
                                            probes_out, device_ptrs, allow);
}

int kmamd_knn_index_query_probe(kmamd_knn_index *h, uint32_t k, uint32_t nprobe, uint32_t n_queries,
                                const void *queries, const uint32_t *probes, uint32_t *neighbors, float *distances,
                                uint32_t *probes_out, int32_t device_ptrs) {
  return kmamd_knn_index_query_probe_allow(h, k, nprobe, n_queries, queries, probes, neighbors, distances, probes_out,
                                           device_ptrs, nullptr);
}

int kmamd_knn_index_radius_count_allow(kmamd_knn_index *h, float radius, uint32_t n_queries, const void *queries,
                                       const uint32_t *query_assignments, uint32_t *counts,
                                       uint32_t *query_assignments_out, int32_t device_ptrs, const uint8_t *allow) {
  RadiusRequest rq;
  rq.r = radius; rq.Q = n_queries; rq.queries = queries;
  rq.qassign_in = query_assignments; rq.qassign_out = query_assignments_out;
  rq.counts = counts; rq.allow = allow; rq.device_ptrs = device_ptrs;
  return radius_call(h, rq);
}

int kmamd_knn_index_radius_count(kmamd_knn_index *h, float radius, uint32_t n_queries, const void *queries,
                                 const uint32_t *query_assignments, uint32_t *counts, uint32_t *query_assignments_out,
                                 int32_t device_ptrs) {
  return kmamd_knn_index_radius_count_allow(h, radius, n_queries, queries, query_assignments, counts,
                                            query_assignments_out, device_ptrs, nullptr);
}

int kmamd_knn_index_radius_fill_allow(kmamd_knn_index *h, float radius, uint32_t n_queries, const void *queries,
                                      const uint32_t *query_assignments, const uint64_t *offsets, uint32_t *neighbors,
                                      float *distances, int32_t device_ptrs, const uint8_t *allow) {
  RadiusRequest rq;
  rq.fill = true; rq.r = radius; rq.Q = n_queries; rq.queries = queries;
  rq.qassign_in = query_assignments;
  rq.offsets = offsets; rq.neighbors = neighbors; rq.distances = distances; rq.allow = allow; rq.device_ptrs = device_ptrs;
  return radius_call(h, rq);
}

int kmamd_knn_index_radius_fill(kmamd_knn_index *h, float radius, uint32_t n_queries, const void *queries,
                                const uint32_t *query_assignments, const uint64_t *offsets, uint32_t *neighbors,
                                float *distances, int32_t device_ptrs) {
  return kmamd_knn_index_radius_fill_allow(h, radius, n_queries, queries, query_assignments, offsets, neighbors,
                                           distances, device_ptrs, nullptr);
}

int kmamd_knn_index_add(kmamd_knn_index *h, uint32_t n_rows, const void *rows, const uint32_t *assignments,
                        uint32_t *assignments_out, uint32_t *first_row, int32_t device_ptrs) {
  if (!h) return kmcudaInvalidArguments;
  KnnIndex &ix = h->ix;
  if (n_rows > 0 && !rows) return kmcudaInvalidArguments;
  if (device_ptrs >= 0 && device_ptrs != ix.s.dev) return kmcudaInvalidArguments;
  if (!knn_add_fits(ix.s.N, n_rows)) return kmcudaInvalidArguments;
  // the reference's half2 arithmetic has no assignment pass (a probed query refuses its ranking likewise): the caller's only
  if (!assignments && ix.fp16 && (ix.path.strict_h2 || knn_switches().fp16_strict)) return kmcudaInvalidArguments;
  const uint32_t first = ix.s.N;
  if (n_rows != 0) {
    sync_callers_writes(device_ptrs);
    KNN_TRY(ix.add(n_rows, rows, assignments, assignments_out, device_ptrs));
  }
  if (first_row) *first_row = first;
  return kmcudaSuccess;
}

int kmamd_knn_index_remove(kmamd_knn_index *h, uint32_t n_ids, const uint32_t *ids, uint32_t *n_removed,
                           int32_t device_ptrs) {
  if (!h) return kmcudaInvalidArguments;
  KnnIndex &ix = h->ix;
  if (n_ids > 0 && !ids) return kmcudaInvalidArguments;
  if (device_ptrs >= 0 && device_ptrs != ix.s.dev) return kmcudaInvalidArguments;
  if (n_ids != 0) sync_callers_writes(device_ptrs);
  return ix.remove(n_ids, ids, n_removed, device_ptrs);
}

int kmamd_knn_index_radii(kmamd_knn_index *h, float *radii) {
  if (!h || !radii) return kmcudaInvalidArguments;
  return h->ix.radii(radii);
}

int kmamd_knn_index_radii_allow(kmamd_knn_index *h, const uint8_t *allow, int32_t device_ptrs, float *radii_host) {
  if (!h || !radii_host) return kmcudaInvalidArguments;
  if (device_ptrs >= 0 && device_ptrs != h->ix.s.dev) return kmcudaInvalidArguments;
  if (allow) sync_callers_writes(device_ptrs);
  return h->ix.radii(radii_host, allow, device_ptrs);
}

int kmamd_knn_index_info(kmamd_knn_index *h, uint32_t *n_rows, uint32_t *n_clustered, int *filter) {
  if (!h) return kmcudaInvalidArguments;
  const KnnIndex &ix = h->ix;
  if (n_rows) *n_rows = ix.s.N;
  if (n_clustered) *n_clustered = ix.off_host[ix.s.K];
  if (filter) *filter = ix.path.use_f16 ? 2 : (ix.path.dp_filter ? 1 : 0);
  return kmcudaSuccess;
}

void kmamd_knn_index_destroy(kmamd_knn_index *h) { delete h; }

}  // extern "C"
