// knn_host.hpp -- the one host pipeline of the k-NN search (knn_host.cpp): the switches, the corpus preparation, the
// block plan, the search launch and the scatter to a caller's device.  Its two callers add their query side:
// knn_cuda()'s self-join (knn_job.cpp) and the query batches of kmamd_knn_index_* (knn_index.cpp).
#pragma once
#include <vector>

#include "host_job.hpp"

namespace kmx {

// What a search launch needs besides the prepared corpus: radix-sort scratch (the CSR of the rows, then the query order
// of a search; it belongs to whoever allocated it) and the optional buffers of the f16 search for up to `rows` queries
// per launch (knn_search allocates them on first use and keeps them for the next launch; they go with the scratch).
struct KnnScratch {
  uint32_t *keys_tmp = nullptr, *vals_tmp = nullptr, *keys_sorted = nullptr;
  void *sort_temp = nullptr;
  size_t sort_bytes = 0, rows = 0;
  float *lb = nullptr;
  uint32_t *qperm = nullptr;
  ~KnnScratch() {
    (void)hipFree(lb);
    (void)hipFree(qperm);
  }
};

// One GPU's prepared copy of the corpus: the arena's buffers and stream, and what knn_prepare_corpus leaves in them.
struct KnnShard : DeviceArena {
  int metric = 0;
  uint32_t N = 0, D = 0, DP = 0, K = 0;
  float mu2 = 0.f;
  const float *samples = nullptr, *centroids = nullptr;
  const uint32_t *assignments = nullptr;
  float *xs = nullptr, *mydist = nullptr, *rdist = nullptr, *R = nullptr, *C = nullptr, *heaps = nullptr;
  // plain squared norms and their maximum stats[0] (the f32 filter's bound; stats[1]: the half-range flag); centred
  // ones (the f16 filter's) where the split leaves them: buffers of their own, or the plain ones overwritten
  float *n2s = nullptr, *n2c = nullptr;
  uint32_t *stats = nullptr, *stats_c = nullptr;
  float *mu = nullptr, *mux = nullptr, *kbias = nullptr;
  uint16_t *xs16 = nullptr;
  uint32_t *inv = nullptr, *offsets = nullptr, *blocks = nullptr, *out = nullptr;
  unsigned long long *calced = nullptr;
  KnnScratch scratch;
  uint32_t first_block = 0, nblocks = 0, p_base = 0, p_end = 0;
};

// The KMCUDA_AMD_* switches of the k-NN entry points, read once per call (tests change them between calls).
struct KnnSwitches {
  bool exact = false;        // KMCUDA_AMD_KNN_EXACT: every candidate with the exact arithmetic
  bool fp16_strict = false;  // KMCUDA_AMD_FP16_STRICT: the reference's half2 arithmetic (fp16x2 only)
  bool filter_f32 = false;   // KMCUDA_AMD_FILTER=f32
  bool tight = true;         // KMCUDA_AMD_KNN_TIGHT=0: the reference's cluster prune test alone
  int order = 3;             // KMCUDA_AMD_KNN_ORDER: how a cluster's queries are grouped into waves (knn_search)
  bool xcd = false;          // KMCUDA_AMD_KNN_XCD: one query cluster's blocks to one XCD (knn_xcd_plan)
  bool stats = false;        // KMCUDA_AMD_KNN_STATS: the f16 search's counters at any verbosity
  unsigned shard_i = 0, shard_n = 0;  // KMCUDA_AMD_KNN_SHARD="i/n" (shard_n = 0: unset)
  size_t query_chunk = 0;    // KMCUDA_AMD_KNN_QUERY_CHUNK: queries per chunk of an index query (0: unset)
  size_t add_chunk = 0;      // KMCUDA_AMD_KNN_ADD_CHUNK: rows per chunk (one merge each) of an index add (0: unset)
  bool add_time = false;     // KMCUDA_AMD_KNN_ADD_TIME: an index add prints the device time of its three stages
  bool remove_time = false;  // KMCUDA_AMD_KNN_REMOVE_TIME: an index remove prints the device time of its four stages
};
KnnSwitches knn_switches();

// Which search runs: dp_filter = the padded width of the matrix-core filter (0: every candidate evaluated exactly), DP
// = the row stride of the sorted copies, use_f16 = the f16 filter (else the f32 one), strict_h2 = the reference's half2
// arithmetic.  The half range can still send a call from the f16 filter to another one (knn_leaves_half_range).
struct KnnPath {
  uint32_t dp_filter = 0, DP = 0;
  bool use_f16 = false, strict_h2 = false;
};
KnnPath knn_choose_path(uint32_t D, bool fp16, int verbosity, const KnnSwitches &sw);

// The half range: a finite row whose centred value is no finite half (`flag`, raised by the gather)
// would be scored NaN by the f16 filter -- the search takes the f32 filter (D <= 256) or the exact kernel instead.
// True if that happened (the caller says so in its own words).
bool knn_leaves_half_range(bool *use_f16, uint32_t *dp_filter, uint32_t D, uint32_t flag);

// The corpus as the caller hands it over (D counts single features, also for fp16x2)
struct KnnCorpus {
  int metric = 0;
  bool fp16 = false;
  uint32_t N = 0, D = 0, K = 0;
  const void *samples = nullptr, *centroids = nullptr;
  const uint32_t *assignments = nullptr;
  int32_t device_ptrs = -1;
};

// Prepares the corpus on every shard (dev set by the caller): staging, the cluster-sorted copies, radii, the K x K
// centroid distances and, for the f16 filter, the centred split.  keep_plain: the centred norms and their maximum get
// buffers of their own (a later search may still take the f32 filter); otherwise they overwrite the plain ones.  Waits
// for the first shard only where the half-range flag or offsets_host (K + 1, may be null) has to reach the host;
// everything else stays enqueued on the shards' streams.  *path and *left_half_range: knn_leaves_half_range.
int knn_prepare_corpus(KnnShard *const *shards, size_t nshards, const KnnCorpus &c, bool keep_plain, KnnPath *path,
                       bool *left_half_range, uint32_t *offsets_host);

// The block plan: (cluster, first position) pairs, qpb consecutive sorted positions of one cluster per block
void knn_block_plan(const uint32_t *offsets, uint32_t K, uint32_t qpb, std::vector<uint32_t> *plan);
inline uint32_t knn_qpb(bool use_f16, uint32_t DP) { return use_f16 ? knn_qpb_f16(DP) : KNN_QPB_F32; }
// KMCUDA_AMD_KNN_XCD: the plan with the blocks of one query cluster on one XCD (empty slots: 0xFFFFFFFF)
std::vector<uint32_t> knn_xcd_plan(const std::vector<uint32_t> &plan);

// The corpus side of a search's arguments from the prepared shard: f16 = the f16 filter's norms and statistics (else
// the plain ones), R = the radii every prune reads (the shard's, or a mask's over the allowed rows), eps = the filters'
// slack.  knn_search fills it; the radius search, which launches kernels of its own, calls it too.
void knn_corpus_args(const KnnShard &s, bool f16, const float *R, KnnArgs *a);

// The second cluster test's table and the query order made from it (L2, D <= 1024), for the sorted query positions
// [p_base, p_end) of the rows qxs (CSR qoffsets, distances to the own centroid qmydist): x.lb, which the caller has
// allocated for p_end - p_base queries (the table's stride), gets every query's bound for every centroid under the
// radii R, and a->lb / a->lb_stride name it; order != 0 and x.qperm there: the queries of a cluster grouped into waves
// by mode `order` (a->qperm; left null where the sort cannot run: sorted-position order, the same lists).
int knn_bound_queries(const KnnShard &s, const KnnScratch &x, const float *qxs, const uint32_t *qoffsets,
                      const float *qmydist, uint32_t p_base, uint32_t p_end, const float *R, int order, KnnArgs *a);

// What gives a probed f16 search its query order: the chunk's raw lists (query order) and sorted position -> query
struct KnnProbeOrder {
  const uint32_t *raw = nullptr, *qinv = nullptr;
};

// One search launch on s.stream.  The caller fills the query side of `a` (p_base / p_end, blocks, heaps, out and, with
// self = false, the q* fields); this adds the corpus side from the prepared shard, the per-query centroid bounds and
// the query order of the f16 search (buffers and sort scratch: `x`, with x.rows >= p_end - p_base) and picks the
// kernel `path` names: the exact one (dp_filter = 0), else the f16 or the f32 filter.  Probe mode (a.plist set, self =
// false): the PROBE kernels, without the centroid bounds; probe_order (null: none) gives the f16 search
// its query order.  Masked (a.allow_bits set, self = false): the caller also sets a.allow_count and
// a.R, the radii over the allowed rows, which every prune here reads instead of the shard's; the MASK kernels.  There
// is no f32-filtered probe or masked kernel: such a call names the f16 filter or none (refused otherwise).
int knn_search(const KnnShard &s, KnnScratch &x, KnnArgs a, const KnnPath &path, const KnnSwitches &sw,
               uint32_t nblocks, bool self, int verbosity, const KnnProbeOrder *probe_order);

// Rows [p_base, p_end) of a search's output (`out` on src_dev in sorted-position order; null: 0xFFFFFFFF, no
// neighbours) into the caller's `neighbors` on device `dev`, by `inv` of src_dev; waits for it.
int knn_scatter_on(int dev, int src_dev, const uint32_t *out, const uint32_t *inv, uint32_t N, uint32_t p_base,
                   uint32_t p_end, uint32_t k, uint32_t *neighbors);

// The ranking of kmamd_kmeans_assign_top in its two parts (assign_top_job.cpp), so that the k-NN index
// can prepare its centroids once and rank every chunk of probed queries with the same kernels.
struct AssignTopRanker {
  int metric = 0;
  uint32_t D = 0, K = 0, K_pad = 0, Kt = 0;
  uint32_t DP = 0;   // the filter's width; 0: the exhaustive kernel alone
  const float *cen = nullptr;
  float *csqr = nullptr, *ct = nullptr;
  unsigned long long *evaluated = nullptr;   // exact keys computed so far (zeroed by prepare)
  AssignTopFilter fa{};
  uint32_t sub = 0;   // rows per score matrix
  // The centroid preparation, enqueued on w.stream; the buffers belong to `w`.  cen: K x D fp32 on w's device.
  // exact_only: no filter panel (KMCUDA_AMD_ASSIGN_TOP=exact for the whole call)
  int prepare(DeviceArena &w, int metric, const float *cen, uint32_t K, uint32_t D, bool exact_only);
  // the buffers of one chunk of up to Nc rows (KMCUDA_AMD_ASSIGN_TOP_ROWS applies); they belong to `w`
  int reserve(DeviceArena &w, uint32_t Nc);
  // top[n x m] of the chunk's n rows (fp32, on the device), enqueued on st; exact_only: the exhaustive kernel this time
  int rank(const float *rows, uint32_t n, uint32_t m, uint32_t *top, bool exact_only, hipStream_t st);
};
bool assign_top_exact_only();   // KMCUDA_AMD_ASSIGN_TOP=exact

// knn_cuda() behind its argument checks (knn_job.cpp); nvirtual: KMCUDA_AMD_VIRTUAL_SHARDS (test hook)
int knn_job_run(const std::vector<int> &devs, int nvirtual, uint32_t k, const KnnCorpus &corpus, int verbosity,
                uint32_t *neighbors);

}  // namespace kmx
