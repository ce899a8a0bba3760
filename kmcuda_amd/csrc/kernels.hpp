// kernels.hpp -- launch interfaces between the HIP kernels (*.hip) and the host engine.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "launch_dispatch.hpp"

namespace kmx {

struct LloydArgs {
  const float *samples;      // N x D row-major (this device's rows)
  uint32_t N, D, K;
  uint32_t K_pad;            // K rounded up to 32 (filter tiles)
  uint32_t DP;               // filter feature padding (0: no MFMA filter for this D)
  uint32_t Kt;               // K rounded up to 64 (row length of ct)
  const float *cfil;         // K_pad x DP sanitised, CENTRED centroid panel (c - mu)
  const float *bias;         // K_pad: -||c - mu||^2/2 (L2) / mu.(c - mu) (angular) / -inf (never chosen)
  const float *mu;           // DP: mean of the finite centroids (zero padded)
  const float *ct;           // D x Kt transposed centroids
  const float *csqr;         // K exact squared norms (reference's sum_squares)
  const uint32_t *stats;     // bits of: [0] max ||c - mu||^2, [1] max bias magnitude, [2] max ||c||^2,
                             //          [3] ||mu||^2, [4] max bias2 magnitude (original-row variant)
  float eps;                 // relative error coefficient of the filter bound
  float tie_slack;           // absolute slack (angular: acos plateau width)
  uint32_t *assignments, *assignments_prev;
  uint32_t *flagged;         // N: rows with three or more contenders (full exact scan)
  uint32_t *pairs;           // 3N: (row, i1, i2) rows with exactly two contenders
  uint32_t *counters;        // [0] changed, [1] flagged, [2] passed (yinyang), [3] pairs, [4] undecided by stage 1,
                             // [kStopFlag] the device-side stop flag
  uint32_t coarse_mfma = 16; // stage 1's MFMA (lloyd_coarse.hpp, SHAPE): 16 = 16x16x32 where it applies, 32 = 32x32x16
};
// counters[kStopFlag] != 0: the stop rule fired ON THE DEVICE (apply_delta_kernel with a threshold): the kernels
// that assign every row return at once, so iterations enqueued past the stop leave the state untouched
// Kernels with one wave per row (four rows per 256-thread block) stride over the rows from a bounded grid: a grid of
// N / 4 blocks x 256 threads passes 2^32 threads at N = 2^26 rows, which the runtime does not launch as asked (found by
// the reference's 167 772 160-row case, test.py:307-326: the k-means++ byte copy was only partly written)
constexpr uint32_t kWaveRowGridMax = 1u << 20;
inline uint32_t wave_row_grid(uint32_t n_rows) {
  const uint32_t g = (n_rows + 3u) / 4u;
  return g < kWaveRowGridMax ? (g ? g : 1u) : kWaveRowGridMax;
}
constexpr uint32_t kStopFlag = 8;
// counters[kCarryCursor]: length of the carried-bounds pass's row list (zeroed by the preparation kernel);
// counters[kCarrySkipped], [kCarrySkipped + 1]: one 64-bit total of the rows the bounds have spared since the engine was made
constexpr uint32_t kCarryCursor = 9, kCarrySkipped = 10;
// counters[kCarryPaired], [kCarryPaired + 1]: 64-bit total of the rows the carried PAIR certificates have sent straight to
// the two-contender kernel (lloyd_carry.hip)
constexpr uint32_t kCarryPaired = 12;
// counters[kDuoCount]: length of stage 1's list of rows whose (two) contenders it knows by index (lloyd_coarse.hpp:
// the four quarters' trackers); zeroed with counters[4] by the preparation kernels
constexpr uint32_t kDuoCount = 14;
// Bounds carried from one Lloyd pass to the next (lloyd_carry.hip): per row an upper bound of the distance to its
// centroid and a lower bound of the distance to every other finite centroid.
struct CarryArgs {
  float *ub = nullptr, *lb = nullptr;
  const uint32_t *row_list = nullptr;   // CARRY == 2: the rows of this pass (carry_skip_kernel's survivors) ...
  const uint32_t *n_list = nullptr;     // ... and their number, on the device
  uint32_t *host_report = nullptr;      // device address of 2 pinned words: [0] <- the list's length (N for a whole pass), [1] <- seq
  uint32_t seq = 0;
  // angular metric: ub[] holds the certified SCORE gap between the row's centroid and every other one instead (the
  // reference decides on products there; |x.(c_new - c_old)| <= ||x|| ||c_new - c_old|| moves it), lb[] is unused
  int angular = 0;
  // The rows stage 2 decides between two contenders (p1, p2) come out of it with l3[] > 0.  L2: an upper bound of BOTH
  // distances in ub[], lb[] void, l3[] a lower bound of the distance to every other finite centroid: while l3 stays
  // above ub under the drifts, the reference's nearest is one of the two and the pair kernel alone looks at the row.
  // Angular: l3[] = the gap by which both contenders' scores exceed every other centroid's, shrunk by the drifts.
  // l3[] == 0: no such statement (stage 1 writes that for every row it sees)
  float *l3 = nullptr;
  uint32_t *p1 = nullptr, *p2 = nullptr;
};
// the device-side stop rule of launch_apply_delta (reference: check_changed, kmeans.cu:697-717)
struct StopCtl {
  float threshold = -1.f;         // stop when (float)reassigned <= threshold (= tolerance * N in float); < 0: no test
  uint32_t *counters = nullptr;   // engine counters: [0] zeroed when the run goes on, [kStopFlag] raised when it stops
  uint32_t *host_tail = nullptr;  // device-visible pinned words: [0..3] reduced counters, [4] stopped, [5] seq
  uint32_t seq = 0;
};

// (filter_dp_for, lloyd_dp_for: launch_dispatch.hpp, next to the width ladders)
hipError_t launch_centroid_prep(int metric, const float *centroids, uint32_t K, uint32_t D, uint32_t K_pad,
                                uint32_t DP, uint32_t Kt, float *csqr, float *bias, float *bias2, float *cfil,
                                float *ct, float *mu, bool freeze_mu, uint32_t *finite, uint32_t *stats, uint32_t *zero_a,
                                uint32_t *zero_b, uint32_t *zero_c, hipStream_t st);
hipError_t launch_lloyd_filter(const LloydArgs &a, hipStream_t st);
hipError_t launch_lloyd_pair(int metric, const LloydArgs &a, const float *centroids, uint32_t grid, hipStream_t st);
hipError_t launch_lloyd_exact(int metric, const LloydArgs &a, const uint32_t *rows, const uint32_t *nrows,
                              uint32_t grid, hipStream_t st);
// the pair rows and the full-scan rows of a pass in ONE launch, operands staged through LDS / prefetched three
// groups deep (lloyd.hip: lloyd_settle_kernel); supported: D % 4 == 0 and 16-byte aligned rows
bool lloyd_settle_supported(const LloydArgs &a, const float *centroids);
hipError_t launch_lloyd_settle(int metric, const LloydArgs &a, const float *centroids, hipStream_t st);

// lloyd_f16.hip -- the two-stage filter on the f16 matrix cores (centred operands), for fp32
// rows and for the fp16x2 path's half rows; decisions identical in kind, refine kernels shared
bool lloyd_filter_f16_supported(uint32_t D, uint32_t DP);
// panelhi = hi(c - mu) rows + clamped biases for the coarse pass, K_pad rounded up to 64 rows,
// (DP + 2) * 2 bytes per row; stats[5] = max ||c' - hi(c')||^2
hipError_t launch_centroid_panelhi(const float *centroids, uint32_t K, uint32_t D, uint32_t K_pad, uint32_t DP,
                                   const uint32_t *finite, const float *mu, const float *bias, void *panelhi,
                                   uint32_t *stats, hipStream_t st);
// the steady-state preparation of the two-stage filter in one kernel (mean frozen); zeroes stats_next
// and the three list counters.  csqr / ct come from launch_centroid_rows on another stream
hipError_t launch_centroid_prep_frozen(int metric, const float *centroids, uint32_t K, uint32_t D, uint32_t K_pad,
                                       uint32_t DP, const float *mu, uint32_t *finite, float *bias, float *bias2,
                                       float *cfil, void *panelhi, uint32_t *stats, uint32_t *stats_next,
                                       uint32_t *zero_a, uint32_t *zero_b, uint32_t *zero_c,
                                       float *drift /* K: ||c - c of the previous pass||, or null; its maximum -> stats[6] */,
                                       uint32_t *zero_d /* or null */, hipStream_t st);
// L2 metric: the centroid update of launch_apply_delta (same formula, same StopCtl) fused in front of that
// preparation -- one launch between the all-reduce and stage 1
hipError_t launch_apply_prep_frozen(const double *delta, const double *dcount_d, float *centroids, uint32_t *ccounts,
                                    const StopCtl &stop, uint32_t K, uint32_t D, uint32_t K_pad, uint32_t DP,
                                    const float *mu, uint32_t *finite, float *bias, float *bias2, float *cfil,
                                    void *panelhi, uint32_t *stats, uint32_t *stats_next, uint32_t *zero_a,
                                    uint32_t *zero_b, uint32_t *zero_c, float *drift, uint32_t *zero_d, hipStream_t st);
// lloyd_carry.hip -- passes that carry per-row distance bounds (CarryArgs): the coarse stage over every row
// (cy.row_list == nullptr: from the row cache) or over the listed rows, leaving fresh bounds; carry_skip moves the
// bounds by the drifts (launch_centroid_prep_frozen) and lists the rows they no longer decide into row_list /
// counters[kCarryCursor] (probe: only counts them)
hipError_t launch_lloyd_coarse_carry(const LloydArgs &a, const void *rows, bool half_rows, const void *xcache,
                                     const float *xmeta, const void *panelhi, uint32_t *undecided, float *und_thr,
                                     const CarryArgs &cy, uint32_t rows_hint, uint32_t *duo, hipStream_t st);
// (cy.l3 / p1 / p2 / finite / pairs: the pair certificates; pairs[3 counters[3]++] = (row, p1, p2))
hipError_t launch_carry_skip(uint32_t N, uint32_t K, const uint32_t *assignments, uint32_t *assignments_prev,
                             const CarryArgs &cy, const float *xmeta, const float *drift, const uint32_t *stats,
                             float tie_slack, uint32_t *row_list, const uint32_t *finite, uint32_t *pairs,
                             uint32_t *counters, bool probe, hipStream_t st, uint32_t wide_dg = 0);
// (wide_dg != 0: xmeta is the streamed filter's record table, lloyd_wide.hip, rows padded to wide_dg features)
// the reference's exact sum_squares (csqr) + the transposed panel (ct) alone: what the pair / exact kernels read
hipError_t launch_centroid_rows(int metric, const float *centroids, uint32_t K, uint32_t D, uint32_t Kt, float *csqr,
                                float *ct, hipStream_t st);
// stage 1 of the default filter: hi.hi products only; rows it cannot decide -> undecided[counters[4]++].
// xcache / xmeta: the engine's row cache (launch_row_cache) or nullptr (operands converted from rows)
// (duo != nullptr: undecided rows whose two contenders stage 1 knows by index go to duo[4 counters[kDuoCount]++]
//  = (row, contender, contender, best score of the others) instead, for launch_lloyd_duo)
hipError_t launch_lloyd_coarse(const LloydArgs &a, const void *rows, bool half_rows, const void *xcache,
                               const float *xmeta, const void *panelhi, uint32_t *undecided, float *und_thr,
                               uint32_t *duo, hipStream_t st);
// stage 2 without its sweep for the duo rows (lloyd_duo.hip): the two contenders scored in fp32, decided like
// launch_lloyd_refine's rows
// cy (a carried pass with pair certificates: cy->l3 != nullptr): the rows leave with stage 2's bounds and certificates
hipError_t launch_lloyd_duo(const LloydArgs &a, const uint32_t *duo, hipStream_t st, const CarryArgs *cy = nullptr);
// stage 2 of the default filter: the undecided rows' contenders (coarse score >= und_thr) scored in fp32
hipError_t launch_lloyd_refine(const LloydArgs &a, const void *rows, bool half_rows, const void *panelhi,
                               const uint32_t *row_list, const float *thr_list, const uint32_t *n_list,
                               uint32_t rows_hint /* expected list length, 0xFFFFFFFF = unknown */, hipStream_t st);
// the same in a carried pass (lloyd_carry.hip): the rows it settles leave with bounds and pair certificates (cy.l3)
hipError_t launch_lloyd_refine_carry(const LloydArgs &a, const void *rows, bool half_rows, const void *panelhi,
                                     const uint32_t *row_list, const float *thr_list, const uint32_t *n_list,
                                     uint32_t rows_hint, const CarryArgs &cy, hipStream_t st);
// x' = x - mu as halves in the coarse kernel's operand order (N rounded up to 256 rows: DP*2 bytes per
// row) + (||x'||^2, x_0) per row (8 bytes); valid while mu is unchanged
hipError_t launch_row_cache(const void *rows, bool half_rows, uint32_t N, uint32_t D, uint32_t DP, const float *mu,
                            void *xcache, float *xmeta, hipStream_t st);

// lloyd_wide.hip -- the assignment filter for D beyond the register-resident kernels: both operands streamed through
// LDS (256 rows x 256 centroids per block, 64-feature chunks), best / second-best per row in registers, no score ever
// written; then the same sweep over the rows it listed for their contenders
hipError_t launch_row_halves(const void *rows, bool half_rows, uint32_t N, uint32_t D, uint32_t DG, const float *mu,
                             void *xg, float *meta /* 4 floats per row, N + 1 records: ||mu|| in the last */, hipStream_t st);
size_t wide_cont_words(uint32_t N);   // contender table: (1 + 16) words per row
// commits / lists (undecided, und_thr, counters[4]) every row, then writes the listed rows' contenders (und_cont).
// cy (carried bounds, as launch_lloyd_coarse_carry): every row (cy->row_list == nullptr) or the rows of cy->row_list,
// and the rows the pass looks at leave with fresh bounds (cy->ub / lb; no pair certificates on this path)
hipError_t launch_lloyd_wide(const LloydArgs &a, const void *xg, const float *meta, uint32_t DG /* % 64 == 0 */,
                             const void *panelhi, uint32_t *undecided, float *und_thr, uint32_t *und_cont, hipStream_t st,
                             const CarryArgs *cy = nullptr);
hipError_t launch_wide_contenders(int metric, const LloydArgs &a, const float *centroids, uint32_t DG,
                                  const uint32_t *und_rows, const uint32_t *und_cont, hipStream_t st);

// update.hip -- centroid update (reference: kmeans.cu:366-429 kmeans_adjust)
size_t sort_temp_bytes(size_t n, uint32_t max_key);
uint32_t move_bucket_stride(uint32_t K);
size_t move_bucket_words(uint32_t K);        // launch_move_deltas' bucket_work, zero-initialised by the owner
uint32_t move_bucket_cap(uint32_t N, uint32_t K);   // rows per (centroid, sign) bucket: bucket_rows is 2 K x cap words
hipError_t launch_inverse_assignments(const uint32_t *assignments, uint32_t N, uint32_t K, uint32_t *keys_tmp,
                                      uint32_t *vals_tmp, uint32_t *keys_sorted, uint32_t *inv,
                                      uint32_t *offsets, void *temp, size_t temp_bytes, hipStream_t st);
// host-side state of the update across calls (engine-owned)
struct MoveState {
  uint32_t *host = nullptr;            // 4 pinned words the kernels report to: [0] events, [1] largest list,
  uint32_t *host_dev = nullptr;        //   [2] undecided rows of the last assignment pass; host_dev: their device address
  uint32_t last_events = 0xFFFFFFFFu;  // newest event count the host knows
  int force = 0;                       // kmamd_set_update_mode
  uint32_t n_radix = 0, n_direct = 0;  // calls by path (KMCUDA_AMD_UPDATE_TRACE: kmeans_cuda prints them at its end)
};
// per-row sample weights (kmamd_set_weights): the weighted instantiations of the sums.  dweight: K + 1 doubles,
// [c] = weight moved into centroid c - weight moved out, [K] = the pass's reassigned weight; win: K doubles of scratch
struct MoveWeights {
  const float *weights;
  double *dweight;
  double *win;
};
hipError_t launch_move_deltas(const float *samples, uint32_t N, uint32_t D, uint32_t K, const uint32_t *prev,
                              const uint32_t *cur, uint32_t *keys_tmp, uint32_t *vals_tmp, uint32_t *keys_sorted,
                              uint32_t *rows_sorted, uint32_t *offsets2, void *temp, size_t temp_bytes,
                              uint32_t *bucket_rows, uint32_t cap, double *delta, int32_t *dcount /* may be null */,
                              double *tail /* fused buffer's [dcount | counters], may be null */,
                              const uint32_t *counters, uint32_t *blockoff, uint32_t *bucket_work, MoveState *ms,
                              hipStream_t st, const MoveWeights *mw = nullptr);
hipError_t launch_adjust_exact(int metric, const float *samples, uint32_t N, uint32_t D, uint32_t K,
                               const uint32_t *prev, const uint32_t *cur, uint32_t *keys_tmp, uint32_t *vals_tmp,
                               uint32_t *keys_sorted, uint32_t *rows_sorted, uint32_t *offsets2, void *temp,
                               size_t temp_bytes, float *work, float *centroids, uint32_t *ccounts, hipStream_t st);
hipError_t launch_apply_delta(int metric, const double *delta, const int32_t *dcount /* or */,
                              const double *dcount_d /* the fused buffer's tail */, uint32_t K, uint32_t D,
                              float *centroids, uint32_t *ccounts, const StopCtl &stop, hipStream_t st,
                              const double *wtail = nullptr /* weighted: [dweight K | reassigned weight], with ... */,
                              double *cweights = nullptr /* ... the K running cluster weights */);
// sample weights: work[0] = their fp64 total (fixed order), work[1] = how many are not finite and > 0;
// work: weights_check_doubles() doubles
size_t weights_check_doubles();
hipError_t launch_weights_check(const float *weights, uint32_t N, double *work, hipStream_t st);
// out[b][i] = sum over b of bufs[b][i] in ascending b, written to every buffer (the one-device stand-in for the
// all-reduce: KMCUDA_AMD_VIRTUAL_SHARDS)
hipError_t launch_sum_buffers(double *const *bufs_dev, uint32_t nbuf, size_t len, hipStream_t st);

// Code objects load on the first use of a kernel of their translation unit: ~24 ms per process in front of the first
// iteration's kernels (16 of them the update's radix sort).  kmeans_cuda() touches them from a helper thread while its
// own thread uploads and seeds (kmcuda_api.cpp: preload_code_objects).
hipError_t preload_update_code();
hipError_t preload_lloyd_f16_code();
hipError_t preload_lloyd_code();
hipError_t preload_lloyd_carry_code();
hipError_t preload_lloyd_duo_code();
hipError_t launch_gather_rows(const float *samples, const uint32_t *idx, uint32_t K, uint32_t D, float *out, hipStream_t st);
// seeding.hip (reference: kmeans.cu:42-67 kmeans_plus_plus, transpose.cu:6-14 copy_sample_t,
// kmeans.cu:674-691 kmeans_calc_average_distance)
hipError_t launch_kmpp_step(int metric, const float *samples, uint32_t N, uint32_t D, const float *centroid,
                            uint32_t cc, float *dists, hipStream_t st);
// k-means++ with the chooser on the device (seeding.hip): step = distances + exact block sums + exponent
// range; totals_host = pinned { double sum_g, sum_d; uint32 emin, emax, bad, chosen } (32 bytes)
// fail (one device word, 0 while all is well): raised by launch_kmpp_choose's kernel at a step the device cannot
// decide; every kmpp kernel launched with it returns at once while it is set (the host enqueues steps ahead)
// out: the step's exponent cut (one device word, read; zero-initialised by the owner, written by launch_kmpp_choose)
// and where the non-zero distances below it are listed instead of summed (kmpp_outlier_bytes() + one count word,
// zero on entry, zeroed again by launch_kmpp_choose) -- seeding.hip: KmppOutlier
struct KmppOutlierBuf {
  uint32_t *ecut = nullptr;
  void *outl = nullptr;
  uint32_t *outl_count = nullptr;
};
size_t kmpp_outlier_bytes();
size_t kmpp_totals_bytes();
hipError_t launch_kmpp_step2(int metric, const float *samples, uint32_t N, uint32_t D, const float *centroid,
                             uint32_t cc, float *dists, void *block_stats, double *bpre, void *totals,
                             const uint32_t *fail, const KmppOutlierBuf &out, hipStream_t st,
                             const float *weights = nullptr, float *terms = nullptr);
// sample weights: terms[s] = fl(weights[s] * dists[s]), what the chooser sums instead of dists[] (the steps above take
// `weights` / `terms` and do it in front of their statistics; the host chooser calls it itself).  fail: may be null
hipError_t launch_kmpp_weigh(const float *dists, const float *weights, uint32_t N, float *terms, const uint32_t *fail,
                             hipStream_t st);
// the reference's chooser (kmcuda.cc:300-326) for step `step` with random number `choice`, on the device, over the
// concatenation of `nshards` row shards (1: the whole job on one GPU): every shard has run the step on its rows
// (launch_kmpp_step2 / _filtered with its own length and buffers); the kernel runs on shards[0]'s device, reads the
// other shards' totals / prefixes / distances in place (peer access), copies the chosen row from its owner into
// centroid slot `step` of EVERY shard, or raises every shard's *fail = step.  offset % 256 == 0 for every shard.
constexpr int kKmppMaxShards = 16;
struct KmppShardPtrs {
  const float *dists;
  const double *bpre;
  void *totals;
  const float *samples;
  float *centroids;
  uint32_t *fail;
  uint32_t offset, length;
  KmppOutlierBuf out;
};
hipError_t launch_kmpp_choose(const KmppShardPtrs *shards, uint32_t nshards, uint32_t N, double choice, uint32_t log2n,
                              uint32_t step, uint32_t D, hipStream_t st);
// filtered k-means++ steps (seeding.hip): a centred BYTE copy of the rows (per-row scale and measured residual), then
// per step the survivors of the k-NN candidate bound get the exact chain.  DP: D rounded up to 128; xs8: N x DP bytes;
// meta: N x 4 floats; stats: 4 words ([2..3]: exact chains run so far, 64 bits); list: N words.
hipError_t launch_kmpp_cache(const float *samples, uint32_t N, uint32_t D, uint32_t DP, double *part, float *mu,
                             void *xs8, float *meta, uint32_t *stats, hipStream_t st);
hipError_t launch_kmpp_step_filtered(int metric, const float *samples, uint32_t N, uint32_t D, uint32_t DP,
                                     const void *xs8, const float *meta, const float *mu, uint32_t *stats,
                                     uint32_t *list, const float *centroid, uint32_t cc, float *dists,
                                     void *block_stats, double *bpre, void *totals, const uint32_t *fail,
                                     const KmppOutlierBuf &out, hipStream_t st, const float *weights = nullptr,
                                     float *terms = nullptr);
size_t kmpp_block_stat_bytes(uint32_t N);
size_t kmpp_blocks(uint32_t N);
size_t kmpp_prefix_doubles(uint32_t N);   // doubles of `bpre`
// AFK-MC2 seeding (seeding.hip; reference kmeans.cu:69-212)
hipError_t launch_afk_qdist(int metric, const float *samples, uint32_t N, uint32_t D, const float *c1, float *dists,
                            hipStream_t st);
hipError_t launch_afk_q(float *q, uint32_t N, float dsum, hipStream_t st);
// n draws of each of `threads` streams (seed, subsequence = thread, offset): out[thread * n + i] (tests)
hipError_t launch_afk_draws(unsigned long long seed, unsigned long long offset, uint32_t threads, uint32_t n, uint32_t *out,
                            hipStream_t st);
hipError_t launch_afk_random_step(uint32_t m, uint64_t seed, uint64_t seq, const float *q, uint32_t N,
                                  uint32_t *choices, float *rand_a, hipStream_t st);
hipError_t launch_afk_min_dist(int metric, uint32_t m, uint32_t k, const float *samples, uint32_t D,
                               const uint32_t *choices, const float *centroids, float *min_dists, hipStream_t st);
hipError_t launch_member_distances(int metric, const float *samples, uint32_t N, uint32_t D,
                                   const float *centroids, const uint32_t *assignments, uint32_t K,
                                   float *dists, hipStream_t st,
                                   bool libm_acos = false /* angular: acosf_fdlibm (exact.hpp), kmamd_kmeans_assign's */);

// assign_dist.hip -- what kmamd_kmeans_assign adds to the assignment pass (assign_job.cpp)
// dists[s] = distance(row s, centroid assignments[s]) as launch_member_distances(..., libm_acos = true) gives it (the
// same bits: distance_vv's under L2, the C library's acosf of distance_vv's product under the angular metric), NaN
// for an assignment >= K (no centroid is read for it); both operands through LDS tiles instead of one line per lane
hipError_t launch_assigned_distances(int metric, const float *samples, uint32_t N, uint32_t D, const float *centroids,
                                     const uint32_t *assignments, uint32_t K, float *dists, hipStream_t st);
// counts[c] += the rows of cluster c, sums[c] += the fp64 sum of their dists[] in a fixed order (either may be null),
// over the CSR launch_inverse_assignments leaves (inv, offsets: K + 1 entries)
hipError_t launch_cluster_stats(const float *dists, const uint32_t *inv, const uint32_t *offsets, uint32_t K,
                                uint32_t *counts, double *sums, hipStream_t st);

// seed_par.hip -- the sampling side of k-means|| seeding (kmamd_kmeans_seed_parallel, seed_par_job.cpp).
// A block is 256 consecutive rows: seed_par_block_count(N) of them, in seed_par_chunk_count(N) chunks of 1024.
size_t seed_par_block_count(uint32_t N);
size_t seed_par_chunk_count(uint32_t N);
// t[s] <- d[s] where d[s] < t[s] (a NaN d changes nothing); rows_first != null: the first update -- t starts at +inf
// and a row whose first feature is NaN (rows_first: the N x D fp32 rows) gets the term 0.  bsum[b] = the fp64 sum of
// block b's terms (NaN and inf count as 0) in a fixed tree, *phi = their sum in a fixed order.
hipError_t launch_seed_par_update(float *t, const float *d, uint32_t N, const float *rows_first, uint32_t D,
                                  double *bsum, double *phi, hipStream_t st);
// Row s is drawn iff U(seed, round, s) * *phi < (double)oversampling * (double)t[s] (include/kmcuda_amd.h).  draw:
// bcount[b] = block b's drawn rows, boff[b] their exclusive prefix inside b's chunk, aux[c] the chunks' totals,
// carry[c] their exclusive prefix and carry[chunk count] the number of drawn rows M.  fill: ids[0 .. M) the drawn rows
// in ascending order, cand32 (M x D) their rows.
hipError_t launch_seed_par_draw(const float *t, uint32_t N, uint32_t seed, uint32_t round, const double *phi,
                                float oversampling, uint32_t *bcount, uint32_t *boff, uint32_t *aux, uint32_t *carry,
                                hipStream_t st);
hipError_t launch_seed_par_fill(const float *t, uint32_t N, uint32_t seed, uint32_t round, const double *phi,
                                float oversampling, const uint32_t *boff, const uint32_t *carry, uint32_t M,
                                const float *rows32, uint32_t D, uint32_t *ids, float *cand32, hipStream_t st);
// counts[a] += 1 for every row whose assignment a is below M
hipError_t launch_seed_par_weights(const uint32_t *assignments, uint32_t N, uint32_t M, uint32_t *counts,
                                   hipStream_t st);
// out[j] = in[idx[j]] for j < M, rows of D floats (in32 -> out32) and / or of D halves (in16 -> out16)
hipError_t launch_seed_par_gather(const float *in32, const void *in16, const uint32_t *idx, uint32_t M, uint32_t D,
                                  float *out32, void *out16, hipStream_t st);
// *best = min over the rows whose first feature is not NaN of (s - start) mod N (the caller sets it to all ones)
hipError_t launch_seed_par_first_valid(const float *rows, uint32_t N, uint32_t D, uint32_t start,
                                       unsigned long long *best, hipStream_t st);

// minibatch.hip -- mini-batch K-means (kmamd_minibatch_*, minibatch_job.cpp)
// One step's update of the resident state, in place and in one launch, over the CSR launch_inverse_assignments leaves
// for the batch (inv, offsets: K + 1 entries): for every centroid c with members, n_c = the fp64 sum of their weights
// (weights == nullptr: their number), S_c = the fp64 sum of w * x over them in list_sum.hpp's association,
// W' = W + n_c, C' = (float)((C W + S_c) / W') (L2) or (float)((C W + S_c) / |C W + S_c|) (angular).  A centroid
// without members keeps C and W bit for bit.  rows: n x D fp32; weights: n, finite and > 0.
hipError_t launch_minibatch_update(int metric, const float *rows, const float *weights, const uint32_t *inv,
                                   const uint32_t *offsets, uint32_t K, uint32_t D, float *centroids,
                                   double *cluster_weights, hipStream_t st);
// out row j = corpus row floor(h(seed, step, j) N / 2^64) for j < batch (hash_draw.hpp), copied as it is -- D floats,
// or D halves (fp16) --, and weights_out[j] = that row's weight (weights != nullptr)
hipError_t launch_minibatch_draw_gather(const void *corpus, uint64_t N, uint32_t D, bool fp16, const float *weights,
                                        uint32_t seed, uint32_t step, uint32_t batch, void *out, float *weights_out,
                                        hipStream_t st);

// assign_top.hip -- the m nearest centroids of every row (kmamd_kmeans_assign_top, assign_top_job.cpp)
// top[s * m + j] = the j-th centroid of row s by (key, index), K where fewer qualify; *evaluated += the exact keys
// computed.  The exhaustive kernel: every row of [0, N) (rows == nullptr) or rows[0 .. *nrows), N then bounding the grid
hipError_t launch_assign_top_exact(int metric, const float *samples, uint32_t N, uint32_t D, const float *ct,
                                   const float *csqr, uint32_t K, uint32_t Kt, uint32_t m, const uint32_t *rows,
                                   const uint32_t *nrows, uint32_t *top, unsigned long long *evaluated, hipStream_t st);
// the filtered path: what centroid_prep left (cfil, bias, mu, stats: launch_centroid_prep; DP = filter_dp_for(D) != 0)
// and the buffers of one sub-chunk: scores (rows x K_pad floats), meta (rows x 4 floats); fb_rows / fb_count: the rows
// handed to launch_assign_top_exact (chunk-relative indices; fb_count zeroed by the owner)
struct AssignTopFilter {
  int metric;
  uint32_t D, DP, K, K_pad, m;
  const float *centroids, *csqr, *cfil, *bias, *mu;
  const uint32_t *stats;
  float eps;
  float *scores;
  float4 *meta;
  uint32_t *fb_rows, *fb_count;
  unsigned long long *evaluated;
};
// rows [row0, row0 + n) of a chunk: `samples` and `top` point at row row0
hipError_t launch_assign_top_filter(const AssignTopFilter &a, const float *samples, uint32_t n, uint32_t row0,
                                    uint32_t *top, hipStream_t st);
// dists[s * m + j] = distance(row s, centroid top[s * m + j]) as launch_assigned_distances gives it, NaN for K
hipError_t launch_assign_top_distances(int metric, const float *samples, uint32_t N, uint32_t D,
                                       const float *centroids, uint32_t K, uint32_t m, const uint32_t *top,
                                       float *dists, hipStream_t st);

// yinyang.hip (reference: kmeans.cu:431-672)
hipError_t launch_yy_init(int metric, const float *xt, uint32_t len, uint32_t D, uint32_t G, const float *centroids,
                          const uint32_t *assignments, const uint32_t *cperm, const uint32_t *gstart, float *bounds,
                          hipStream_t st);
hipError_t launch_yy_group_max(uint32_t K, uint32_t D, uint32_t G, const uint32_t *groups, const float *drifts,
                               float *gdrifts, hipStream_t st);
hipError_t launch_yy_drifts(int metric, const float *centroids, uint32_t K, uint32_t D, uint32_t G,
                            const uint32_t *groups, float *drifts, float *gdrifts, hipStream_t st);

// yinyang_mfma.hip: the same steps with the matrix-core filter in front of the exact arithmetic
struct YyArgs {
  const float *samples;      // len x D row-major
  const float *centroids;    // K x D original values (exact chains)
  uint32_t len, D, DP, K, K_pad, G;
  const float *cfil, *bias, *mu;  // centred panel of centroid_prep (ascending c)
  const uint32_t *stats;
  float eps;
  const uint32_t *groups;    // K, padded with 0xFFFFFFFF to a multiple of 64
  const float *drifts, *gdrifts;
  uint32_t *assignments;
  float *bounds;
  const uint32_t *passed;
  const uint32_t *count_ptr; // length of `passed` (counters + 2, or counters + 5 for the fall-back list)
  uint32_t *counters;        // + [5] rows of the hinted kernel handed to the plain one
  uint32_t *stat_stripes;    // 64 x 16 words: the hinted kernel's statistics ([6] rows, [7] handed over, [8..11] why), summed by the reader
  // hinted local filter (yinyang_hint.hip)
  const void *panelhi;       // hi halves of the centred panel (centroid_panelhi_kernel), DP halves per row
  const void *xcache;        // the engine's row cache (lloyd_f16.hip: row_cache_kernel) for the SAME mean, or null:
  const float *xmeta;        //   hi halves of x - mu in operand order + (||x'||^2, ||x' - hi(x')||^2) per row
  float *hint;               // per passed row: S' >= upper bound (or +inf: no hint)
  uint32_t *flag_rows;       // rows the hinted kernel could not settle
  const uint32_t *gfirst, *gsecond;  // G: the two smallest member indices of every group (0xFFFFFFFF: none)
  // yy_init: group-sorted padded panel
  const float *pfil, *pbias;
  const uint32_t *pids, *pmeta, *cperm, *gstart;
  uint32_t nslots;
};
hipError_t launch_yy_local_mfma(int metric, const YyArgs &a, hipStream_t st);
// yinyang_hint.hip: coarse second-best estimate per passed row (f16 matrix cores), then the local filter
// with that estimate as its candidate threshold; rows it cannot settle go to flag_rows (counters[5])
bool yy_hint_supported(uint32_t DP);
hipError_t launch_yy_hint(int metric, const YyArgs &a, hipStream_t st);
hipError_t launch_yy_local_hint(int metric, const YyArgs &a, hipStream_t st);
// yinyang_init.hip: the same step with the exact chains fed from registers and LDS (original-value panel)
hipError_t launch_yy_init_lds(int metric, const YyArgs &a, hipStream_t st);
hipError_t launch_yy_orig_panel(int metric, const float *centroids, uint32_t D, uint32_t DP, const uint32_t *pids,
                                uint32_t nslots, float *pfil, float *pbias, hipStream_t st);
hipError_t launch_yy_global_filter(int metric, const float *samples, uint32_t len, uint32_t D, uint32_t K, uint32_t G,
                                   const float *centroids, const float *drifts, const float *gdrifts,
                                   const uint32_t *assignments, uint32_t *assignments_prev, float *bounds,
                                   uint32_t *passed, uint32_t *counters, hipStream_t st);
hipError_t launch_yy_local_filter(int metric, const float *samples, uint32_t len, uint32_t D, uint32_t K, uint32_t G,
                                  const float *centroids, const uint32_t *groups, const float *drifts,
                                  const float *gdrifts, uint32_t *assignments, float *bounds, const uint32_t *passed,
                                  uint32_t *counters, hipStream_t st);

// knn.hip (reference: knn.cu)
// queries (consecutive sorted positions of one cluster) per block: f32 filter 4 waves x 32, f16 filter
// knn16_waves(DP) x knn16_nset(DP) x 32
// Rows up to 256 features: 8 waves x 2 operand sets = 512 queries share every staged candidate tile, ONE block per CU
// (round 5: 4 waves x 2 sets, two blocks per CU, until then -- 2 bytes fetched per scored pair, 4.3 TB for config D's
// share, the kernel HBM co-bound; 8-wave blocks halve the fetches -- 2.27 TB by FETCH_SIZE -- and take 1.02 s against
// 1.10, profiles/r5e_knn_filter_8wave_blocks_ab.log).  Wider rows (DP = 512 / 768 / 1024): ONE operand set per wave (a
// lane's half of a 512-feature row in halves is 128 registers) and four waves (768 / 1024: a wave needs its SIMD to
// itself, 512 registers), one 32-candidate sub-tile per staged tile (32 / 48 / 64 KB).
#ifndef KNN16_WAVES_NARROW
#define KNN16_WAVES_NARROW 8    // waves per block, DP <= 256
#define KNN16_NSET 2            // 32-query operand sets per wave, DP <= 256
#endif
#ifndef KNN16_SUB
#define KNN16_SUB 2             // 32-candidate sub-tiles per staged tile (per barrier)
#endif
#ifndef KNN16_NBUF
#define KNN16_NBUF 2            // LDS ring of candidate tiles (knn_f16.hip)
#endif
#ifndef KNN16_PD
#define KNN16_PD 3              // candidate fragments in flight per wave
#endif
#define KNN16_PAD_ROWS 64   // rows of xs16 / entries of kbias the caller allocates (and the split zeroes) past N
constexpr int knn16_waves(int DP) { return DP > 256 ? 4 : KNN16_WAVES_NARROW; }
constexpr int knn16_blocks_per_cu(int DP) { return DP > 512 ? 1 : (DP > 256 ? 2 : (KNN16_WAVES_NARROW > 4 ? 1 : 2)); }
constexpr int knn16_nset(int DP) { return DP > 256 ? 1 : KNN16_NSET; }
constexpr int knn16_sub(int DP) { return DP > 256 ? 1 : KNN16_SUB; }
constexpr int knn16_nbuf(int DP) { return DP > 256 ? 2 : KNN16_NBUF; }   // (the wide instantiations' tiles: two buffers fill their LDS)
constexpr uint32_t KNN_QPB_F32 = 128;
constexpr uint32_t knn_qpb_f16(uint32_t DP) { return (uint32_t)knn16_waves((int)DP) * (uint32_t)knn16_nset((int)DP) * 32u; }
struct KnnArgs {
  const float *xs;          // N x DP cluster-sorted rows (zero padded to DP)
  const float *n2s;         // N plain squared norms of the sorted rows
  const uint32_t *inv;      // N: sorted position -> sample index (inverse assignments)
  const uint32_t *offsets;  // K+1: cluster c occupies positions [offsets[c], offsets[c+1])
  const float *mydist;      // N: exact distance of each sorted row to its own centroid
  const float *R, *C;       // K radii, K x K centroid distances
  const uint32_t *blocks;   // (cluster, first position) per block of KNN_QPB_* queries
  const uint32_t *stats;    // [0] max squared norm bits
  uint32_t N, D, DP, K, k;
  uint32_t p_base, p_end;   // this launch covers sorted positions [p_base, p_end)
  float eps;
  // f16 matrix-core filter (knn_f16.hip): centred hi/lo-split rows; n2s then holds the CENTRED squared
  // norms, mux[p] = mu.(x_p - mu), mu2 = ||mu||^2
  const void *xs16;         // (N + KNN16_PAD_ROWS) x DP halves
  const float *mux;
  const float *kbias;       // N + KNN16_PAD_ROWS: -0.5 * centred squared norm (L2) / mu.(x - mu) (angular)
  float mu2;
  // optional (L2, f16 filter): lb[c * lb_stride + (p - p_base)] <= d(x_p, centroid c) - R[c] in the reference's
  // arithmetic (knn_centroid_bounds_kernel); nullptr: the reference's prune test alone
  const float *lb = nullptr;
  size_t lb_stride = 0;
  // optional (f16 filter): slot i of the launch's block plan (sorted position p_base + i) handles the query at sorted
  // position qperm[i] of the same cluster (launch_knn_query_order); nullptr: i itself
  const uint32_t *qperm = nullptr;
  float *heaps;             // (p_end - p_base) x 2k
  uint32_t *out;            // (p_end - p_base) x k, sorted-position order
  unsigned long long *calced;  // [0] pairs the REFERENCE's prune rule visits (knn.cu:228); knn_f16.hip also: [1] pairs
                               // scored on the matrix cores (32 x 32 per wave, operand set and sub-tile), [2] of those:
                               // live, unpruned query x real candidate, [3] exact chains evaluated, [4] what [1] would
                               // be if an operand set without a visiting query were not scored
  // The query side (kmamd_knn_index_query: the search kernels' SELF = false instantiations).  knn_cuda's self-join
  // reads its queries from the candidate side above (SELF = true) and leaves these unread; a query batch has its own
  // cluster-sorted rows (qxs: DP-padded fp32, the exact chains; qxs16: centred halves, the f16 filter's B operand),
  // norms (qn2s: plain for the f32 filter, centred for the f16 one), mu.(x - mu) (qmux), distances to their own
  // centroid (qmydist) and CSR offsets (qoffsets, K + 1: own_end, the exact kernel's cluster_of).  Block plan, qperm,
  // lb, heaps and out are indexed by QUERY positions; offsets / xs / xs16 / kbias / inv stay the corpus's.
  const float *qxs = nullptr, *qn2s = nullptr, *qmux = nullptr, *qmydist = nullptr;
  const void *qxs16 = nullptr;
  const uint32_t *qoffsets = nullptr;
  float *outd = nullptr;       // query mode, optional: (p_end - p_base) x k distances beside `out`
  // Probe mode (kmamd_knn_index_query_probe, the search kernels' PROBE instantiations): the query at
  // sorted position p visits its own cluster, then only the clusters of plist[(p - p_base) * pw ..]: pw ids in
  // ascending order without the own cluster, padded with 0xFFFFFFFF (launch_knn_probe_lists).  Unread otherwise.
  const uint32_t *plist = nullptr;
  uint32_t pw = 0;
  // Masked search (kmamd_knn_index_query_allow / _probe_allow, the search kernels' MASK instantiations; DESIGN.md
  // 4.17): bit p & 31 of allow_bits[p >> 5] says whether the corpus row at sorted position p may enter a heap
  // (launch_knn_mask_pack: zeros behind the last clustered row, through the tile padding and one word further);
  // allow_count[c] = the allowed rows of cluster c (0: the cluster is walked over like one without rows).  R then holds
  // the radii over the allowed rows.  Unread otherwise.
  const uint32_t *allow_bits = nullptr;
  const uint32_t *allow_count = nullptr;
  // Capped search (kmamd_knn_index_query_capped / _probe_capped): wherever the procedure reads the kth
  // distance it reads min(kth, cap) -- the push test, both cluster tests and the filters' threshold.  Read in query
  // mode only (knn_cuda's SELF instantiations never load it); FLT_MAX: the uncapped search, bit for bit.
  float cap = 3.402823466e+38f;
};
// the 64-bit words of KnnArgs::allow_bits for an index of N rows: every position a tile can name, plus the word the
// f16 search's two-word read reaches behind it
constexpr size_t knn_mask_words64(uint32_t N) { return ((size_t)N + KNN16_PAD_ROWS + 63) / 64 + 1; }
constexpr int KNN_STATS = 5;
constexpr uint32_t KNN_PROBE_MAX = 64;        // the widest probe list: one entry per lane
constexpr uint32_t KNN_PROBE_BITMAP_K = 65536;  // the f16 probe search keeps a K-bit visit map in LDS: 8 KB at most
// mu (the f16 filter's centre, else null): stats[1] = 1 if a finite row of a cluster leaves the half range once centred
hipError_t launch_knn_gather(const float *samples, uint32_t N, uint32_t D, uint32_t DP, const uint32_t *inv,
                             float *xs, float *n2s, uint32_t *stats, const float *mu, const uint32_t *offsets, uint32_t K,
                             hipStream_t st);
hipError_t launch_knn_prep(int metric, const float *xs, uint32_t N, uint32_t D, uint32_t DP, const uint32_t *offsets,
                           uint32_t K, const float *centroids, float *mydist, float *rdist, float *R, float *C,
                           bool strict_h2, hipStream_t st);
// self = false (the search kernels' query mode, KnnArgs::q*): the candidate distances of the member kernel without the
// radius reduction -- mydist of every sorted row of a query batch (rdist: scratch of N floats)
hipError_t launch_knn_member(int metric, const float *xs, uint32_t N, uint32_t D, uint32_t DP, const uint32_t *offsets,
                             uint32_t K, const float *centroids, float *mydist, float *rdist, bool strict_h2,
                             hipStream_t st);
// query preparation: eff[q] = assignments[q] for a row of finite features, K ("no cluster") for a row with a NaN or
// inf feature; a finite row whose assignment is >= K or names a non-finite centroid raises flags[0] (an invalid
// caller-supplied assignment)
hipError_t launch_knn_query_clusters(const float *rows, uint32_t Q, uint32_t D, const uint32_t *assignments, uint32_t K,
                                     const float *centroids, uint32_t *eff, uint32_t *flags, hipStream_t st);
hipError_t launch_knn_filter(int metric, const KnnArgs &a, uint32_t nblocks, hipStream_t st, bool self = true);
// lb[c * stride + (p - p_base)] for the sorted positions [p_base, p_end) and all K centroids (L2, D <= 1024)
hipError_t launch_knn_centroid_bounds(const float *xs, uint32_t D, uint32_t DP, uint32_t p_base, uint32_t p_end,
                                      const float *centroids, uint32_t K, const float *R, float *lb, size_t stride,
                                      hipStream_t st);
bool launch_knn_query_order(const float *lb, size_t stride, const uint32_t *offsets, uint32_t K, uint32_t p_base,
                            uint32_t p_end, uint32_t *keys_tmp, uint32_t *vals_tmp, uint32_t *keys_sorted,
                            uint32_t *qperm, void *temp, size_t temp_bytes, hipStream_t st, int mode,
                            const float *mydist, const float *R);
// Probe mode.  probes: Q x pw raw lists in the caller's query order (column 0: the own cluster; K: a filler); qinv:
// sorted query position -> query.  lists[p * pw ..]: the list of the query at sorted position p as KnnArgs::plist
// wants it.  An entry > K raises *flag.
hipError_t launch_knn_probe_lists(const uint32_t *probes, uint32_t pw, uint32_t Q, const uint32_t *qinv, uint32_t K,
                                  uint32_t *lists, uint32_t *flag, hipStream_t st);
// qassign[i] = probes[i * pw]: a chunk's own clusters
hipError_t launch_knn_probe_column0(const uint32_t *probes, uint32_t pw, uint32_t Q, uint32_t *qassign, hipStream_t st);
// launch_knn_query_order with the key (own cluster, second entry of the raw probe list): pw >= 2
bool launch_knn_probe_order(const uint32_t *probes, uint32_t pw, const uint32_t *qinv, const uint32_t *offsets,
                            uint32_t K, uint32_t p_base, uint32_t p_end, uint32_t *keys_tmp, uint32_t *vals_tmp,
                            uint32_t *keys_sorted, uint32_t *qperm, void *temp, size_t temp_bytes, hipStream_t st);
// strict_h2 (both): the reference's half2 arithmetic on rows that hold half values (KMCUDA_AMD_FP16_STRICT)
// probe (query mode only): own cluster, then KnnArgs::plist
// mask (query mode only): the MASK instantiations, KnnArgs::allow_bits / allow_count set
hipError_t launch_knn_exact(int metric, const KnnArgs &a, bool strict_h2, hipStream_t st, bool self = true,
                            bool probe = false, bool mask = false);
hipError_t launch_knn_split(int metric, const float *xs, uint32_t N, uint32_t D, uint32_t DP, const float *mu,
                            void *xs16, float *n2c, float *mux, float *kbias, uint32_t *stats, hipStream_t st);
// probe (query mode only, K <= KNN_PROBE_BITMAP_K): the PROBE instantiations
// mask (query mode only, with or without probe): the MASK instantiations
hipError_t launch_knn_filter_f16(int metric, const KnnArgs &a, uint32_t nblocks, hipStream_t st, bool self = true,
                                 bool probe = false, bool mask = false);
hipError_t launch_knn_scatter(const uint32_t *sorted_out, const uint32_t *inv, uint32_t p_base, uint32_t p_end,
                              uint32_t k, uint32_t *neighbors, hipStream_t st);

// knn_merge.hip -- rows added to an index (kmamd_knn_index_add).  What an index keeps per sorted row;
// xs16 / n2c / mux / kbias only while it runs the f16 filter (null otherwise, on all three sides of a merge)
struct KnnSortedRows {
  float *xs, *n2s, *mydist, *n2c, *mux, *kbias;
  uint16_t *xs16;
  uint32_t *inv;
};
// One merge: destination position p of cluster c (K: no cluster) at rank j = p - off_new[c] takes the index's row
// off_old[c] + j while j is below the cluster's old size, else the chunk's row boffs[c] + j - that size, whose inv is
// the chunk's row number: N_old is added.  off_old / off_new / boffs: K + 1 entries on the device.
struct KnnMergeArgs {
  KnnSortedRows old_rows, chunk, out;
  const uint32_t *off_old, *boffs, *off_new;
  uint32_t N_old, n, K, DP;
};
hipError_t launch_knn_merge_rows(const KnnMergeArgs &a, hipStream_t st);
// R_new[c] = max(R_old[c], the chunk's largest rdist in c), NaN only while c stays empty; the statistics: stats_new[0]
// / stats_c_new[0] (null: none) = the larger of the old maximum and the chunk's (bstats[0] plain, bstats[2] centred),
// stats_new[1] = the old half-range flag | bstats[1]
hipError_t launch_knn_merge_radii(const float *R_old, const float *rdist, const uint32_t *boffs, uint32_t K, float *R_new,
                                  const uint32_t *stats_old, const uint32_t *stats_c_old, const uint32_t *bstats,
                                  uint32_t *stats_new, uint32_t *stats_c_new, hipStream_t st);

// knn_remove.hip -- rows removed from an index (kmamd_knn_index_remove).
// *flag |= 1 if one of ids[0 .. n) (device) is >= N
hipError_t launch_knn_remove_ids_check(const uint32_t *ids, uint32_t n, uint32_t N, uint32_t *flag, hipStream_t st);
// the index's CSR (offsets: K + 1 entries, inv: sorted position -> row) back by row id: asg[row] = its cluster (K:
// none), pos[row] = its sorted position
hipError_t launch_knn_remove_scatter(const uint32_t *offsets, uint32_t K, const uint32_t *inv, uint32_t N, uint32_t *asg,
                                     uint32_t *pos, hipStream_t st);
// asg[ids[i]] = K for every i < n (ids < N); *count += the distinct ids whose entry was below K
hipError_t launch_knn_remove_mark(const uint32_t *ids, uint32_t n, uint32_t K, uint32_t *asg, uint32_t *count,
                                  hipStream_t st);
// The gather: destination position p takes the values of the index's position pos[out.inv[p]] -- xs, n2s and, where
// out.xs16 is set, xs16 / n2c / mux / kbias.  out.inv holds the new order already; out.mydist is left alone.
struct KnnRemoveArgs {
  KnnSortedRows old_rows, out;
  const uint32_t *pos;
  uint32_t N, DP;
};
hipError_t launch_knn_remove_rows(const KnnRemoveArgs &a, hipStream_t st);
// knn.hip: R[c] = the largest rdist of cluster c's sorted positions, NaN for an empty cluster (launch_knn_prep's last step)
hipError_t launch_knn_radii(const float *rdist, const uint32_t *offsets, uint32_t K, float *R, hipStream_t st);

// knn_mask.hip -- the allow-mask of a masked query (kmamd_knn_index_query_allow).
// allow: one byte per row id (device), inv: sorted position -> row id (N), assigned: the device word that holds the
// number of clustered rows (offsets + K).  bits (knn_mask_words64(N) words, all of them written): bit p & 63 of word
// p >> 6 = allow[inv[p]] != 0 for p < *assigned, 0 from there on
hipError_t launch_knn_mask_pack(const uint8_t *allow, const uint32_t *inv, uint32_t N, const uint32_t *assigned,
                                unsigned long long *bits, hipStream_t st);
// launch_knn_radii over the rows whose bit is set: R[c] = their largest rdist (NaN where cluster c has none),
// count[c] = how many they are
hipError_t launch_knn_masked_radii(const float *rdist, const uint32_t *offsets, uint32_t K, const uint32_t *bits,
                                   float *R, uint32_t *count, hipStream_t st);

// knn_radius.hip -- radius search of a query batch (kmamd_knn_index_radius_*).  `a` is the query mode's
// KnnArgs (heaps / out / outd / k unread).  Query i of the chunk (caller's order; qinv: sorted query position -> i)
// gets counts[i], or its hits at [offsets[i], offsets[i + 1]) of neighbors / distances, both addressed relative to
// out_base (the chunk's staged range starts there; 0: the caller's own buffers).
struct KnnRadiusArgs {
  KnnArgs a;
  float radius;
  // the triangle prune's margin where a.lb is null: prune_abs + prune_rel * (C + d + R); prune_abs = inf: no prune
  float prune_abs, prune_rel;
  const uint32_t *qinv;
  uint32_t *counts;           // count form
  const uint64_t *offsets;    // fill form: n + 1 entries, non-decreasing
  uint64_t out_base;
  uint32_t *neighbors;
  float *distances;           // optional
  uint32_t *flag;             // fill form: |= 1 if a query's hit count differs from its range
};
// mask (both): the MASK instantiations (kmamd_knn_index_radius_*_allow) -- ra.a.allow_bits / allow_count
// set (hipErrorInvalidValue otherwise) and ra.a.R the radii over the allowed rows
hipError_t launch_knn_radius_f16(int metric, const KnnRadiusArgs &ra, uint32_t nblocks, bool fill, hipStream_t st,
                                 bool mask = false);
// every sorted query position of [a.p_base, a.p_end), the queries without a cluster included (no hits)
hipError_t launch_knn_radius_exact(int metric, const KnnRadiusArgs &ra, bool strict_h2, bool fill, hipStream_t st,
                                   bool mask = false);
// the queries of [a.p_base, a.p_end) the f16 kernel's block plan leaves out (no cluster): count 0 / an empty range
hipError_t launch_knn_radius_rest(const KnnRadiusArgs &ra, bool fill, hipStream_t st);
// *flag |= 1 if offsets[0 .. n] (device) decreases somewhere
hipError_t launch_knn_radius_offsets_check(const uint64_t *offsets, uint32_t n, uint32_t *flag, hipStream_t st);

// fp16x2 boundary conversions (seeding.hip)
hipError_t launch_half_to_float(const void *src, size_t n, float *dst, hipStream_t st);
hipError_t launch_float_to_half(const float *src, size_t n, void *dst, hipStream_t st);
hipError_t launch_quantize_half(float *v, size_t n, hipStream_t st);

// half2_strict.hip -- the reference's half2 arithmetic (fp_abstraction.h:100-182) kernel by kernel; plain
// thread-per-item kernels on fp32 words holding halves (KMCUDA_AMD_FP16_STRICT=1: verification mode)
hipError_t launch_h2_csqr(int metric, const float *centroids, uint32_t K, uint32_t D, float *sq2, hipStream_t st);
hipError_t launch_h2_assign(int metric, const float *samples, uint32_t N, uint32_t D, const float *centroids, uint32_t K,
                            const float *sq2, uint32_t *assignments, uint32_t *assignments_prev, uint32_t *counters,
                            hipStream_t st);
hipError_t launch_h2_adjust(int metric, const float *samples, uint32_t N, uint32_t D, uint32_t K, const uint32_t *prev,
                            const uint32_t *cur, float *centroids, uint32_t *ccounts, hipStream_t st);
hipError_t launch_h2_to_row(int metric, const float *samples, uint32_t N, uint32_t D, const float *row, uint32_t cc,
                            int mode /* 0 k-means++ step, 1 squared distance */, float *dists, hipStream_t st);
hipError_t launch_h2_member(int metric, const float *samples, uint32_t N, uint32_t D, const float *centroids,
                            const uint32_t *assignments, uint32_t K, float *dists, hipStream_t st);
hipError_t launch_h2_afk_min_dist(int metric, uint32_t m, uint32_t k, const float *samples, uint32_t D,
                                  const uint32_t *choices, const float *centroids, float *min_dists, hipStream_t st);
hipError_t launch_h2_yy_init(int metric, const float *samples, uint32_t len, uint32_t D, uint32_t K, uint32_t G,
                             const float *centroids, const uint32_t *assignments, const uint32_t *groups, float *bounds,
                             hipStream_t st);
hipError_t launch_h2_yy_drifts(int metric, const float *centroids, uint32_t K, uint32_t D, float *drifts, hipStream_t st);
hipError_t launch_h2_yy_global(int metric, const float *samples, uint32_t len, uint32_t D, uint32_t K, uint32_t G,
                               const float *centroids, const float *drifts, const float *gdrifts,
                               const uint32_t *assignments, uint32_t *assignments_prev, float *bounds, uint32_t *passed,
                               uint32_t *counters, hipStream_t st);
hipError_t launch_h2_yy_local(int metric, const float *samples, uint32_t len, uint32_t D, uint32_t K, uint32_t G,
                              const uint32_t *passed, const float *centroids, const uint32_t *groups, const float *drifts,
                              const float *gdrifts, uint32_t *assignments, float *bounds, uint32_t *counters,
                              hipStream_t st);

// transpose.hip (reference: transpose.cu:16-54)
hipError_t launch_transpose(const float *in, uint32_t rows, uint32_t cols, float *out, hipStream_t st);

}  // namespace kmx
