/*
 * kmcuda_amd.h -- step-level C ABI of the MI355X engine behind kmeans_cuda()/knn_cuda().
 *
 * The reference keeps these steps private (src/private.h:304-404: kmeans_cuda_setup,
 * kmeans_cuda_lloyd, kmeans_cuda_yy, knn_cuda_calc, cuda_transpose ...) and drives all GPUs
 * from one process with peer copies.  Row-sharded, one-process-per-GPU operation (RCCL
 * all-reduce of the per-iteration centroid deltas between kmamd_move_deltas and
 * kmamd_apply_delta) needs them exported.  Plain pointers and sizes only; every pointer
 * argument is a DEVICE pointer on the engine's GPU unless it says "host".
 * All calls return a KMCUDAResult code (kmcuda.h) and enqueue on the engine's stream.
 */
#ifndef KMCUDA_AMD_H
#define KMCUDA_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kmamd_engine kmamd_engine;

/* Creates the per-GPU workspace for n_rows local rows (reference: the allocations of
 * kmcuda.cc:423-470 + kmeans_cuda_setup kmeans.cu:750-772).  hip_stream: the stream every step is
 * enqueued on -- pass the framework's current stream to order with its work.  NULL: the engine
 * creates its own non-blocking stream (nothing else may touch its buffers without
 * kmamd_engine_sync).  (hipStream_t)-1: the caller works on the legacy default stream (handle 0,
 * torch's default): the engine creates an own BLOCKING stream, which the default stream orders
 * with implicitly in both directions. */
int kmamd_engine_create(kmamd_engine **out, int device, uint32_t n_rows, uint32_t features,
                        uint32_t clusters, int metric, int fp16x2, void *hip_stream);
void kmamd_engine_destroy(kmamd_engine *e);
void *kmamd_engine_stream(kmamd_engine *e);
int kmamd_engine_sync(kmamd_engine *e);

/* One assignment pass over the local rows (reference: kmeans_assign_lloyd, kmeans.cu:293-364,
 * incl. assignments_prev bookkeeping and the changed counter).  Bit-identical assignments. */
int kmamd_lloyd_assign(kmamd_engine *e, const float *samples, const float *centroids,
                       uint32_t *assignments, uint32_t *assignments_prev);
/* Same pass, reference arithmetic only (no matrix-core filter): the in-library cross-check. */
int kmamd_lloyd_assign_exact(kmamd_engine *e, const float *samples, const float *centroids,
                             uint32_t *assignments, uint32_t *assignments_prev);

/* Which matrix-core scheme the assignment filter runs: 0 = two-stage f16 MFMA (default): a coarse
 * pass with the high halves of the centred operands decides most rows, a contender pass in fp32 the
 * rest; 1 = f32 MFMA (cross-check).  Assignments are bit-identical in both (every stage carries a
 * rigorous bound and the exact kernels decide what is left); env KMCUDA_AMD_FILTER=f32 selects 1 at
 * engine creation. */
int kmamd_set_filter(kmamd_engine *e, int mode);

/* fp16x2 path: the engine's local rows as IEEE halves (n_rows x features halves, row-major, kept
 * alive by the caller).  When set, the f16 matrix-core filter of kmamd_lloyd_assign reads these rows
 * (half the HBM bytes) instead of the fp32 ones; `samples` must still point to the
 * same values widened to fp32 (the exact refine kernels read them).  Assignments are unchanged:
 * bit-identical to the fp32 path on the widened values.  NULL switches back. */
int kmamd_set_half_rows(kmamd_engine *e, const void *rows16);

/* Row cache of the two-stage filter's coarse pass.  on != 0: the caller promises that the rows given
 * to kmamd_lloyd_assign (samples, or the half rows) are the SAME, UNMODIFIED buffer on every call
 * from now on -- what the reference guarantees inside one kmeans_cuda() run, where the samples are
 * transposed once and iterated over (kmcuda.cc:505-508).  The next kmamd_lloyd_assign then stores
 * x - mu (mu = mean of that call's centroids, frozen from then on) as halves in the matrix-core
 * operand order (2 * features bytes per row + 8) and later passes stream that copy: half the HBM
 * bytes, whole 1-KB bursts, no conversion.  Assignments are unchanged (the bound is computed for the
 * mu in use).  Calling it again (on or off) drops the copy; off (the default) converts from the rows
 * on every pass.  If the copy cannot be allocated the engine silently stays uncached.
 * Env KMCUDA_AMD_ROW_CACHE=0 vetoes it (A/B runs). */
int kmamd_set_row_cache(kmamd_engine *e, int on);

/* counters: [0] reassigned rows since the last reset (d_changed_number, kmeans.cu:31),
 * [1] rows the filter handed to the full exact scan, [2] Yinyang passed rows (d_passed_number),
 * [3] rows the filter narrowed to two contenders (pair refine).  read = sync + copy to a host array; reset zeroes [0..3] (or one of them). */
int kmamd_counters_read(kmamd_engine *e, uint32_t *host_out4);
int kmamd_counters_reset(kmamd_engine *e, int which /* -1: all */);
/* Yinyang local filter with the second-best estimate (yinyang_hint.hip; KMCUDA_AMD_YY_HINT=0 turns it
 * off): running totals since the engine was created -- [0] rows it processed, [1] rows it handed to the
 * plain kernel (results are the reference's either way; the ratio is a performance figure), [2..5] the
 * hand-overs by first reason: no estimate, a skipped candidate whose bound does not hold, an evaluated
 * candidate whose bound exceeds the estimate, a final second minimum above the estimate. */
int kmamd_yy_hint_stats(kmamd_engine *e, uint32_t *host_out6);

/* Centroid update, split for the all-reduce (reference: kmeans_adjust, kmeans.cu:366-429):
 * move_deltas: delta[K*D] (fp64) = sum(moved-in rows) - sum(moved-out rows), dcount[K];
 * apply_delta: centroids = normalize(centroids*ccounts + delta), ccounts += dcount. */
int kmamd_move_deltas(kmamd_engine *e, const float *samples, const uint32_t *assignments_prev,
                      const uint32_t *assignments, double *delta, int32_t *dcount);
int kmamd_apply_delta(kmamd_engine *e, const double *delta, const int32_t *dcount,
                      float *centroids, uint32_t *ccounts);
/* The same two steps around ONE collective: buf is kmamd_reduce_len(e) = K*D + K + 4 doubles
 * (K + 1 more while sample weights are set: kmamd_set_weights),
 *   [ delta (K*D) | dcount (K) | counters 0..3 ]
 * (counts and counters are exact in fp64), written by reduce_fill with no separate pack step, summed
 * over the row shards by the caller (one all-reduce per iteration, the exchange of SURVEY 8e), and
 * consumed by reduce_apply; buf[K*D + K] then holds the GLOBAL number of reassigned rows.  In steady
 * state reduce_fill enqueues without any host read (update.hip: launch_move_deltas). */
size_t kmamd_reduce_len(kmamd_engine *e);
int kmamd_reduce_fill(kmamd_engine *e, const float *samples, const uint32_t *assignments_prev,
                      const uint32_t *assignments, double *buf);
int kmamd_reduce_apply(kmamd_engine *e, const double *buf, float *centroids, uint32_t *ccounts);
/* reduce_apply with the reference's stop rule (check_changed, kmeans.cu:697-717: evaluated BEFORE the update)
 * decided ON THE DEVICE, so that the caller can enqueue the next pass without waiting for the count:
 *   stop_threshold  tolerance * N as a float; the update happens only if (float)buf[K*D + K] (the reduced number
 *                   of reassigned rows) exceeds it, and then counters[0] is zeroed for the next pass.  Otherwise
 *                   NOTHING is modified and the engine's stop flag is raised: from then on kmamd_lloyd_assign
 *                   returns without touching anything (a pass enqueued speculatively leaves the state as the
 *                   reference returns it) until kmamd_stop_clear.  < 0: no test.
 *   seq             the caller's pass number.  The kernel reports to pinned words of the engine (two slots,
 *                   seq & 1); kmamd_stop_report(seq) waits for THIS call only (an event behind it on the engine's
 *                   stream; nothing has to wait in front of the next pass) and returns [0..3] the reduced
 *                   counters, [4] 1 if it stopped, [5] seq.  Reading a pass after the one after next has been
 *                   enqueued is an error (its slot has been reused). */
int kmamd_reduce_apply_stop(kmamd_engine *e, const double *buf, float *centroids, uint32_t *ccounts,
                            float stop_threshold, uint32_t seq);
int kmamd_stop_report(kmamd_engine *e, uint32_t seq, uint32_t *host_out6);
/* kmamd_reduce_apply_stop with the NEXT kmamd_lloyd_assign's centroid preparation fused into the same launch
 * (L2 metric, two-stage filter with the row cache in its steady state; in any other state it IS
 * kmamd_reduce_apply_stop).  Contract: the caller does not modify `centroids` between this call and that
 * kmamd_lloyd_assign, which recognises the buffer by its address. */
int kmamd_reduce_apply_prepare(kmamd_engine *e, const double *buf, float *centroids, uint32_t *ccounts,
                               float stop_threshold, uint32_t seq);
int kmamd_stop_clear(kmamd_engine *e);

/* Per-row sample weights: a row of weight w counts as w copies of the row in the centroid update and the stop rule
 * (the assignment passes do not depend on them).  weights: n_rows float32 on the engine's GPU, every one finite and
 * > 0 (anything else: InvalidArguments, the engine stays unweighted), kept alive and unmodified by the caller; NULL
 * switches back.  The call checks the weights (one stream synchronisation) and ZEROES the engine's running cluster
 * weights: call it before the first update of a run, with ccounts zeroed as for any run.
 * While weights are set:
 *   - kmamd_move_deltas / kmamd_reduce_fill form delta = sum(w x of the rows that moved in) - sum(w x moved out) in
 *     fp64; dcount and ccounts stay the integer member counts;
 *   - kmamd_reduce_len grows by K + 1 doubles,
 *       [ delta (K*D) | dcount (K) | counters 0..3 | dweight (K) | changed_weight ]
 *     dweight[c] = weight moved into c - weight moved out, changed_weight = the weight of the rows that joined a
 *     cluster in this pass; both are fp64 sums in an order fixed by the move lists (no floating-point atomics), so
 *     a call repeated gives the same bits.  Still ONE all-reduce per iteration.  With the split calls
 *     (kmamd_move_deltas, kmamd_apply_delta) the K + 1 words stay inside the engine between the two;
 *   - kmamd_apply_delta / kmamd_reduce_apply* compute (c * W_old + delta) / W_new (angular: normalised) with the
 *     cluster weights W the ENGINE keeps in fp64 (W_new = W_old + dweight[c]; a cluster whose COUNT is 0 is empty,
 *     gets NaN centroids and weight exactly 0 -- the weight itself is never asked);
 *   - stop_threshold of kmamd_reduce_apply_stop / _prepare is tolerance * (total weight over all shards) as a float
 *     and is compared with (float)changed_weight; the reported counters stay row counts.  kmamd_reduce_apply_prepare
 *     updates in a launch of its own (the next kmamd_lloyd_assign prepares its centroids itself).
 * kmamd_adjust_exact has no weighted form and ignores the weights. */
int kmamd_set_weights(kmamd_engine *e, const float *weights);
/* The caller has written `centroids` itself (new seeds, an imported set, a rounding pass) since the engine last
 * saw them: whatever kmamd_reduce_apply_prepare prepared for that buffer is void.  (The engine recognises the
 * buffer by its ADDRESS only; without this call the next kmamd_lloyd_assign would filter against the panels of
 * the old values.) */
int kmamd_centroids_written(kmamd_engine *e);
/* Bounds carried from pass to pass (the Yinyang phase of kmeans_cuda()'s default schedule; lloyd_carry.hip).  on != 0:
 * from the next kmamd_lloyd_assign on, a pass in the two-stage filter's steady state (row cache valid) leaves per
 * row an upper bound of the distance to its centroid and a lower bound of the distance to every other centroid --
 * read off the coarse stage's best two scores, no extra distance work --, the next preparation measures how far every
 * centroid has moved, and the next pass only looks at the rows whose bounds, moved by those drifts, no longer certify
 * the assignment (Hamerly's test with the rounding of the reference's arithmetic as margin; angular metric: one number
 * per row, the certified gap of the scores).  Assignments, previous
 * assignments and counters are exactly those of plain passes.  Contract: between two passes the centroids change only
 * through kmamd_reduce_apply* / kmamd_apply_delta or are announced with kmamd_centroids_written (which voids the
 * bounds), and `assignments` / `assignments_prev` are the buffers of the previous pass, untouched.
 * kmamd_carry_stats: rows_spared = row passes the bounds have decided since the engine was created (one stream
 * synchronisation), last_list = the length of the newest list the host has heard of (0xFFFFFFFF: none yet). */
int kmamd_set_carry(kmamd_engine *e, int on);
int kmamd_carry_stats(kmamd_engine *e, uint64_t *rows_spared, uint32_t *last_list);
/* A row that stage 2 settles between two contenders carries the pair, an upper bound of both distances and a lower
 * bound of every other centroid's (angular: the gap by which both scores exceed every other centroid's); while the
 * drifts leave the latter above the former (the gap positive) the row goes straight to the
 * two-contender kernel (the reference's arithmetic and tie rule: kmeans.cu:214-364 restricted to the two) instead of
 * through the filter.  rows_paired = such row passes since the engine was created (they are not in rows_spared).
 * KMCUDA_AMD_CARRY_PAIRS=0 in the environment: without (A/B). */
int kmamd_carry_pair_stats(kmamd_engine *e, uint64_t *rows_paired);
/* The default Lloyd filter's duo list (csrc/lloyd_duo.hip; the reference has no counterpart, its kmeans_assign_lloyd
 * -- kmeans.cu:293-364 -- scans every centroid for every row): rows of the LAST assignment pass that stage 1 could
 * not decide but whose two contenders it knew by index, so that stage 2 settled them without sweeping the centroids
 * again.  The engine uses the list where it pays (lists beyond one round of stage-2 blocks); KMCUDA_AMD_DUO=0 / 2 in
 * the environment: never / always. */
int kmamd_duo_rows(kmamd_engine *e, uint32_t *rows);
/* The host side of the carried bounds replayed without a device (tests): pass i + 1 would count list_len[i] rows if it
 * counts a list, a pass's report reaches the host `lag` >= 1 passes later; out[i] = 0 plain pass (the bounds are paused),
 * 1 whole pass that leaves bounds but has none to move, 2 whole pass that counts its would-be list, 3 listed pass.
 * changed (may be null): the passes' reassignment counts, which the host judges `lag` passes late too -- a run that
 * converges slowly (counts falling by less than a third per pass) answers two hopeless lists with one long pause. */
int kmamd_carry_policy_sim(uint32_t n_passes, uint32_t n_rows, float list_max, const uint32_t *list_len, uint32_t lag,
                           uint8_t *out, const uint32_t *changed);
/* Test / A-B hook for the update's host logic: 0 default, 1 radix path always, 2 always read the
 * counts before choosing (the pre-round-2 behaviour), 3 bucket path always without reading (exercises
 * the device-side fallback of oversized buckets).  Env KMCUDA_AMD_UPDATE=radix|sync|bucket sets it at
 * engine creation.  Sums are bit-identical on every path. */
int kmamd_set_update_mode(kmamd_engine *e, int mode);

/* Strict-parity centroid update: kmeans_adjust (kmeans.cu:366-429) operation for operation --
 * one serial fp32 Kahan chain per centroid over its move events in ascending row order with the
 * reference's single shared compensation term, then normalize.  Centroids and ccounts are
 * bit-identical to the reference's.  Needs ALL rows on this engine (the chain order is global),
 * so it is the single-GPU verification mode (kmeans_cuda: env KMCUDA_AMD_EXACT_UPDATE=1). */
int kmamd_adjust_exact(kmamd_engine *e, const float *samples, const uint32_t *assignments_prev,
                       const uint32_t *assignments, float *centroids, uint32_t *ccounts);

/* Yinyang steps (reference: kmeans.cu:431-672), all on the engine's n_rows local rows.
 *   groups   K host uint32: centroid -> group, >= G for a NaN centroid (kmamd_yy_configure uploads it
 *            and builds the group-sorted panel index)
 *   bounds   (G+1) x n_rows group-major: [0] upper bound, [1+g] lower bound to group g
 *   drifts   K*D old centroids followed by K per-centroid drifts; gdrifts: G per-group maxima
 * yy_init: kmeans_yy_init (:431-485).  yy_drifts: kmeans_yy_calc_drifts + _find_group_max_drifts
 * (:487-538).  yy_filters: kmeans_yy_global_filter then _local_filter (:540-672); counters[2]
 * (passed) must be reset by the caller, counters[0] accumulates reassignments.
 * yy_init and the local filter run the matrix-core filter in front of the exact arithmetic
 * (env KMCUDA_AMD_YY_EXACT=1 at configure time: plain exact kernels); either way bounds, drifts
 * and assignments are bit-identical to the reference arithmetic. */
int kmamd_yy_configure(kmamd_engine *e, uint32_t G, const uint32_t *groups_host);
int kmamd_yy_init(kmamd_engine *e, const float *samples, const float *centroids, const uint32_t *assignments,
                  float *bounds);
int kmamd_yy_drifts(kmamd_engine *e, const float *centroids, float *drifts, float *gdrifts);
int kmamd_yy_filters(kmamd_engine *e, const float *samples, const float *centroids, const float *drifts,
                     const float *gdrifts, uint32_t *assignments, uint32_t *assignments_prev, float *bounds,
                     uint32_t *passed);

/* AFK-MC2's random numbers (reference: kmeans_afkmc2_random_step, kmeans.cu:107-116: curand_init(seed, thread, step)):
 * out[t * n + i] = draw i of the XORWOW stream (seed, subsequence t, offset), t < threads, as the seeding kernels
 * generate them -- cuRAND's seed scrambling in front of the generator cuRAND and rocRAND share (csrc/seeding.hip).
 * A window for tests: the draws must equal the oracle's restatement (tests/test_gpu_afkmc2_rng.py). */
int kmamd_afkmc2_draws(kmamd_engine *e, uint64_t seed, uint64_t offset, uint32_t threads, uint32_t n, uint32_t *out);

/* out[c][r] = in[r][c], 4-byte elements (reference: cuda_transpose, transpose.cu:83-117). */
int kmamd_transpose(kmamd_engine *e, const float *in, uint32_t rows, uint32_t cols, float *out);

/* Which filter kmamd_lloyd_assign runs in front of the exact kernels for this engine's shape: 1 the register-resident
 * ones (features <= 256: lloyd.hip / lloyd_f16.hip), 2 the LDS-streamed one (features > 256: lloyd_wide.hip), 0 none
 * (the exact kernels alone: the streamed filter switched off or out of memory).  *padded_width: the feature count the
 * filter's operands are padded to (0 with no filter).  Both kinds carry bounds (kmamd_set_carry; kind 2 up to 4096
 * features and without pair certificates). */
int kmamd_filter_kind(kmamd_engine *e, uint32_t *padded_width);

/* Timing of the dominant kernel on the engine's own stream (HIP events): start/stop bracket
 * the next lloyd filter launches; elapsed returns the summed milliseconds and launch count. */
int kmamd_profile_reset(kmamd_engine *e);
int kmamd_profile_read(kmamd_engine *e, double *filter_ms, uint32_t *filter_launches,
                       double *exact_ms, double *update_ms);
/* stage 1 of the two-stage filter on its own (HIP events around that one launch, inside the filter span) */
int kmamd_profile_read_coarse(kmamd_engine *e, double *coarse_ms);
int kmamd_profile_enable(kmamd_engine *e, int on);

/* What the last kmeans_cuda() call of this process did: iterations of its Lloyd / Yinyang loops, the
 * wall-clock seconds spent in them (after upload + seeding, before the outputs are gathered), the
 * seconds before (upload, seeding), the number of row shards and of RCCL ranks (0: single GPU or the
 * one-device test hook).  Lets a driver time the drop-in entry point itself (bench.py --api). */
int kmamd_last_run_stats(uint32_t *iterations, double *loop_seconds, double *setup_seconds, uint32_t *shards,
                         uint32_t *rccl_ranks);

/* kmeans_cuda() (kmcuda.h: same arguments, same meaning, same result codes; init / metric are the KMCUDAInitMethod /
 * KMCUDADistanceMetric values) with per-row sample weights: sample_weights = samples_size float32, a host pointer
 * when device_ptrs < 0, else a pointer on device `device_ptrs` like `samples` (always float32, also when the rows are
 * fp16x2).  NULL: exactly kmeans_cuda() -- which is this call with NULL.  A row of weight w counts as w copies:
 * centroids are sum(w x) / sum(w) of their members (angular: the normalised weighted sum), the run stops when the
 * reassigned weight is at most tolerance * the total weight (Yinyang's 11 % hand-over point likewise),
 * *average_distance is sum(w d) / sum(w), and k-means++ draws every seed after the first (uniform, as the reference)
 * with probability proportional to w * its distance term.  init = random / imported centroids ignore the weights.
 * InvalidArguments, before any clustering work and with the outputs untouched: a weight that is not finite and > 0;
 * weights with init = afkmc2, with KMCUDA_AMD_EXACT_UPDATE=1 or with KMCUDA_AMD_FP16_STRICT=1 on fp16x2 rows (those
 * restate the reference's own arithmetic, which has no weights).  KMCUDA_AMD_YY=reference works with weights: it
 * shares the default update. */
int kmamd_kmeans_weighted(int init, const void *init_params, float tolerance, float yinyang_t, int metric,
                          uint32_t samples_size, uint16_t features_size, uint32_t clusters_size, uint32_t seed,
                          uint32_t device, int32_t device_ptrs, int32_t fp16x2, int32_t verbosity, const float *samples,
                          float *centroids, uint32_t *assignments, float *average_distance,
                          const float *sample_weights);

/* With KMCUDA_AMD_TIME_COLLECTIVE=1 in the environment of that call (several row shards): the summed duration of its
 * per-iteration all-reduces -- ncclAllReduce over the device mask, or the one-device stand-in under
 * KMCUDA_AMD_VIRTUAL_SHARDS -- as HIP events on the first shard's stream bracketed them (the wait for the slowest
 * shard's move sums is inside: that is what an iteration pays), and their number.  0 / 0 otherwise. */
int kmamd_last_run_collective(double *milliseconds, uint32_t *count);

/* k nearest neighbours of NEW rows (queries) among a clustered corpus (no counterpart in the reference, whose knn_cuda
 * -- kmcuda.h, kmcuda.cc:572-730 -- is the self-join of the corpus).  An index owns one GPU's prepared corpus: the
 * cluster-sorted fp32 copy, its f16 split, the radii, the K x K centroid distances, mu and the stats, built once as
 * knn_cuda() builds them and reused by every query.
 *   create   samples n_rows x features, centroids clusters x features (fp32, or IEEE halves when fp16x2 != 0 --
 *            `features` counts halves then and must be even; fp32 arithmetic on the half values as knn_cuda()),
 *            assignments n_rows (>= clusters: the row has no cluster and is never returned).  device_ptrs: -1 host
 *            buffers, else the index's device.  The index keeps copies: the caller's buffers may change afterwards.
 *   query    k in [1, min(n_rows, 65535)]; n_queries x features rows in the corpus's dtype.  query_assignments
 *            (optional, in): each query's cluster c_q in [0, clusters) with a finite centroid (else InvalidArguments); NULL: its nearest
 *            centroid in kmamd_lloyd_assign's arithmetic and tie rule, written to query_assignments_out if that is
 *            given (the passed-in ones otherwise).  Outputs n_queries x k: neighbors (corpus row indices), distances
 *            (optional, float32: the exact distance the heap compared -- L2 distance or the angular metric's acos
 *            value).  A query's list is the reference's procedure for it as one more row of cluster c_q WITHOUT the
 *            self-skip: own cluster in ascending corpus order, then the others in ascending id under the triangle
 *            prune, push iff distance <= kth, output in the heap's sorted order.  Any c_q gives the same lists (the
 *            prune is rigorous); only the speed changes.  A query with a NaN or inf feature: indices 0xFFFFFFFF,
 *            distances NaN.  device_ptrs: -1 host buffers, else the index's device (all of the call's buffers).
 *            Synchronous: the outputs are complete on return.  Env KMCUDA_AMD_KNN_QUERY_CHUNK=<n> (tests): at most n
 *            queries per chunk (default: lb and heaps of a chunk within 4 GiB).
 * KMCUDA_AMD_KNN_EXACT, KMCUDA_AMD_FILTER=f32 and KMCUDA_AMD_FP16_STRICT select the search as for knn_cuda(). */
typedef struct kmamd_knn_index kmamd_knn_index;
int kmamd_knn_index_create(kmamd_knn_index **out, int device, int metric, int fp16x2, uint32_t n_rows,
                           uint32_t features, uint32_t clusters, const void *samples, const void *centroids,
                           const uint32_t *assignments, int32_t device_ptrs, int verbosity);
int kmamd_knn_index_query(kmamd_knn_index *ix, uint32_t k, uint32_t n_queries, const void *queries,
                          const uint32_t *query_assignments, uint32_t *neighbors, float *distances,
                          uint32_t *query_assignments_out, int32_t device_ptrs);
void kmamd_knn_index_destroy(kmamd_knn_index *ix);

/* Multi-probe (approximate) search on the same index: every query looks only at the clusters of its
 * probe list P(q), nprobe ids wide, 1 <= nprobe <= min(clusters, 64).  The result is a defined object, not "roughly the
 * neighbours": the list of kmamd_knn_index_query with one more skip rule -- a cluster outside the effective probe set
 * is never visited.  Own cluster c_q = P(q)[0] first, in ascending corpus order; then the other probed clusters in
 * ascending id under the same triangle prune; push iff distance <= kth; output in the heap's sorted order with the
 * exact distances the heap compared.  The effective probe set is the distinct entries of P(q) below `clusters`:
 * entries equal to `clusters` (kmamd_kmeans_assign_top's filler) and repeated entries are ignored, and the order after
 * column 0 does not matter.  Slots no probed row fills hold index 0 at FLT_MAX, as in query.  With nprobe = clusters
 * the lists are those of query with query_assignments = column 0.
 *   probes      (optional, in) n_queries x nprobe.  Column 0 must be < clusters and name a finite centroid, later
 *               columns may hold any id <= clusters; anything else is InvalidArguments.  NULL: the lists are
 *               kmamd_kmeans_assign_top(queries, centroids, nprobe)'s top_assignments, by the same kernels (clusters
 *               == 1: {0}); a query it finds no centroid for has no cluster.  KMCUDA_AMD_ASSIGN_TOP and
 *               KMCUDA_AMD_ASSIGN_TOP_ROWS apply.  With KMCUDA_AMD_FP16_STRICT and half rows the ranking is refused
 *               (InvalidArguments), the caller's lists work.
 *   probes_out  (optional) n_queries x nprobe: the lists used, in query order.
 * A query with a NaN or inf feature: indices 0xFFFFFFFF, distances NaN.  k, neighbors, distances, device_ptrs,
 * KMCUDA_AMD_KNN_QUERY_CHUNK (default: a chunk's heaps and lists within 4 GiB) as in query; n_queries == 0 is success.
 * The f16-filtered search runs where query's would; every other case (KMCUDA_AMD_KNN_EXACT, KMCUDA_AMD_FP16_STRICT,
 * KMCUDA_AMD_FILTER=f32, more than 1024 features, data beyond the half range, more than 65536 clusters) takes the
 * exact probe kernel -- there is no f32-filtered one.  The per-query centroid bounds (KMCUDA_AMD_KNN_TIGHT) are not
 * used.  KMCUDA_AMD_KNN_STATS prints the search's counters at the end of the call. */
int kmamd_knn_index_query_probe(kmamd_knn_index *ix, uint32_t k, uint32_t nprobe, uint32_t n_queries,
                                const void *queries, const uint32_t *probes /* optional, n_queries x nprobe */,
                                uint32_t *neighbors, float *distances /* optional */,
                                uint32_t *probes_out /* optional, n_queries x nprobe */, int32_t device_ptrs);

/* Radius search on the same index: the hits of a query are the corpus rows that have a cluster
 * (assignment < clusters) and whose distance to it is <= radius -- the exact distance kmamd_knn_index_query returns and
 * compares (L2 distance / the angular metric's acos value; a NaN distance is no hit; a query with a NaN or inf feature
 * has none).  The result is the brute-force set over the clustered rows, in ascending (cluster id, corpus row index)
 * order, whatever query_assignments say (they only group the queries and feed the cluster prune) and however the batch
 * is chunked.  radius: float32, finite, >= 0 (else InvalidArguments).  Two stateless, synchronous calls; the caller
 * owns all memory and the search runs once in each:
 *   count    counts[q] = number of hits (n_queries).  query_assignments / query_assignments_out as in query.
 *   fill     offsets: n_queries + 1 non-decreasing positions (the exclusive prefix sum of the counts); query q's hits
 *            go to [offsets[q], offsets[q + 1]) of neighbors (corpus row indices) and distances (optional).
 *            InvalidArguments before anything is written if offsets decreases somewhere; InvalidArguments after the
 *            search if a query's hit count differs from its range -- nothing has been written outside the ranges.
 * Buffers and device_ptrs as in query (-1: host; else the index's device, all of the call's buffers).  n_queries == 0
 * is success.  KMCUDA_AMD_KNN_QUERY_CHUNK applies (default: a chunk's centroid bounds within 4 GiB; with host buffers a
 * chunk's range of hits is staged on the device within 4 GiB more).  KMCUDA_AMD_KNN_EXACT, KMCUDA_AMD_FP16_STRICT and
 * KMCUDA_AMD_FILTER=f32 take the exact radius kernel (there is no f32-filtered one); KMCUDA_AMD_KNN_TIGHT does not
 * apply (the per-query centroid bounds are the prune test); KMCUDA_AMD_KNN_STATS prints the search's counters. */
int kmamd_knn_index_radius_count(kmamd_knn_index *ix, float radius, uint32_t n_queries, const void *queries,
                                 const uint32_t *query_assignments, uint32_t *counts,
                                 uint32_t *query_assignments_out, int32_t device_ptrs);
int kmamd_knn_index_radius_fill(kmamd_knn_index *ix, float radius, uint32_t n_queries, const void *queries,
                                const uint32_t *query_assignments, const uint64_t *offsets /* n_queries + 1 */,
                                uint32_t *neighbors, float *distances /* optional */, int32_t device_ptrs);

/* More rows for an index, in place.  After add the index is observably the index that
 * kmamd_knn_index_create builds from the concatenation of its rows so far and the new ones, with the same centroids:
 * the new rows get the ids n_rows_so_far, n_rows_so_far + 1, ... in the order given, and query, query_probe and both
 * radius calls return what they return on that fresh index, bit for bit in indices and distances, on every search path
 * (nothing the searches read depends on how the corpus arrived).
 *   rows             n_rows x features in the index's dtype (fp32, or halves for an fp16x2 index)
 *   assignments      (optional, in) n_rows cluster ids by create's rule: an id >= clusters means "no cluster" -- the row
 *                    is never returned, but it takes an id and counts in n_rows.  NULL: the rows' clusters are
 *                    kmamd_kmeans_assign(rows, the index's centroids)'s assignments (the engine's filtered bit-exact
 *                    pass, as a query chunk runs it; `clusters` for a row that pass gives no cluster), written to
 *                    assignments_out if given.  So add(B) is exactly add(B, kmeans_predict(B, centroids)).
 *   assignments_out  (optional) n_rows: the clusters used
 *   first_row        (optional, host) the id of rows[0]
 *   device_ptrs      -1 host buffers, else the index's device (all of the call's buffers but first_row)
 * Synchronous.  n_rows == 0 succeeds and changes nothing.  NOT safe against a concurrent call on the same index.
 * InvalidArguments, before any device work and with the index untouched: a null handle, null rows with n_rows > 0,
 * device_ptrs naming another device, more than 0xFFFFFFFE rows in all (0xFFFFFFFF is the "no neighbour" marker), and
 * assignments == NULL where the index runs the half2 arithmetic (KMCUDA_AMD_FP16_STRICT has no assignment pass, as
 * query_probe refuses its ranking; a caller's assignments work there).  If an allocation fails the call returns
 * kmcudaMemoryAllocationFailure and the index is exactly what it was, still usable: the new sorted copies are built
 * beside the old ones (peak: both, about 2 x (6 DP + 24) bytes per row, DP the padded row width) and swapped in at the
 * end.  Afterwards k <= the new n_rows is accepted by the queries.  A centred new row outside the half range makes the
 * index leave the f16 filter for good, as create on the concatenation would (the f32 filter up to 256 features, the
 * exact search beyond); verbosity > 0 says so once.  Env KMCUDA_AMD_KNN_ADD_CHUNK=<rows> (tests): rows per chunk -- each
 * chunk is one merge -- (default: a chunk's staged and sorted copies within 4 GiB); the result does not depend on it.
 *   info   n_rows, n_clustered (the rows that have a cluster) and filter (2: the f16 matrix-core filter, 1: the f32
 *          one, 0: every candidate evaluated exactly); any of the three may be NULL. */
int kmamd_knn_index_add(kmamd_knn_index *ix, uint32_t n_rows, const void *rows,
                        const uint32_t *assignments /* optional in, n_rows */,
                        uint32_t *assignments_out /* optional, n_rows */,
                        uint32_t *first_row /* optional out, host: the id of rows[0] */, int32_t device_ptrs);
int kmamd_knn_index_info(kmamd_knn_index *ix, uint32_t *n_rows, uint32_t *n_clustered,
                         int *filter /* 2: f16, 1: f32, 0: exact; any may be NULL */);

/* Rows out of an index, in place.  After remove the index is observably the index that
 * kmamd_knn_index_create builds from the same rows and centroids with the assignments of the listed ids set to
 * `clusters` ("no cluster"): the rows are never returned again by query, query_probe or either radius call, and those
 * calls return what they return on that fresh index, bit for bit in indices and distances, on every search path.  Ids
 * are stable: n_rows does not change, every other row keeps its id, and a later add hands out n_rows, n_rows + 1, ...
 * as before.  n_clustered drops by the rows that lost a cluster; k up to n_rows stays valid (slots nothing fills hold
 * what the fresh index puts there).
 *   ids          n_ids row ids, each below n_rows, in any order.  An id whose row has no cluster (removed before, or
 *                given as >= clusters at create / add) is allowed and changes nothing; a repeated id counts once.
 *   n_removed    (optional, host) the rows that actually lost a cluster.  If that is 0 -- n_ids == 0 included -- the
 *                index's buffers are not touched at all.
 *   device_ptrs  -1: ids is a host buffer, else the index's device
 * Synchronous.  NOT safe against a concurrent call on the same index.  InvalidArguments, before any device work that
 * changes the index and with the index and *n_removed untouched: a null handle, null ids with n_ids > 0, device_ptrs
 * naming another device, an id >= n_rows.  If an allocation fails the call returns kmcudaMemoryAllocationFailure and
 * the index is exactly what it was, still usable: the new sorted copies are built beside the old ones (peak: both, and
 * about 7 words per row of scratch) and swapped in at the end.  The cost is that of one pass over the whole index,
 * whatever the length of the list.  Memory is NOT reclaimed: a removed row moves to the no-cluster tail of the sorted
 * copies, where a fresh index keeps such rows; there is no compaction and no reuse of ids.  The index never returns to
 * a filter it has left: one that left the f16 filter (a centred row outside the half range) stays where it is even if
 * that row is removed -- the results are the same bits either way, info's `filter` is the one difference from the
 * fresh index.  Env KMCUDA_AMD_KNN_REMOVE_TIME=1 prints the device time of the call's stages.
 *   radii   the clusters' radii as the searches' prune reads them (clusters floats, host; NaN: an empty cluster), after a
 *           wait for the index's stream.  A window for tests: a stale radius would only loosen the prune without
 *           changing any result, so nothing else shows it. */
int kmamd_knn_index_remove(kmamd_knn_index *ix, uint32_t n_ids, const uint32_t *ids,
                           uint32_t *n_removed /* optional out, host */, int32_t device_ptrs);
int kmamd_knn_index_radii(kmamd_knn_index *ix, float *radii /* host, clusters floats */);

/* Filtered search: a query batch over a SUBSET of the corpus, for one call, without touching the index (DESIGN.md
 * 4.17).  allow: one flag per corpus row id, n_rows bytes as the index counts them now (after any add / remove), on the
 * side device_ptrs names; a row is allowed iff its flag is non-zero; one mask serves the whole batch.  A masked call
 * returns, bit for bit in indices and distances, what the same call returns on the index kmamd_knn_index_create builds
 * from the same rows and centroids with the assignments of every non-allowed row set to `clusters` -- remove()'s
 * definition, for one call.  On every search path.  So:
 *   - the flag of a row that has no cluster is ignored;
 *   - with every flag set the call returns the bits of the unmasked call;
 *   - with no row allowed every finite query gets index 0 at FLT_MAX in all k slots (a query with a NaN or inf feature
 *     0xFFFFFFFF / NaN as ever);
 *   - k up to n_rows stays valid; slots no allowed row fills hold what the fresh index puts there (index 0, FLT_MAX);
 *   - computed query assignments and computed probe lists (query_assignments == NULL, probes == NULL) do not depend on
 *     the mask: they rank centroids, not rows;
 *   - the index is not modified.  If an allocation fails the call returns kmcudaMemoryAllocationFailure and the index
 *     is still usable.  The per-call scratch is n_rows / 8 bytes of bits, 8 bytes per row for the member distances the
 *     masked radii are reduced from and, for a host mask, its n_rows bytes staged on the device;
 *   - NOT safe against a concurrent call on the same index, as the other calls are not.
 * allow == NULL is exactly kmamd_knn_index_query / kmamd_knn_index_query_probe.  Every other argument, the refusals,
 * the chunking (KMCUDA_AMD_KNN_QUERY_CHUNK; the mask is prepared once per call and shared by its chunks) and
 * n_queries == 0 behave as in the call mirrored.  The cluster prunes -- the triangle test and the L2 per-query centroid
 * bounds -- read the radii over the ALLOWED rows, the radii of that fresh index; a cluster without an allowed row is
 * walked over like one without rows.  The f16-filtered search runs where the unmasked call's would; every other case
 * (KMCUDA_AMD_KNN_EXACT, KMCUDA_AMD_FP16_STRICT, KMCUDA_AMD_FILTER=f32, an index or a query chunk that has left the
 * f16 filter, more than 1024 features) takes the masked exact kernel: there is NO masked f32 filter.  The f16 filter
 * still scores every row of a visited cluster (the mask drops candidates where survivors are queued).  Radius search
 * through kmamd_knn_index_radius_count / _fill: that pair takes no mask; the masked radius search is
 * kmamd_knn_index_radius_count_allow / _fill_allow below.
 *   radii_allow   the radii a masked search with this mask prunes with (clusters floats, host; NaN: a cluster without
 *                 an allowed row).  A window for tests, as kmamd_knn_index_radii.  allow == NULL: the index's own. */
int kmamd_knn_index_query_allow(kmamd_knn_index *ix, uint32_t k, uint32_t n_queries, const void *queries,
                                const uint32_t *query_assignments, uint32_t *neighbors, float *distances,
                                uint32_t *query_assignments_out, int32_t device_ptrs,
                                const uint8_t *allow /* optional, n_rows bytes */);
int kmamd_knn_index_query_probe_allow(kmamd_knn_index *ix, uint32_t k, uint32_t nprobe, uint32_t n_queries,
                                      const void *queries, const uint32_t *probes /* optional, n_queries x nprobe */,
                                      uint32_t *neighbors, float *distances /* optional */,
                                      uint32_t *probes_out /* optional, n_queries x nprobe */, int32_t device_ptrs,
                                      const uint8_t *allow /* optional, n_rows bytes */);
int kmamd_knn_index_radii_allow(kmamd_knn_index *ix, const uint8_t *allow /* optional, n_rows bytes */,
                                int32_t device_ptrs /* where allow lies */, float *radii_host /* clusters floats */);

/* Masked radius search: kmamd_knn_index_radius_count / _fill over a SUBSET of the corpus, for one
 * call.  allow as in kmamd_knn_index_query_allow: one flag per corpus row id, n_rows bytes as the index counts them now,
 * on the side device_ptrs names.  A hit of query q under mask allow and radius r is a corpus row i with
 *     assignments[i] < clusters   and   allow[i] != 0   and   d(q, i) <= r,
 * d the exact distance kmamd_knn_index_query returns and compares; hits come in ascending (cluster id, row id) order.
 * That is what the unmasked radius call returns on the index kmamd_knn_index_create builds from the same rows and
 * centroids with every denied row's assignment set to `clusters`, and equally the unmasked result of THIS index with
 * the denied rows struck out -- a radius result is a brute-force set, so both are the same bits, on every search path
 * and under every chunking.  So:
 *   - the flag of a row that has no cluster is ignored;
 *   - with every flag set the calls return the bits of the unmasked calls;
 *   - with no row allowed every count is 0, and a fill whose offsets are all equal succeeds and writes nothing;
 *   - a query with a NaN or inf feature has no hits;
 *   - query_assignments still only group the queries and feed the cluster prune;
 *   - the index is not modified.  If an allocation fails the call returns kmcudaMemoryAllocationFailure and the index
 *     is still usable (the per-call scratch is that of kmamd_knn_index_query_allow);
 *   - NOT safe against a concurrent call on the same index;
 *   - the fill contract is unchanged: the offsets are checked before any write, and a query whose hit count differs
 *     from its range gives InvalidArguments after the search with nothing written outside the ranges -- which is what
 *     a count under one mask followed by a fill under another gets.  The count and the fill each prepare the mask: the
 *     two calls are stateless;
 *   - n_queries == 0 is success before the mask is looked at, and the unmasked call's refusals come first, in its order.
 * allow == NULL is exactly kmamd_knn_index_radius_count / _fill (which are these calls with NULL).  The cluster prunes
 * read the radii over the ALLOWED rows; a cluster without an allowed row is walked over like one without rows.  The
 * masked f16 kernel runs where the unmasked one would and does not score a 32-row sub-tile none of whose rows is
 * allowed; everything else (KMCUDA_AMD_KNN_EXACT, KMCUDA_AMD_FP16_STRICT -- which still prunes nothing --,
 * KMCUDA_AMD_FILTER=f32, more than 1024 features, an index or a chunk that has left the half range) takes the masked
 * exact kernel.  KMCUDA_AMD_KNN_STATS prints the same lines ("radius count" / "radius fill"). */
int kmamd_knn_index_radius_count_allow(kmamd_knn_index *ix, float radius, uint32_t n_queries, const void *queries,
                                       const uint32_t *query_assignments, uint32_t *counts,
                                       uint32_t *query_assignments_out, int32_t device_ptrs,
                                       const uint8_t *allow /* optional, n_rows bytes */);
int kmamd_knn_index_radius_fill_allow(kmamd_knn_index *ix, float radius, uint32_t n_queries, const void *queries,
                                      const uint32_t *query_assignments, const uint64_t *offsets,
                                      uint32_t *neighbors, float *distances /* optional */, int32_t device_ptrs,
                                      const uint8_t *allow /* optional, n_rows bytes */);

/* Capped search: the k nearest rows of every query, but only those within max_distance -- the hybrid
 * search (radius plus a limit on the count) in one pass.  max_distance = r is a float32 that is not NaN and >= 0 (else
 * InvalidArguments, before any device call); +inf is accepted and means FLT_MAX.  The list of a query is the list of
 * kmamd_knn_index_query (of _query_probe when probed, of the _allow forms when masked) with ONE change: wherever that
 * procedure reads kth, it reads min(kth, r).  So
 *   - a candidate is pushed iff distance <= min(kth, r) -- inclusive: a row at exactly r is returned;
 *   - a cluster is skipped iff C[c][c_q] - d(q, c_q) - R[c] > min(kth, r), and the f16 search's second test reads
 *     lb[c][q] > min(kth, r);
 *   - the heap is the same heap: k slots of (FLT_MAX, index 0) at the start, popped into the same sorted order.  The
 *     real entries of a row are those with distance <= r and they come first; a slot no row within r filled holds
 *     index 0 at FLT_MAX, as the filler tail of query does;
 *   - a query with a NaN or inf feature still gets 0xFFFFFFFF / NaN;
 *   - with r = FLT_MAX (or inf) the call returns the bits of the uncapped call, fillers included.
 * On data without distance ties this is query's list with every entry beyond r replaced by the filler; the procedure
 * above is the definition.  The cap is live from the first candidate: the filters' threshold and both cluster prunes
 * start at r instead of FLT_MAX, so a query with fewer than k rows within r no longer scans the corpus.  One cap per
 * call (no per-query array).  Every other argument, the refusals (a null handle among them), the chunking, allow (NULL:
 * no mask) and n_queries == 0 behave as in kmamd_knn_index_query_allow / kmamd_knn_index_query_probe_allow, which are
 * these calls at FLT_MAX; the same kernels run on the same paths.  KMCUDA_AMD_KNN_STATS: query_capped prints the
 * search's counters as "capped query" at the end of the call, query_probe_capped the "probe query" line. */
int kmamd_knn_index_query_capped(kmamd_knn_index *ix, uint32_t k, float max_distance, uint32_t n_queries,
    const void *queries, const uint32_t *query_assignments, uint32_t *neighbors, float *distances,
    uint32_t *query_assignments_out, int32_t device_ptrs, const uint8_t *allow /* optional */);

int kmamd_knn_index_query_probe_capped(kmamd_knn_index *ix, uint32_t k, float max_distance, uint32_t nprobe,
    uint32_t n_queries, const void *queries, const uint32_t *probes, uint32_t *neighbors, float *distances,
    uint32_t *probes_out, int32_t device_ptrs, const uint8_t *allow /* optional */);

/* Assigns rows to GIVEN centroids -- the "predict" of a trained K-means (no counterpart in the reference, whose
 * kmeans_cuda returns the assignments of the rows it was trained on only) -- with, as asked, the distance of every row
 * to its centroid and per-cluster statistics.  Stateless and synchronous; the caller owns all memory.
 *   metric, fp16x2     as kmeans_cuda: 0 L2 / 1 angular (rows expected at unit length, nothing is normalised); fp16x2 != 0:
 *                      rows and centroids are IEEE halves, features_size counts halves and must be even (as
 *                      kmamd_knn_index_create), fp32 arithmetic on the half values
 *   device             ONE device id, as for the k-NN index (not kmeans_cuda's mask)
 *   device_ptrs        -1: every buffer is on the host; else every buffer is on that device, which must be `device`
 *   assignments[s]     what ONE kmamd_lloyd_assign pass leaves when every assignment starts at clusters_size: the
 *                      nearest centroid in the reference's arithmetic (round-down-FMA Kahan dot, lloyd_distance), strict
 *                      `<` in ascending centroid order (the lowest index wins a tie, a NaN centroid never wins);
 *                      clusters_size -- "no cluster", what kmeans_cuda returns and the k-NN index accepts -- for a row
 *                      whose first feature is NaN or whose distances are all NaN
 *   distances[s]       optional: the reference's distance(row, centroid[assignments[s]]) (metric_abstraction.h:59-72 /
 *                      :179-191, the per-sample term of kmeans_calc_average_distance), NaN for a row without a cluster
 *                      (angular: the angle of the reference's Kahan product by the C library's acosf, restated on the
 *                      device operation for operation -- the CPU oracle's bits; kmeans_cuda / the k-NN index take the
 *                      device library's acosf, which can differ by one in the last place)
 *   cluster_counts[c]  optional: the number of rows assigned to c
 *   cluster_distance_sums[c]  optional: the fp64 sum of the float32 distances of the rows assigned to c (0.0 for an
 *                      empty cluster; the distances are computed in scratch if they are not asked for).  No
 *                      floating-point atomics: per chunk the members in ascending row order through a fixed reduction
 *                      tree, the chunks added in chunk order -- two identical calls give identical bits; another chunk
 *                      size may change the last places.
 * clusters_size >= 2.  samples_size == 0 is success (counts and sums zero).  InvalidArguments before any device work,
 * with the outputs untouched: bad sizes, null pointers, device_ptrs naming another device, and KMCUDA_AMD_FP16_STRICT=1
 * with fp16x2 rows (the reference's half2 arithmetic has no predict form).  The rows go through in chunks whose staged
 * fp32 copy stays within 4 GiB; env KMCUDA_AMD_ASSIGN_CHUNK=<rows> (tests) sets the chunk.  KMCUDA_AMD_FILTER=f32
 * applies as to any engine.  KMCUDA_AMD_ASSIGN_DIST=member: the distance pass on kmeans_cuda's per-thread kernel
 * (its instantiation with the acosf above) instead of the LDS-tiled one (the same bits; A/B runs). */
int kmamd_kmeans_assign(int metric, uint32_t samples_size, uint16_t features_size, uint32_t clusters_size, int device,
                        int32_t device_ptrs, int32_t fp16x2, int32_t verbosity, const void *samples,
                        const void *centroids, uint32_t *assignments /* samples_size */,
                        float *distances /* optional, samples_size */,
                        uint32_t *cluster_counts /* optional, clusters_size */,
                        double *cluster_distance_sums /* optional, clusters_size */);
/* The m nearest centroids of every row, in the order one assignment pass would find them (beyond the reference;
 * DESIGN.md 4.11).  Stateless and synchronous; device, device_ptrs, fp16x2, the chunks (KMCUDA_AMD_ASSIGN_CHUNK) and a
 * shorter last chunk as kmamd_kmeans_assign.
 *   key(s, c)  what kmamd_lloyd_assign compares: L2 RD(-2 prod(s, c) + (0 + csqr(c))) with the reference's round-down-FMA
 *              Kahan chains; angular the clamp rule on the Kahan product (>= 1: 0, <= -1: pi, else acos) with the C
 *              library's acosf restated on the device (the CPU oracle's bits, not the device library's acosf).
 *              A centroid qualifies for a row iff key < FLT_MAX (the reference's strict `<` from FLT_MAX): a NaN, inf or
 *              overflowing centroid never does.
 *   top_assignments[s * m + j]  the j-th qualifying centroid of row s by (key ascending, centroid index ascending);
 *              clusters_size ("no cluster") in the slots beyond the number of qualifying centroids, and in all m slots
 *              of a row whose first feature is NaN.  Slot 0 is what kmamd_kmeans_assign assigns.
 *   top_distances[s * m + j]    optional: the reference's distance(row, centroid) as kmamd_kmeans_assign reports it
 *              -- L2: the square root of the Kahan sum of squared differences, NOT the key, so that the distances of
 *              neighbouring ranks may step backwards by a last place; angular: the key itself -- NaN for "no cluster".
 * 1 <= m <= min(clusters_size, 64).  samples_size == 0 is success.  InvalidArguments before any device work, with the
 * outputs untouched: m out of range, and everything kmamd_kmeans_assign refuses (bad sizes, null pointers, device_ptrs
 * naming another device, KMCUDA_AMD_FP16_STRICT=1 with fp16x2 rows).
 * Rows of up to 256 features (and up to 2^19 centroids) are filtered on the matrix cores: exact keys are evaluated only
 * for the centroids whose score lies within the filter's error bound of the m-th best; wider rows take the exhaustive
 * exact kernel.  KMCUDA_AMD_ASSIGN_TOP=exact: that kernel alone for every shape (the cross-check; the same bits).
 * KMCUDA_AMD_ASSIGN_TOP_ROWS=<rows> (tests): rows per score matrix of the filtered path.  No floating-point atomics: two
 * identical calls give identical bits. */
int kmamd_kmeans_assign_top(int metric, uint32_t samples_size, uint16_t features_size, uint32_t clusters_size,
                            uint32_t m, int device, int32_t device_ptrs, int32_t fp16x2, int32_t verbosity,
                            const void *samples, const void *centroids,
                            uint32_t *top_assignments /* samples_size x m */,
                            float *top_distances /* optional, samples_size x m */);
/* the last kmamd_kmeans_assign_top call of this process that succeeded: the exact keys it evaluated and its row-centroid
 * pairs in all (samples_size * clusters_size); either pointer may be null */
int kmamd_assign_top_stats(uint64_t *pairs_exact, uint64_t *pairs_total);
/* The distance pass of kmamd_kmeans_assign on its own, enqueued on hip_stream (device pointers on `device`, fp32):
 * distances[s] = distance(row s, centroid assignments[s]), NaN where assignments[s] >= clusters (no centroid is read).
 * KMCUDA_AMD_ASSIGN_DIST=member applies.  A window for tests and for timing the kernel (scripts/assign_bench.py). */
int kmamd_assigned_distances(int metric, uint32_t n_rows, uint32_t features, uint32_t clusters, int device,
                             const float *samples, const float *centroids, const uint32_t *assignments,
                             float *distances, void *hip_stream);

/* k-means|| seeding (Bahmani et al., "Scalable K-Means++"; no counterpart in the reference): K seeds, each
 * bit-equal to an input row, from a handful of passes over the rows instead of k-means++'s K - 1 dependent ones.
 * Stateless and synchronous.  metric, fp16x2, device and device_ptrs as kmamd_kmeans_assign (features_size counts halves
 * under fp16x2); samples and centroids are host buffers (device_ptrs = -1) or buffers on `device`; every other pointer
 * is HOST memory.
 *   h(seed, r, s)   splitmix64's finaliser (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 *                   z ^= z >> 31) of z = ((uint64)r << 32 | s) + ((uint64)seed + 1) * 0x9E3779B97F4A7C15 mod 2^64;
 *                   U(seed, r, s) = (h >> 11) * 2^-53.  No generator state: a row's draw depends on (seed, r, s) alone.
 *   term t[s]       the float32 distance (kmamd_kmeans_assign's `distances`, not squared: what k-means++ draws with) of
 *                   row s to its nearest candidate so far; 0 for good for a row whose first feature is NaN; a term that
 *                   is NaN or inf counts as 0 in everything below, and a term of 0 is never drawn.
 *   round 0         the first candidate is the first row at or cyclically after h(seed, 0, 0) % N whose first feature is
 *                   not NaN (none: InvalidArguments); t[s] = distance(row s, that row), where that is not NaN.
 *   round 1..R      phi = the fp64 sum of the terms (per 256 rows in a fixed tree, the blocks in a fixed order: two
 *                   identical calls give identical bits); row s is drawn iff U(seed, r, s) * phi <
 *                   (double)oversampling * (double)t[s], each side one fp64 product.  The drawn rows in ascending order
 *                   are the round's M new candidates (no cap).  M >= 2: t[s] <- d[s] where d[s] < t[s], d being
 *                   kmamd_kmeans_assign's distances against the new candidates; M == 1: d[s] the distance to that row.
 *                   phi == 0 draws nothing.
 *   weights         counts[j] = kmamd_kmeans_assign(rows, all candidates).cluster_counts[j] (the lowest index wins a
 *                   tie); a candidate of count 0 -- a duplicate of an earlier one -- is dropped, the live ones keep
 *                   their order.
 *   seeds           the K seeds kmamd_kmeans_weighted(init = k-means++, tolerance = 1, yinyang_t = 0, seed) draws over
 *                   the live candidates with weights (float)count: no Lloyd iteration runs on the candidates.  With
 *                   fewer than K live candidates: that call on the ROWS, unweighted -- plain k-means++ -- and
 *                   *fell_back = 1.
 * rounds: 1..64, 0 = 5.  oversampling: the expected number of draws per round, finite and > 0; 0 = 2 * clusters_size.
 * Optional reports: candidate_rows / candidate_counts receive the row ids and counts of the first candidate_capacity
 * candidates (dropped ones included, with count 0), *n_candidates their number in all, round_ends[r] (rounds + 1
 * entries) the number of candidates after round r, *fell_back 0 or 1.
 * InvalidArguments before any device work, with the outputs untouched: bad sizes, clusters_size < 2 or > samples_size,
 * rounds > 64, oversampling not finite or < 0, null samples / centroids, device_ptrs naming another device,
 * KMCUDA_AMD_FP16_STRICT=1 with fp16x2 rows.  KMCUDA_AMD_TIMING=1: the phases' wall-clock laps on stderr. */
int kmamd_kmeans_seed_parallel(int metric, uint32_t samples_size, uint16_t features_size, uint32_t clusters_size,
                               uint32_t rounds /* 0: 5 */, float oversampling /* 0: 2 * K */, uint32_t seed,
                               int device, int32_t device_ptrs, int32_t fp16x2, int32_t verbosity,
                               const void *samples, void *centroids /* K x D out, the rows' dtype */,
                               uint32_t *candidate_rows /* optional */, uint32_t *candidate_counts /* optional */,
                               uint32_t candidate_capacity,
                               uint32_t *n_candidates /* optional out: all candidates, dropped included */,
                               uint32_t *round_ends /* optional, rounds + 1: candidates after round 0..R */,
                               int32_t *fell_back /* optional */);
/* kmeans_cuda's init = kmcudaInitMethodParallel (kmcuda.h): init_params of that init is NULL or points to one of
 * these; 0 means the default. */
typedef struct {
  uint32_t rounds;
  float oversampling;
} kmamd_seed_parallel_params;

/* Mini-batch K-means (Sculley, "Web-Scale K-Means Clustering"; the per-centre learning rate of scikit-learn's
 * MiniBatchKMeans.partial_fit; no counterpart in the reference): a model that stays on the device
 * between calls and is updated with new rows, a stream, or draws from a corpus of any size.
 *   state      K x D float32 centroids C, K float64 cluster weights W >= 0, a step counter t.  The centroids are float32
 *              also when the rows are halves: a half centroid would swallow updates smaller than its last place.
 *   one step   n rows X (float32, or halves with fp16x2 != 0: fp32 arithmetic on the half values) and optional float32
 *              weights w, finite and > 0 (none: every w = 1):
 *              1. a = kmamd_kmeans_assign(X, C).assignments: one filtered, bit-exact pass.  A row whose first feature is
 *                 NaN or whose distances are all NaN gets K and takes no part; a NaN centroid is never chosen.
 *              2. for every cluster c with members in the batch: n_c = sum of w_i in fp64, S_c = sum of
 *                 (double)w_i * (double)x_i in fp64 over the members in ascending batch position, in a FIXED association
 *                 that depends on the member list alone (DESIGN.md 4.3's list_sum).  No floating-point atomics: two
 *                 identical calls give identical bits.
 *              3. W'_c = W_c + n_c;  L2: C'_c[f] = (float)(((double)C_c[f] * W_c + S_c[f]) / W'_c);  angular:
 *                 v = C_c * W_c + S_c, C'_c = (float)(v / |v|) (|v|: the fp64 root of the sum of squares, in a fixed
 *                 order).  A cluster without a member in the batch keeps C_c and W_c bit for bit -- an unvisited centre
 *                 stays where it is; it is NOT set to NaN as an emptied cluster of kmeans_cuda is.  With W_c = 0 the
 *                 seed is forgotten: the centre becomes the batch mean of its members.
 *              4. t += 1 (also for n == 0, which changes nothing else).
 *   fit        over a corpus of N rows: `steps` steps of `batch` rows each.  Slot j of the step with counter t holds row
 *              floor(h(seed, (uint32)t, j) * N / 2^64) -- h: k-means||'s hash above; the high 64 bits of the 128-bit
 *              product: rows are drawn with replacement --, with its weight.  t is the handle's running counter, so
 *              fit(.., 10) twice is fit(.., 20).  No early stop.
 * create: centroids K x D float32 and cluster_weights (K float64, or NULL: zeros) are copied; device_ptrs -1: host
 * buffers, else buffers on `device`.  step / fit: rows, weights and assignments (optional out, n words) are host buffers
 * (device_ptrs -1) or buffers on the handle's device; a step holds at most kmamd_kmeans_assign's chunk of rows (env
 * KMCUDA_AMD_ASSIGN_CHUNK).  read: any of the three outputs may be NULL; steps_done is host memory.  All calls are
 * synchronous.  A fit on a device-resident corpus draws and gathers on the device and reads nothing back between its
 * steps; on a host corpus the host gathers every batch into pinned memory while the device works on the step before.
 * InvalidArguments before any device work, with the outputs and the state untouched and *out left NULL: a bad metric,
 * features == 0 or > 65535, an odd feature count with fp16x2, clusters < 2, device_ptrs naming another device, null
 * pointers (handle, centroids, rows), more rows than the chunk, batch == 0 or samples_size == 0 in fit, a cluster
 * weight that is negative or not finite, KMCUDA_AMD_FP16_STRICT=1 with fp16x2 rows.  (Cluster weights passed on the
 * device are looked at after they were copied; nothing has been handed out by then.)  A sample weight that is not
 * finite and > 0 is InvalidArguments with C, W and t unchanged. */
typedef struct kmamd_minibatch kmamd_minibatch;
int kmamd_minibatch_create(kmamd_minibatch **out, int metric, uint32_t features, uint32_t clusters, int device,
                           int32_t device_ptrs, int32_t verbosity, const float *centroids,
                           const double *cluster_weights /* optional */);
int kmamd_minibatch_step(kmamd_minibatch *h, uint32_t n_rows, int32_t fp16x2, const void *rows,
                         const float *weights /* optional */, uint32_t *assignments /* optional out */,
                         int32_t device_ptrs);
int kmamd_minibatch_fit(kmamd_minibatch *h, uint64_t samples_size, int32_t fp16x2, const void *samples,
                        const float *weights /* optional */, uint32_t batch, uint32_t steps, uint32_t seed,
                        int32_t device_ptrs);
int kmamd_minibatch_read(kmamd_minibatch *h, float *centroids, double *cluster_weights, uint64_t *steps_done,
                         int32_t device_ptrs);
void kmamd_minibatch_destroy(kmamd_minibatch *h);

/* host -> raw device pointer copy on `device` (what python.cc:330-345 does with cudaMemcpy for imported
 * centroids in device-pointer mode; lets a binding without a HIP runtime of its own fill caller-owned memory). */
int kmamd_copy_to_device(int device, void *dst, const void *host_src, size_t bytes);

/* Library identification: returns the gfx arch string this library was compiled for. */
const char *kmamd_build_arch(void);

#ifdef __cplusplus
}
#endif
#endif /* KMCUDA_AMD_H */
