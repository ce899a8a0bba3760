// kmcuda_api.cpp -- the drop-in C ABI: kmeans_cuda() and knn_cuda() of include/kmcuda.h (knn_cuda()'s argument checks;
// its host job is knn_job.cpp).
//
// Host orchestration mirroring the reference's contract (src/kmcuda.cc:402-531 kmeans_cuda,
// src/kmeans.cu:934-1026 kmeans_cuda_lloyd, :1028-1263 kmeans_cuda_yy): same argument
// validation and return codes, same srand()/rand()-driven seeding, same stop rule evaluated
// BEFORE the centroid update, same "iteration %d: %u reassignments" progress lines.
//
// What is different by design: samples stay row-major and are ROW-SHARDED over the GPUs of
// the device mask (the reference replicates everything on every GPU and exchanges slices by
// N*(N-1) peer copies); the only per-iteration exchange is one all-reduce of the centroid
// deltas (RCCL over xGMI, loaded lazily so single-GPU use has no RCCL dependency).
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/kmcuda.h"
#include "../../include/kmcuda_amd.h"
#include "engine.hpp"
#include "knn_host.hpp"

using namespace kmx;

#define INFO(...) do { if (verbosity > 0) { printf(__VA_ARGS__); } } while (false)
#define DEBUG(...) do { if (verbosity > 1) { printf(__VA_ARGS__); } } while (false)
#define RETERR(call) do { int rc__ = (call); if (rc__ != 0) return static_cast<KMCUDAResult>(rc__); } while (false)

namespace {

constexpr double kYinyangGroupTolerance = 0.02;      // kmeans.cu:27
constexpr double kYinyangDraftReassignments = 0.11;  // kmeans.cu:28
constexpr double kYinyangRefreshEpsilon = 1e-4;      // kmeans.cu:29

// ---------------------------------------------------------------------------------------
// RCCL, loaded on first multi-GPU use
// ---------------------------------------------------------------------------------------
struct Rccl {
  void *handle = nullptr;
  int (*CommInitAll)(void **, int, const int *) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
  bool load() {
    if (handle) return true;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (handle) break;
    }
    if (!handle) return false;
    CommInitAll = (decltype(CommInitAll))dlsym(handle, "ncclCommInitAll");
    CommDestroy = (decltype(CommDestroy))dlsym(handle, "ncclCommDestroy");
    GroupStart = (decltype(GroupStart))dlsym(handle, "ncclGroupStart");
    GroupEnd = (decltype(GroupEnd))dlsym(handle, "ncclGroupEnd");
    AllReduce = (decltype(AllReduce))dlsym(handle, "ncclAllReduce");
    return CommInitAll && CommDestroy && GroupStart && GroupEnd && AllReduce;
  }
};
constexpr int kNcclFloat64 = 8, kNcclSum = 0;  // rccl.h ncclDataType_t / ncclRedOp_t

// ---------------------------------------------------------------------------------------
// device list from the mask (reference: setup_devices, kmcuda.cc:63-137)
// ---------------------------------------------------------------------------------------
std::vector<int> setup_devices(uint32_t device, int verbosity) {
  std::vector<int> devs;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return devs;
  if (device == 0) device = ndev >= 32 ? 0xFFFFFFFFu : ((1u << ndev) - 1);
  for (int dev = 0; device; dev++, device >>= 1) {
    if (!(device & 1)) continue;
    if (dev >= ndev || hipSetDevice(dev) != hipSuccess) {
      INFO("failed to hipSetDevice(%d)\n", dev);
      continue;
    }
    devs.push_back(dev);
  }
  return devs;
}

// contiguous row blocks, one per shard (the reference's distribute(), private.h:240-273,
// aligns to 512 B; rows here are whole samples so plain balanced blocks do)
// Shards of at least 1024 rows start on multiples of 256 rows: the k-means++ chooser's exact block sums (256 rows) and
// the reference's butterfly sums (aligned groups of 32 rows, kmeans.cu:63-66) then never straddle two shards, and the
// per-shard sums concatenate into the one-shard sums (seeding.hip: kmpp_choose_kernel).
std::vector<std::pair<uint32_t, uint32_t>> row_plan(uint32_t N, size_t nshards) {
  std::vector<std::pair<uint32_t, uint32_t>> plan;
  const bool align = nshards > 1 && (uint64_t)N / nshards >= 1024u;
  auto start = [&](size_t i) -> uint32_t {
    if (i >= nshards) return N;
    const uint32_t o = (uint32_t)(((uint64_t)N * i) / nshards);
    return align ? (o & ~255u) : o;
  };
  for (size_t i = 0; i < nshards; i++) plan.emplace_back(start(i), start(i + 1) - start(i));
  return plan;
}

// sum of `n` floats the way the reference forms it on device (kmeans.cu:63-66, :687-690):
// float butterfly over each aligned group of 32, then a double accumulation
static float butterfly_group(const float *v, uint32_t base, uint32_t n) {
  float lane[32];
  for (int l = 0; l < 32; l++) lane[l] = (base + l < n) ? v[base + l] : 0.f;
  for (int off = 16; off > 0; off /= 2)
    for (int l = 0; l < 32; l++) lane[l] = lane[l] + ((l + off < 32) ? lane[l + off] : lane[l]);
  return lane[0];
}

double butterfly_sum(const float *v, uint32_t n) {
  const uint32_t groups = (n + 31) / 32;
  if (groups < 4096) {
    double sum = 0.0;
    for (uint32_t g = 0; g < groups; g++) sum += (double)butterfly_group(v, g * 32, n);
    return sum;
  }
  // the group sums are independent (threads), the double accumulation keeps its sequential order
  std::vector<float> gs(groups);
  unsigned nt = std::thread::hardware_concurrency();
  nt = nt == 0 ? 4 : (nt > 16 ? 16 : nt);
  std::vector<std::thread> pool;
  const uint32_t per = (groups + nt - 1) / nt;
  for (unsigned t = 0; t < nt; t++) {
    const uint32_t g0 = t * per, g1 = std::min(groups, g0 + per);
    if (g0 >= g1) break;
    pool.emplace_back([&gs, v, n, g0, g1]() {
      for (uint32_t g = g0; g < g1; g++) gs[g] = butterfly_group(v, g * 32, n);
    });
  }
  for (auto &th : pool) th.join();
  double sum = 0.0;
  for (uint32_t g = 0; g < groups; g++) sum += (double)gs[g];
  return sum;
}

// ---------------------------------------------------------------------------------------
// One host thread per shard for the lifetime of the job.  A multi-GPU iteration is a dozen launches per GPU
// and lasts well under a millisecond on a 1M-row shard: enqueueing eight GPUs from one thread, or creating and
// joining eight threads per iteration, costs about as much as the GPUs take to run it.
// ---------------------------------------------------------------------------------------
class ShardWorkers {
 public:
  ~ShardWorkers() {
    {
      std::lock_guard<std::mutex> l(m_);
      quit_ = true;
      gen_++;
    }
    cv_go_.notify_all();
    for (auto &t : threads_) t.join();
  }
  size_t size() const { return threads_.size(); }
  void start(size_t n) {
    rcs_.assign(n, 0);
    for (size_t i = 0; i < n; i++) threads_.emplace_back([this, i]() { loop(i); });
  }
  // fn(i) on worker i, for every i; returns when all are done, with the first non-zero code
  int run(const std::function<int(size_t)> &fn) {
    {
      std::lock_guard<std::mutex> l(m_);
      fn_ = &fn;
      pending_ = threads_.size();
      gen_++;
    }
    cv_go_.notify_all();
    std::unique_lock<std::mutex> l(m_);
    cv_done_.wait(l, [this]() { return pending_ == 0; });
    for (int rc : rcs_)
      if (rc) return rc;
    return 0;
  }

 private:
  void loop(size_t i) {
    uint64_t seen = 0;
    for (;;) {
      const std::function<int(size_t)> *fn;
      {
        std::unique_lock<std::mutex> l(m_);
        cv_go_.wait(l, [&]() { return gen_ != seen; });
        seen = gen_;
        if (quit_) return;
        fn = fn_;
      }
      const int rc = (*fn)(i);
      {
        std::lock_guard<std::mutex> l(m_);
        rcs_[i] = rc;
        if (--pending_ == 0) cv_done_.notify_one();
      }
    }
  }
  std::mutex m_;
  std::condition_variable cv_go_, cv_done_;
  std::vector<std::thread> threads_;
  std::vector<int> rcs_;
  const std::function<int(size_t)> *fn_ = nullptr;
  uint64_t gen_ = 0;
  size_t pending_ = 0;
  bool quit_ = false;
};

// ---------------------------------------------------------------------------------------
// one GPU's share of the job
// ---------------------------------------------------------------------------------------
struct Shard {
  int dev = 0;
  uint32_t offset = 0, length = 0;
  std::unique_ptr<Engine> eng;
  const float *samples = nullptr;  // length x D on this device
  float *centroids = nullptr;      // K x D (replicated)
  uint32_t *assignments = nullptr, *prev = nullptr, *ccounts = nullptr;
  double *reduce = nullptr;        // the iteration's ONE exchange: [delta K*D | dcount K | counters 4] (kmcuda_amd.h)
  float *dists = nullptr;          // length floats (k-means++ / average distance)
  const float *weights = nullptr;  // length floats: the rows' sample weights (kmamd_kmeans_weighted), or null
  float *wterms = nullptr;         // length floats: w * dists, what the weighted k-means++ chooser sums
  // Yinyang state (allocated when the Yinyang phase starts; reference: kmcuda.cc:448-470)
  float *bounds = nullptr;         // (G+1) x length, group-major (kmeans.cu:431-485 layout)
  float *drifts = nullptr;         // K*D old centroids + K per-centroid drifts
  float *gdrifts = nullptr;        // G per-group max drifts
  uint32_t *passed = nullptr;      // length
  hipEvent_t ev_filled = nullptr;  // several shards on one device: this shard's reduce buffer is written
  ~Shard() {
    (void)hipSetDevice(dev);
    if (ev_filled) (void)hipEventDestroy(ev_filled);
  }
  // device memory of the job's lifetime: the engine's (small buffers share its slabs, a large one is its own hipMalloc)
  template <typename T>
  int alloc(T **p, size_t count) { return eng->alloc(p, count); }
  // enqueues the copy of `count` elements of a caller buffer -- host memory (device_ptrs < 0) or device device_ptrs'
  // -- into dst, on this shard's stream
  template <typename T>
  int copy_in(T *dst, const T *src, size_t count, int32_t device_ptrs) {
    const hipError_t e = device_ptrs < 0
                             ? hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, eng->stream_)
                             : hipMemcpyPeerAsync(dst, dev, src, device_ptrs, count * sizeof(T), eng->stream_);
    return e == hipSuccess ? 0 : kmcudaMemoryCopyError;
  }
  // The one rule for a caller's read-only buffer (DeviceArena::stage_in's, host_job.hpp): used in place where it lies
  // on this shard's device, otherwise copied into a buffer of alloc()
  template <typename T>
  int stage_in(const T *src, size_t count, int32_t device_ptrs, const T **dst) {
    if (device_ptrs >= 0 && device_ptrs == dev) {
      *dst = src;
      return 0;
    }
    T *buf = nullptr;
    int rc = alloc(&buf, count);
    if (rc == 0) rc = copy_in(buf, src, count, device_ptrs);
    *dst = buf;
    return rc;
  }
};

// glibc's rand() (random_r, TYPE_3: 31 words, r[k] = r[k - 31] + r[k - 3], output r[k] >> 1) restated, for the one place
// that draws N numbers (init = "random").  attach(seed): called right after srand(seed); checks the restatement against
// the library's own first draws (false: not this generator -- the caller uses rand()), then moves the library onto a
// scratch buffer (initstate) while detach() overwrites the library's OWN state table with the restated generator's state
// and moves it back (setstate): the library's rand() goes on exactly where the same number of rand() calls would have
// left it, in its own memory.
class GlibcRand {
 public:
  bool attach(uint32_t seed) {
    seed_ = seed;
    reseed();
    uint32_t mine[4];
    for (uint32_t &v : mine) v = next();
    bool same = true;
    for (uint32_t v : mine) same = same && (uint32_t)rand() == v;
    srand(seed);   // back to the start for either path
    if (!same) return false;
    reseed();
    return true;
  }
  uint32_t next() {
    s_[f_] += s_[r_];
    const uint32_t out = s_[f_] >> 1;
    f_ = f_ + 1 == 31 ? 0 : f_ + 1;
    r_ = r_ + 1 == 31 ? 0 : r_ + 1;
    return out;
  }
  void detach() {
    // The generator goes back to the C library's OWN state table (or whatever buffer the caller had installed), with
    // the restated generator's words in it: initstate() parks the library on a scratch buffer and returns the table
    // it was using, the table is overwritten, setstate() moves the library back onto it.  Nothing of this library
    // stays referenced by rand() afterwards (round 4 left the library on a static buffer of ours: a dlclose away
    // from unmapped memory).  attach() has verified that the table is the 31-word TYPE_3 one.
    static std::mutex m;
    std::lock_guard<std::mutex> lock(m);
    int32_t scratch[32];
    char *table = initstate(1u, reinterpret_cast<char *>(scratch), sizeof(scratch));
    if (!table) return;
    int32_t *st = reinterpret_cast<int32_t *>(table);
    for (int i = 0; i < 31; i++) st[1 + i] = (int32_t)s_[i];
    st[0] = (int32_t)(r_ * 5 + 3);   // glibc: rear * MAX_TYPES + TYPE_3 (setstate() reads type and position from it)
    (void)setstate(table);           // (stores the scratch buffer's position word first: into `scratch`, ours)
  }

 private:
  void reseed() {   // srandom_r: 16807 LCG fills the table, 310 outputs are discarded
    int32_t word = seed_ ? (int32_t)seed_ : 1;
    s_[0] = (uint32_t)word;
    for (int i = 1; i < 31; i++) {
      const long hi = word / 127773, lo = word % 127773;
      long w = 16807 * lo - 2836 * hi;
      if (w < 0) w += 2147483647;
      word = (int32_t)w;
      s_[i] = (uint32_t)word;
    }
    f_ = 3;
    r_ = 0;
    for (int i = 0; i < 310; i++) (void)next();
  }
  uint32_t s_[31], seed_ = 0;
  int f_ = 3, r_ = 0;
};

// what the last kmeans_cuda() call did (kmamd_last_run_stats): iterations of the Lloyd / Yinyang loops and
// the wall time spent in them (everything after seeding), for drivers that time the drop-in entry point
struct RunStats {
  uint32_t iterations = 0; double loop_seconds = 0, setup_seconds = 0; uint32_t shards = 0, rccl = 0;
  // kmamd_last_run_collective: the per-iteration all-reduce as HIP events on the first shard's stream saw it
  double collective_ms = 0; uint32_t collectives = 0;
};
RunStats g_last_run;        // published once per kmeans_cuda() call, under g_last_run_mutex (the Python module
std::mutex g_last_run_mutex;  // releases the GIL around the call: two threads may be inside the library)

// The KMCUDA_AMD_* switches of kmeans_cuda(), read once when the call starts (tests change them between calls); the
// job, its nested group-clustering job and the seeding take them from here.  The engines' own switches (engine.cpp,
// seeding.hip, lloyd_carry.hip) are theirs.
struct KmeansSwitches {
  bool timing = false;           // KMCUDA_AMD_TIMING (set at all): laps and iteration stamps on stderr
  bool exact_update = false;     // KMCUDA_AMD_EXACT_UPDATE: the reference's serial Kahan chain (single shard)
  bool fp16_strict = false;      // KMCUDA_AMD_FP16_STRICT: the reference's half2 arithmetic (fp16x2 only)
  enum class Yy { unset, reference, carry } yy = Yy::unset;   // KMCUDA_AMD_YY (anything else: unset)
  double yy_switch = -1.0;       // KMCUDA_AMD_YY_SWITCH=<fraction> (tests; negative: unset)
  enum class Carry { unset, off, on } carry = Carry::unset;   // KMCUDA_AMD_CARRY: 0 / non-zero
  bool speculate = true;         // KMCUDA_AMD_SPECULATE=0: every iteration waits for its stop test before its update
  bool time_collective = false;  // KMCUDA_AMD_TIME_COLLECTIVE
  bool force_rccl = false;       // KMCUDA_AMD_FORCE_RCCL (test hook)
  bool kmpp_host = false;        // KMCUDA_AMD_KMPP_HOST (set at all): k-means++ chooses on the host
  int kmpp_filter = 1;           // KMCUDA_AMD_KMPP_FILTER: 0 plain steps, >= 2 filtered steps for small jobs too
  bool update_trace = false;     // KMCUDA_AMD_UPDATE_TRACE (set at all)
  bool preload = true;           // KMCUDA_AMD_PRELOAD=0: no helper thread loads the code objects
  int virtual_shards = 0;        // KMCUDA_AMD_VIRTUAL_SHARDS: row shards on one GPU (test hook)
  // KMCUDA_AMD_YY_SWITCH (tests): hand over to the reference's bounds once the reassigned fraction is at most that
  bool hand_over_forced() const { return yy_switch >= 0; }
  bool hand_over_now(uint32_t changed, uint32_t N) const { return hand_over_forced() && (double)changed <= yy_switch * (double)N; }
};
KmeansSwitches kmeans_switches() {
  KmeansSwitches sw;
  auto on = [](const char *v) { return v && atoi(v) != 0; };
  sw.timing = getenv("KMCUDA_AMD_TIMING") != nullptr;
  sw.exact_update = on(getenv("KMCUDA_AMD_EXACT_UPDATE"));
  sw.fp16_strict = fp16_strict_requested();
  if (const char *v = getenv("KMCUDA_AMD_YY"))
    sw.yy = strcmp(v, "reference") == 0 ? KmeansSwitches::Yy::reference
                                        : (strcmp(v, "carry") == 0 ? KmeansSwitches::Yy::carry : KmeansSwitches::Yy::unset);
  if (const char *v = getenv("KMCUDA_AMD_YY_SWITCH")) sw.yy_switch = atof(v);
  if (const char *v = getenv("KMCUDA_AMD_CARRY")) sw.carry = atoi(v) != 0 ? KmeansSwitches::Carry::on : KmeansSwitches::Carry::off;
  if (const char *v = getenv("KMCUDA_AMD_SPECULATE")) sw.speculate = atoi(v) != 0;
  sw.time_collective = on(getenv("KMCUDA_AMD_TIME_COLLECTIVE"));
  sw.force_rccl = on(getenv("KMCUDA_AMD_FORCE_RCCL"));
  sw.kmpp_host = getenv("KMCUDA_AMD_KMPP_HOST") != nullptr;
  if (const char *v = getenv("KMCUDA_AMD_KMPP_FILTER")) sw.kmpp_filter = atoi(v);
  sw.update_trace = getenv("KMCUDA_AMD_UPDATE_TRACE") != nullptr;
  if (const char *v = getenv("KMCUDA_AMD_PRELOAD")) sw.preload = atoi(v) != 0;
  if (const char *v = getenv("KMCUDA_AMD_VIRTUAL_SHARDS")) sw.virtual_shards = atoi(v);
  return sw;
}

// What the schedule of one call is going to be (Job::plan_schedule)
struct SchedulePlan {
  // kmeans.cu:1037-1050: no Yinyang phase at all
  enum class LloydOnly { no, too_few_clusters, tolerance_too_high } lloyd_only = LloydOnly::no;
  bool adaptive = false;        // behind the hand-over point: Lloyd passes go on (else the reference's bounds)
  bool carry = false;           // ... and may carry per-row bounds from pass to pass
  bool carry_at_once = false;   // ... from the first pass on, not once the run has been seen to go on
  bool cluster_groups_for_real = true;   // the groups are clustered (else only the draws of their seeding are replayed)
};

class Job {
 public:
  uint32_t N = 0, D = 0, K = 0;
  int metric = 0, verbosity = 0;
  KmeansSwitches sw;  // the call's switches (setup(); a nested job gets its parent's)
  bool fp16 = false;  // fp16x2 boundary: half buffers outside, fp32 arithmetic on the half values inside
  // KMCUDA_AMD_FP16_STRICT=1 (fp16x2 jobs, one GPU): every step in the reference's half2 ARITHMETIC
  // (half2_strict.hip) -- the verification mode the oracle's half2 restatement is compared with
  bool strict_h2 = false;
  RunStats stats;   // this job's own counts (a nested group-clustering job has its own)
  // Sample weights (kmamd_kmeans_weighted): sharded with the rows; the engines run the weighted update, the reduce
  // buffers end in [K cluster-weight deltas | reassigned weight] and the stop tests compare WEIGHT: the reassigned
  // weight against tolerance * weight_total, in the float arithmetic of the counts' rule (kmeans.cu:707)
  bool weighted = false;
  double weight_total = 0.0;   // the shards' fp64 totals, added in shard order
  size_t reduce_len() const { return (size_t)K * D + K + 4 + (weighted ? (size_t)K + 1 : 0); }
  float stop_threshold(float tolerance) const { return weighted ? tolerance * (float)weight_total : tolerance * N; }
  std::vector<std::unique_ptr<Shard>> shards;
  ShardWorkers workers;   // (after `shards`: joined before the shards go)
  Rccl rccl;
  std::vector<void *> comms;
  // several shards on ONE device (KMCUDA_AMD_VIRTUAL_SHARDS): the all-reduce's stand-in is a sum kernel on the
  // first shard's stream, ordered with the others by events -- the dependency structure of the real collective
  double **reduce_ptrs_dev = nullptr;
  hipEvent_t ev_summed = nullptr;
  bool speculate = true;   // KMCUDA_AMD_SPECULATE=0: every iteration waits for its stop test before its update
  // KMCUDA_AMD_TIME_COLLECTIVE=1 (bench.py --api): a pair of HIP events around every iteration's all-reduce (its
  // stand-in under KMCUDA_AMD_VIRTUAL_SHARDS) on the first shard's stream, read when the loops are over -- so that a
  // multi-GPU run says by itself how long the collective takes (kmamd_last_run_collective)
  bool time_collective = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> coll_events;
  size_t coll_used = 0;
  int collective_mark(bool begin) {
    if (!time_collective) return 0;
    // (the caller's current device is its own business: the events belong to the first shard's device, and the device
    //  that was current comes back -- the grouped all-reduce sets its own per shard, the stand-in has set the first's)
    int prev_dev = -1;
    (void)hipGetDevice(&prev_dev);
    (void)hipSetDevice(shards[0]->dev);
    int rc = 0;
    if (begin) {
      if (coll_used == coll_events.size()) {
        if (coll_events.size() >= 4096) {   // (enough of a sample)
          time_collective = false;
        } else {
          hipEvent_t a = nullptr, b = nullptr;
          if (hipEventCreate(&a) != hipSuccess) {
            rc = kmcudaRuntimeError;
          } else if (hipEventCreate(&b) != hipSuccess) {
            (void)hipEventDestroy(a);   // (a pair or nothing: ~Job destroys pairs)
            rc = kmcudaRuntimeError;
          } else {
            coll_events.emplace_back(a, b);
          }
        }
      }
      if (rc == 0 && time_collective &&
          hipEventRecord(coll_events[coll_used].first, shards[0]->eng->stream_) != hipSuccess)
        rc = kmcudaRuntimeError;
    } else if (coll_used < coll_events.size()) {
      if (hipEventRecord(coll_events[coll_used++].second, shards[0]->eng->stream_) != hipSuccess) rc = kmcudaRuntimeError;
    }
    if (prev_dev >= 0) (void)hipSetDevice(prev_dev);
    return rc;
  }
  void collective_collect() {   // after sync_all()
    for (size_t i = 0; i < coll_used; i++) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, coll_events[i].first, coll_events[i].second) == hipSuccess) {
        stats.collective_ms += ms;
        stats.collectives++;
      }
    }
    coll_used = 0;
  }

  ~Job() {
    for (void *c : comms)
      if (c) rccl.CommDestroy(c);
    if (!shards.empty()) (void)hipSetDevice(shards[0]->dev);
    if (reduce_ptrs_dev) (void)hipFree(reduce_ptrs_dev);
    if (ev_summed) (void)hipEventDestroy(ev_summed);
    for (auto &e : coll_events) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  }

  // on_stream: the (single) shard's engine works on this existing stream instead of creating one -- the nested job
  // that clusters the centroids into groups rides on its parent's: a stream's first launches cost milliseconds
  int setup(const KmeansSwitches &sw_, const std::vector<int> &devs, int nvirtual, uint32_t N_, uint32_t D_, uint32_t K_,
            int metric_, int verbosity_, const float *samples, int32_t device_ptrs, hipStream_t on_stream = nullptr,
            const float *sample_weights = nullptr) {
    sw = sw_;
    N = N_; D = D_; K = K_; metric = metric_; verbosity = verbosity_;
    exact_update = sw.exact_update || strict_h2;   // (strict: the reference's serial update, in half2 arithmetic)
    weighted = sample_weights != nullptr;
    std::vector<int> shard_devs = devs;
    if (nvirtual > 1 && devs.size() == 1) shard_devs.assign(nvirtual, devs[0]);  // test hook
    auto plan = row_plan(N, shard_devs.size());
    for (size_t i = 0; i < shard_devs.size(); i++) {
      auto sh = std::make_unique<Shard>();
      sh->dev = shard_devs[i];
      sh->offset = plan[i].first;
      sh->length = plan[i].second;
      if (hipSetDevice(sh->dev) != hipSuccess) return kmcudaNoSuchDevice;
      sh->eng = std::make_unique<Engine>();
      int rc = sh->eng->init(sh->dev, sh->length, D, K, metric, 0, shard_devs.size() == 1 ? on_stream : nullptr);
      if (rc) return rc;
      sh->eng->strict_h2_ = strict_h2;
      const size_t n = (size_t)sh->length * D;
      if (fp16) {
        // `samples` holds halves: the raw halves on the device (kept: the f16 matrix-core filter reads the rows as
        // halves), widened into the fp32 working copy
        float *buf = nullptr;
        if ((rc = sh->alloc(&buf, n))) return rc;
        const uint16_t *dev_half = nullptr;
        if ((rc = sh->stage_in(reinterpret_cast<const uint16_t *>(samples) + (size_t)sh->offset * D, n, device_ptrs, &dev_half)))
          return rc;
        if (launch_half_to_float(dev_half, n, buf, sh->eng->stream_) != hipSuccess ||
            hipStreamSynchronize(sh->eng->stream_) != hipSuccess)
          return kmcudaRuntimeError;
        sh->samples = buf;
        sh->eng->half_rows_ = dev_half;
      } else if ((rc = sh->stage_in(samples + (size_t)sh->offset * D, n, device_ptrs, &sh->samples))) {
        return rc;   // (resident rows are used in place and never modified)
      }
      if ((rc = sh->alloc(&sh->centroids, (size_t)K * D))) return rc;
      if ((rc = sh->alloc(&sh->assignments, sh->length))) return rc;
      if ((rc = sh->alloc(&sh->prev, sh->length))) return rc;
      if ((rc = sh->alloc(&sh->ccounts, K))) return rc;
      if ((rc = sh->alloc(&sh->reduce, reduce_len()))) return rc;
      if ((rc = sh->alloc(&sh->dists, sh->length))) return rc;
      if (weighted && (rc = sh->stage_in(sample_weights + sh->offset, sh->length, device_ptrs, &sh->weights))) return rc;
      shards.push_back(std::move(sh));
    }
    bool distinct = shards.size() > 1;
    for (size_t i = 0; i < shards.size() && distinct; i++)
      for (size_t j = 0; j < i; j++)
        if (shards[i]->dev == shards[j]->dev) distinct = false;
    // KMCUDA_AMD_FORCE_RCCL=1 (test hook): a ONE-shard job also creates its (one-rank) communicator and sends its
    // reduce buffer through ncclAllReduce every iteration -- the library loading, the entry points' signatures, the
    // enum values and the stream the collective is enqueued on get exercised on a box with a single GPU
    const bool force_rccl = shards.size() == 1 && sw.force_rccl;
    if (distinct || force_rccl) {
      if (!rccl.load()) {
        INFO("failed to load librccl.so: multi-GPU operation is unavailable\n");
        return kmcudaRuntimeError;
      }
      std::vector<int> ids;
      for (auto &s : shards) ids.push_back(s->dev);
      comms.resize(ids.size(), nullptr);
      if (rccl.CommInitAll(comms.data(), (int)ids.size(), ids.data()) != 0) return kmcudaRuntimeError;
    } else if (shards.size() > 1) {
      std::vector<double *> ptrs;
      for (auto &s : shards) {
        ptrs.push_back(s->reduce);
        (void)hipSetDevice(s->dev);
        if (hipEventCreateWithFlags(&s->ev_filled, hipEventDisableTiming) != hipSuccess) return kmcudaRuntimeError;
      }
      (void)hipSetDevice(shards[0]->dev);
      if (hipMalloc((void **)&reduce_ptrs_dev, ptrs.size() * sizeof(double *)) != hipSuccess)
        return kmcudaMemoryAllocationFailure;
      if (hipMemcpy(reduce_ptrs_dev, ptrs.data(), ptrs.size() * sizeof(double *), hipMemcpyHostToDevice) != hipSuccess)
        return kmcudaMemoryCopyError;
      if (hipEventCreateWithFlags(&ev_summed, hipEventDisableTiming) != hipSuccess) return kmcudaRuntimeError;
    }
    speculate = sw.speculate;
    time_collective = sw.time_collective && (shards.size() > 1 || !comms.empty());
    RETERR(sync_all());  // uploads complete: later cross-stream reads of the samples are safe
    for (auto &s : shards) {   // (every weight finite and > 0, or InvalidArguments before any clustering work)
      if (!weighted) break;
      (void)hipSetDevice(s->dev);
      RETERR(s->eng->set_weights(s->weights));
      weight_total += s->eng->weight_total_;
    }
    return 0;
  }

  int sync_all() {
    for (auto &s : shards) RETERR(s->eng->sync());
    return 0;
  }

  // ---- replicated-state helpers ----
  // the shard that holds sample row `index` (global numbering)
  Shard *owner_of(uint32_t index) {
    for (auto &s : shards)
      if (index >= s->offset && index < s->offset + s->length) return s.get();
    return nullptr;
  }

  // copies sample row `index` (global numbering) into centroid slot `slot` on every shard
  int copy_sample_to_centroid(uint32_t index, uint32_t slot) {
    Shard *owner = owner_of(index);
    if (!owner) return kmcudaRuntimeError;
    const float *src = owner->samples + (size_t)(index - owner->offset) * D;
    for (auto &s : shards) {
      hipError_t e;
      float *dst = s->centroids + (size_t)slot * D;
      // the copy is enqueued on the DESTINATION shard's stream (ordered after anything pending there),
      // with that stream's device current
      (void)hipSetDevice(s->dev);
      if (s->dev == owner->dev)
        e = hipMemcpyAsync(dst, src, D * sizeof(float), hipMemcpyDeviceToDevice, s->eng->stream_);
      else
        e = hipMemcpyPeerAsync(dst, s->dev, src, owner->dev, D * sizeof(float), s->eng->stream_);
      if (e != hipSuccess) return kmcudaMemoryCopyError;
    }
    return 0;
  }

  // `count` features of sample row `index` from feature `first` on, once its shard's stream has run dry
  int read_sample(uint32_t index, uint32_t first, uint32_t count, float *out) {
    Shard *s = owner_of(index);
    if (!s) return kmcudaRuntimeError;
    (void)hipSetDevice(s->dev);
    RETERR(s->eng->sync());
    if (hipMemcpy(out, s->samples + (size_t)(index - s->offset) * D + first, count * sizeof(float),
                  hipMemcpyDeviceToHost) != hipSuccess)
      return kmcudaMemoryCopyError;
    return 0;
  }

  // ---- seeding (reference: kmeans_init_centroids, kmcuda.cc:189-400) ----
  int init_centroids(KMCUDAInitMethod method, uint32_t seed, const float *host_centroids, int32_t device_ptrs,
                     uint32_t afk_m = 0) {
    if (metric == kmcudaDistanceMetricCosine && !fp16) RETERR(check_unit_norms());  // (fp32 only)
    srand(seed);  // kmcuda.cc:222
    switch (method) {
      case kmcudaInitMethodImport:
        return seed_import(host_centroids, device_ptrs);
      case kmcudaInitMethodRandom:
        return seed_random(seed);
      case kmcudaInitMethodPlusPlus:
        RETERR(seed_plusplus());
        break;
      case kmcudaInitMethodAFKMC2:
        RETERR(seed_afkmc2(seed, afk_m));
        break;
      case kmcudaInitMethodParallel:   // (runs at the entry of kmamd_kmeans_weighted and arrives here as Import)
        return kmcudaInvalidArguments;
    }
    INFO("\rdone            \n");
    return 0;
  }

  int check_unit_norms() {  // kmcuda.cc:195-220: three unit-norm probes
    std::vector<float> probe(D);
    for (uint32_t s : {0u, N / 2, N - 1}) {
      RETERR(read_sample(s, 0, D, probe.data()));
      double norm = 0;
      for (uint32_t i = 0; i < D; i++) norm += probe[i] * probe[i];
      const float high = 1.00001, low = 0.99999;
      if (norm > high || norm < low) {
        INFO("error: angular distance: samples[%u] has L2 norm = %f which is outside [%f, %f]\n", s, norm, low, high);
        return kmcudaInvalidArguments;
      }
    }
    return 0;
  }

  // the first seed of k-means++ and AFK-MC2: random rows until one's first feature is not NaN (kmcuda.cc:265-270)
  int draw_first_seed(uint32_t *index) {
    float smoke = NAN;
    while (smoke != smoke) {
      *index = rand() % N;
      RETERR(read_sample(*index, 0, 1, &smoke));
    }
    return 0;
  }

  void seeding_progress(uint32_t step) const {
    if (verbosity > 1 || (verbosity > 0 && (K < 100 || step % (K / 100) == 0))) {
      printf("\rstep %d", step);
      fflush(stdout);
    }
  }

  // K x D centroids of the caller (host memory, or device device_ptrs') into every replica
  int seed_import(const float *host_centroids, int32_t device_ptrs) {
    const size_t n = (size_t)K * D;
    for (auto &s : shards) {
      (void)hipSetDevice(s->dev);
      if (!fp16) {
        RETERR(s->copy_in(s->centroids, host_centroids, n, device_ptrs));
        continue;
      }
      // halves -> the fp32 replica (halves that had to be copied stay in the shard's memory: K x D of them)
      const uint16_t *halves = nullptr;
      RETERR(s->stage_in(reinterpret_cast<const uint16_t *>(host_centroids), n, device_ptrs, &halves));
      if (launch_half_to_float(halves, n, s->centroids, s->eng->stream_) != hipSuccess ||
          hipStreamSynchronize(s->eng->stream_) != hipSuccess)
        return kmcudaMemoryCopyError;   // (the code this step has always failed with)
    }
    return sync_all();
  }

  int seed_random(uint32_t seed) {
    INFO("randomly picking initial centroids...\n");
    // The reference shuffles ALL N indices with libstdc++'s std::random_shuffle over rand() and takes the first K
    // (kmcuda.cc:245-253): for i = 1 .. N-1: swap(a[i], a[rand() % (i + 1)]).  Position i is untouched before its
    // own step and a value that leaves the first K never returns, so the first K entries follow from a K-entry
    // array: steps i < K swap inside it, a step i >= K whose draw j falls below K puts i at j.  Same draws, same
    // rows, no N-entry array; with glibc's generator restated (GlibcRand: a rand() call is 10-20 ns behind its
    // lock -- 45 ms of a 4M-row call, 90 ms at 8M rows) the N - 1 draws take a few ms, and rand()'s own state is
    // set to what N - 1 calls would have left.
    std::vector<uint32_t> chosen(K);
    for (uint32_t c = 0; c < K; c++) chosen[c] = c;
    GlibcRand fast;
    if (fast.attach(seed)) {
      for (uint32_t i = 1; i < N && i < K; i++) std::swap(chosen[i], chosen[fast.next() % (i + 1)]);
      for (uint32_t i = K; i < N; i++) {
        const uint32_t j = fast.next() % (i + 1);
        if (j < K) chosen[j] = i;
      }
      fast.detach();
    } else {   // another C library: its rand(), call by call
      for (uint32_t i = 1; i < N && i < K; i++) std::swap(chosen[i], chosen[rand() % (i + 1)]);
      for (uint32_t i = K; i < N; i++) {
        const uint32_t j = rand() % (i + 1);
        if (j < K) chosen[j] = i;
      }
    }
    DEBUG("shuffle complete, copying to device(s)...\n");
    if (shards.size() == 1) {   // one gather launch (the index list rides in the dists buffer: N >= K floats)
      Shard &s = *shards[0];
      (void)hipSetDevice(s.dev);
      uint32_t *idx = reinterpret_cast<uint32_t *>(s.dists);
      if (hipMemcpyAsync(idx, chosen.data(), K * sizeof(uint32_t), hipMemcpyHostToDevice, s.eng->stream_) != hipSuccess)
        return kmcudaMemoryCopyError;
      if (launch_gather_rows(s.samples, idx, K, D, s.centroids, s.eng->stream_) != hipSuccess) return kmcudaRuntimeError;
    } else {
      for (uint32_t c = 0; c < K; c++) RETERR(copy_sample_to_centroid(chosen[c], c));
    }
    return sync_all();   // (chosen[] must outlive the copy)
  }

  // k-means++ (kmcuda.cc:262-335): the scratch memory and the state of one seeding, from the second seed on.
  // Two ways to the reference's choice (kmcuda.cc:286-326).  HOST: all N distances come back (pinned, 4 N bytes per
  // step), butterfly sum and sequential double prefix sums as the reference.  DEVICE (seeding.hip): sums of floats in
  // double are exact -- order free -- while the distances' exponent range is narrow enough, so the step kernel's
  // exact block sums give the same choice from 4 bytes per batch of steps; a step whose range is too wide (or that
  // holds a NaN / inf distance) takes the host way.
  // Several row shards (round 5): every shard runs the step on its rows and leaves its own exact block sums; ONE
  // chooser kernel on the first shard's device reads them where they lie (peer access) as the concatenation they are
  // and copies the seed's row into every replica (seeding.hip: kmpp_choose_kernel) -- no N-sized transfer, no host in
  // the loop.
  struct KmppSeeding {
    // Per shard: block statistics, local prefixes, totals, the fail flag and the outlier list (the shard's own memory,
    // Shard::alloc), an event behind its step -- and for the filtered steps (seeding.hip) a centred byte copy of its
    // rows (xs8; n2c: 4 floats per row) with what goes with it, in an arena of plain hipMallocs that ends with the
    // seeding: a step's first kernel drops every row that provably is no closer to the new seed than to an earlier
    // one, the exact chains run for the rest.  Same dists[] after every step either way, hence the same seeds.
    struct PerShard {
      unsigned char *block_stats = nullptr, *totals = nullptr, *outliers = nullptr;
      double *bpre = nullptr;
      uint32_t *fail = nullptr;   // [0] the flag, [1] the exponent cut, [2] the listed values' number
      KmppOutlierBuf out;         // the step's exponent cut, the distances below it (seeding.hip: KmppOutlier)
      hipEvent_t ev_step = nullptr;
      std::unique_ptr<DeviceArena> filter_mem;
      unsigned char *xs8 = nullptr;
      float *n2c = nullptr, *mu = nullptr;
      uint32_t *stats = nullptr, *list = nullptr;
      double *part = nullptr;
    };
    Job &job;
    const std::vector<std::unique_ptr<Shard>> &shards;
    const int verbosity;
    const uint32_t dp;                  // D rounded up to 128: the byte copy's row pitch
    uint32_t log2n = 0;
    std::vector<PerShard> kpp;
    std::vector<KmppShardPtrs> views;   // what the chooser kernel reads of every shard
    hipEvent_t ev_chosen = nullptr;
    uint32_t *fail_host = nullptr;      // pinned: the first shard's fail flag after a batch of steps
    float *host_dists = nullptr;        // pinned, N floats: allocated by the first step the host chooses
    bool filter = false;
    uint32_t host_steps = 0;

    explicit KmppSeeding(Job &j)
        : job(j), shards(j.shards), verbosity(j.verbosity), dp((j.D + 127u) / 128u * 128u), kpp(j.shards.size()) {
      while ((1ull << log2n) < (uint64_t)job.N) log2n++;
    }
    ~KmppSeeding() {
      (void)hipSetDevice(shards[0]->dev);
      if (ev_chosen) (void)hipEventDestroy(ev_chosen);
      for (size_t q = 0; q < kpp.size(); q++) {
        (void)hipSetDevice(shards[q]->dev);
        if (kpp[q].ev_step) (void)hipEventDestroy(kpp[q].ev_step);
        kpp[q].filter_mem.reset();
      }
      if (fail_host) (void)hipHostFree(fail_host);
      if (host_dists) (void)hipHostFree(host_dists);
    }

    int run() {
      const bool device_chooser = device_chooser_possible();
      if (device_chooser) RETERR(alloc_chooser());
      RETERR(prepare_filter(device_chooser));
      RETERR(device_chooser ? run_device() : run_host());
      RETERR(job.sync_all());
      if (filter) report_chains();
      return 0;
    }

    // The device chooser needs whole 256-row blocks on every shard but the last (row_plan()) and peer access from the
    // first shard's device to the others'; otherwise the host chooser.
    bool device_chooser_possible() const {
      bool can_choose = !job.strict_h2 && !job.sw.kmpp_host && shards.size() <= (size_t)kKmppMaxShards;
      for (auto &s : shards) {
        can_choose = can_choose && kmpp_blocks(s->length) <= (1u << 20) &&   // (two-level prefix: 1024 x 1024 blocks of 256 rows)
                     (s->offset % 256u == 0u) && s->length != 0;
        if (can_choose && s->dev != shards[0]->dev) {
          int can = 0;
          (void)hipSetDevice(shards[0]->dev);
          if (hipDeviceCanAccessPeer(&can, shards[0]->dev, s->dev) != hipSuccess || !can) {
            can_choose = false;
          } else {
            const hipError_t pe = hipDeviceEnablePeerAccess(s->dev, 0);
            if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) can_choose = false;
          }
          (void)hipGetLastError();
        }
      }
      return can_choose;
    }

    // the chooser's buffers on every shard (small: the shard's slabs, alive until the job ends), the events that order
    // the shards' steps around the chooser, the pinned word the fail flag comes back in
    int alloc_chooser() {
      const bool many = shards.size() > 1;
      views.resize(shards.size());
      for (size_t q = 0; q < shards.size(); q++) {
        Shard &s = *shards[q];
        PerShard &k = kpp[q];
        (void)hipSetDevice(s.dev);
        RETERR(s.alloc(&k.block_stats, kmpp_block_stat_bytes(s.length)));
        RETERR(s.alloc(&k.totals, kmpp_totals_bytes()));
        RETERR(s.alloc(&k.bpre, kmpp_prefix_doubles(s.length)));
        RETERR(s.alloc(&k.fail, 4));
        RETERR(s.alloc(&k.outliers, kmpp_outlier_bytes()));
        k.out.ecut = k.fail + 1;
        k.out.outl_count = k.fail + 2;
        k.out.outl = k.outliers;
        if (hipMemsetAsync(k.fail, 0, 4 * sizeof(uint32_t), s.eng->stream_) != hipSuccess) return kmcudaRuntimeError;
        if (hipMemsetAsync(k.totals, 0, kmpp_totals_bytes(), s.eng->stream_) != hipSuccess) return kmcudaRuntimeError;
        if (many && hipEventCreateWithFlags(&k.ev_step, hipEventDisableTiming) != hipSuccess) return kmcudaRuntimeError;
        KmppShardPtrs &v = views[q];
        v.dists = job.weighted ? s.wterms : s.dists; v.bpre = k.bpre; v.totals = k.totals;
        v.samples = s.samples; v.centroids = s.centroids; v.fail = k.fail;
        v.offset = s.offset; v.length = s.length;
        v.out = k.out;
      }
      (void)hipSetDevice(shards[0]->dev);
      if (many && hipEventCreateWithFlags(&ev_chosen, hipEventDisableTiming) != hipSuccess) return kmcudaRuntimeError;
      if (hipHostMalloc(reinterpret_cast<void **>(&fail_host), sizeof(uint32_t), hipHostMallocDefault) != hipSuccess)
        return kmcudaMemoryAllocationFailure;
      return 0;
    }

    // Whether the steps are the filtered ones, and if so the byte copy of every shard's rows.  Needs DP + 20 bytes per
    // row beside the rows; without that memory on ANY shard (or KMCUDA_AMD_KMPP_FILTER=0) every step on every shard
    // is the plain one, and what was allocated is freed here and now.
    int prepare_filter(bool device_chooser) {
      // (small jobs: the plain step is a few launches of nothing; KMCUDA_AMD_KMPP_FILTER=2 filters them too: tests)
      filter = device_chooser && job.K >= 8 && job.N >= 65536u && dp <= 8192u;
      const int f = job.sw.kmpp_filter;
      filter = f >= 2 ? (device_chooser && job.K >= 3 && dp <= 8192u) : (filter && f != 0);
      if (!filter) return 0;
      bool ok = true;
      for (size_t q = 0; q < shards.size() && ok; q++) {
        Shard &s = *shards[q];
        PerShard &k = kpp[q];
        (void)hipSetDevice(s.dev);
        k.filter_mem.reset(new DeviceArena{s.dev});
        DeviceArena &mem = *k.filter_mem;
        ok = mem.alloc(&k.xs8, (size_t)s.length * dp) == 0 && mem.alloc(&k.n2c, (size_t)s.length * 4) == 0 &&
             mem.alloc(&k.mu, dp) == 0 && mem.alloc(&k.stats, 4) == 0 && mem.alloc(&k.list, s.length) == 0 &&
             mem.alloc(&k.part, (size_t)64 * job.D) == 0;
      }
      if (!ok) {
        (void)hipGetLastError();
        filter = false;
        for (auto &k : kpp) k.filter_mem.reset();   // (the events stay: they end with the seeding)
        DEBUG("k-means++: no memory for the byte copy of the rows, plain steps\n");
        return 0;
      }
      for (size_t q = 0; q < shards.size(); q++) {
        Shard &s = *shards[q];
        PerShard &k = kpp[q];
        (void)hipSetDevice(s.dev);
        if (launch_kmpp_cache(s.samples, s.length, job.D, dp, k.part, k.mu, k.xs8, k.n2c, k.stats, s.eng->stream_) != hipSuccess)
          return kmcudaRuntimeError;
      }
      return 0;
    }

    // Enqueues step t for the random number `choice`: every shard's distances to seed t - 1 with their statistics,
    // the chooser on the first shard's stream behind events of the others' steps, and the others' next steps behind
    // an event of the chooser (the events must be RECORDED before they are waited for: one thread, in order).
    int enqueue_step(uint32_t t, double choice) {
      Shard &lead = *shards[0];
      const bool many = shards.size() > 1;
      for (size_t q = 0; q < shards.size(); q++) {
        Shard &s = *shards[q];
        PerShard &k = kpp[q];
        (void)hipSetDevice(s.dev);
        hipStream_t st = s.eng->stream_;
        const float *newest = s.centroids + (size_t)(t - 1) * job.D;
        const hipError_t se =
            (filter && t >= 2)
                ? launch_kmpp_step_filtered(job.metric, s.samples, s.length, job.D, dp, k.xs8, k.n2c, k.mu, k.stats, k.list,
                                            newest, t, s.dists, k.block_stats, k.bpre, k.totals, k.fail, k.out, st,
                                            s.weights, s.wterms)
                : launch_kmpp_step2(job.metric, s.samples, s.length, job.D, newest, t, s.dists, k.block_stats, k.bpre,
                                    k.totals, k.fail, k.out, st, s.weights, s.wterms);
        if (se != hipSuccess) return kmcudaRuntimeError;
        if (many && q != 0 && hipEventRecord(k.ev_step, st) != hipSuccess) return kmcudaRuntimeError;
      }
      (void)hipSetDevice(lead.dev);
      for (size_t q = 1; q < shards.size(); q++)
        if (hipStreamWaitEvent(lead.eng->stream_, kpp[q].ev_step, 0) != hipSuccess) return kmcudaRuntimeError;
      if (launch_kmpp_choose(views.data(), (uint32_t)views.size(), job.N, choice, log2n, t, job.D, lead.eng->stream_) != hipSuccess)
        return kmcudaRuntimeError;
      if (many) {
        if (hipEventRecord(ev_chosen, lead.eng->stream_) != hipSuccess) return kmcudaRuntimeError;
        for (size_t q = 1; q < shards.size(); q++) {
          (void)hipSetDevice(shards[q]->dev);
          if (hipStreamWaitEvent(shards[q]->eng->stream_, ev_chosen, 0) != hipSuccess) return kmcudaRuntimeError;
        }
      }
      return 0;
    }

    // the reference's chooser on the host (kmcuda.cc:286-326) for step i with random number `choice`: all N
    // distances come back, butterfly sum, sequential double prefix sums; copies the seed
    int host_choose(uint32_t i, double choice) {
      const uint32_t N = job.N;
      host_steps++;
      if (!host_dists &&
          hipHostMalloc(reinterpret_cast<void **>(&host_dists), (size_t)N * sizeof(float), hipHostMallocDefault) != hipSuccess)
        return kmcudaMemoryAllocationFailure;
      for (auto &s : shards) {
        (void)hipSetDevice(s->dev);
        // (weighted: the terms w * d where the reference sums d)
        if (job.weighted && launch_kmpp_weigh(s->dists, s->weights, s->length, s->wterms, nullptr, s->eng->stream_) != hipSuccess)
          return kmcudaRuntimeError;
        if (hipMemcpyAsync(host_dists + s->offset, job.weighted ? s->wterms : s->dists, (size_t)s->length * sizeof(float),
                           hipMemcpyDeviceToHost, s->eng->stream_) != hipSuccess)
          return kmcudaMemoryCopyError;
      }
      RETERR(job.sync_all());
      const double dist_sum = butterfly_sum(host_dists, N);
      const uint32_t choice_approx = choice * N;
      const double choice_sum = choice * dist_sum;
      uint32_t j = 0;
      if (choice_approx < 100) {
        double dist_sum2 = 0;
        for (j = 0; j < N && dist_sum2 < choice_sum; j++) dist_sum2 += host_dists[j];
      } else {
        double dist_sum2 = 0;
        for (uint32_t t = 0; t < choice_approx; t++) dist_sum2 += host_dists[t];
        if (dist_sum2 < choice_sum) {
          for (j = choice_approx; j < N && dist_sum2 < choice_sum; j++) dist_sum2 += host_dists[j];
        } else {
          for (j = choice_approx; j > 1 && dist_sum2 >= choice_sum; j--) dist_sum2 -= host_dists[j];
          j++;
        }
      }
      if (j == 0 || j > N) {
        INFO("\ninternal bug in kmeans_init_centroids: j = %u\n", j);
        return kmcudaRuntimeError;
      }
      return job.copy_sample_to_centroid(j - 1, i);
    }

    // The host only draws the random numbers (one rand() per step, in order, as the reference) and enqueues:
    // distances, statistics, prefix sums, the chooser and the copy of the chosen row all run on the device
    // (seeding.hip).  A step the device cannot decide raises a flag that turns the rest of the enqueued kernels into
    // no-ops; the host looks after every batch of steps, chooses that seed the reference's way from the distances as
    // that step left them, lowers the flag and goes on behind it.
    int run_device() {
      Shard &lead = *shards[0];
      const bool many = shards.size() > 1;
      if (many) RETERR(job.sync_all());   // (the first seed's peer copies and the flags' memsets have landed everywhere)
      std::vector<double> choices(job.K, 0.0);
      // (steps enqueued behind an undecided one are wasted launches: the batch starts small, doubles while the
      //  device decides, and falls back to one step after a hand-over -- a data set whose distances span too many
      //  binades hands over every step)
      constexpr uint32_t kBatchMax = 256;
      uint32_t batch = 8, i = 1;
      uint32_t drawn = 1;   // choices[1 .. drawn) are drawn
      while (i < job.K) {
        const uint32_t end = i + batch < job.K ? i + batch : job.K;
        for (uint32_t t = i; t < end; t++) {
          job.seeding_progress(t);
          if (t >= drawn) {
            choices[t] = ((rand() + .0) / RAND_MAX);   // kmcuda.cc:300
            drawn = t + 1;
          }
          RETERR(enqueue_step(t, choices[t]));
        }
        (void)hipSetDevice(lead.dev);
        if (hipMemcpyAsync(fail_host, kpp[0].fail, sizeof(uint32_t), hipMemcpyDeviceToHost, lead.eng->stream_) != hipSuccess ||
            hipStreamSynchronize(lead.eng->stream_) != hipSuccess)
          return kmcudaMemoryCopyError;
        const uint32_t failed = *fail_host;
        if (failed == 0) {
          i = end;
          batch = batch * 2 < kBatchMax ? batch * 2 : kBatchMax;
          continue;
        }
        batch = 1;
        if (failed < i || failed >= end) return kmcudaRuntimeError;
        RETERR(host_choose(failed, choices[failed]));   // (waits for every shard: sync_all)
        for (size_t q = 0; q < shards.size(); q++) {
          (void)hipSetDevice(shards[q]->dev);
          if (hipMemsetAsync(kpp[q].fail, 0, sizeof(uint32_t), shards[q]->eng->stream_) != hipSuccess) return kmcudaRuntimeError;
        }
        if (many) RETERR(job.sync_all());   // (the seed's peer copies and the lowered flags, before the chooser reads across shards)
        i = failed + 1;
      }
      DEBUG("k-means++: %u of %u steps took the host chooser\n", host_steps, job.K - 1);
      return 0;
    }

    // every step: the plain distances on every shard, then the host chooser
    int run_host() {
      for (uint32_t i = 1; i < job.K; i++) {
        job.seeding_progress(i);
        for (auto &s : shards) {
          (void)hipSetDevice(s->dev);
          const float *newest = s->centroids + (size_t)(i - 1) * job.D;
          const hipError_t ke =
              job.strict_h2 ? launch_h2_to_row(job.metric, s->samples, s->length, job.D, newest, i, 0, s->dists, s->eng->stream_)
                            : launch_kmpp_step(job.metric, s->samples, s->length, job.D, newest, i, s->dists, s->eng->stream_);
          if (ke != hipSuccess) return kmcudaRuntimeError;
        }
        RETERR(host_choose(i, ((rand() + .0) / RAND_MAX)));
      }
      return 0;
    }

    void report_chains() {
      unsigned long long chains = 0;
      bool read = true;
      for (size_t q = 0; q < kpp.size(); q++) {
        unsigned long long v = 0;
        (void)hipSetDevice(shards[q]->dev);
        read = read && hipMemcpy(&v, kpp[q].stats + 2, sizeof(v), hipMemcpyDeviceToHost) == hipSuccess;
        chains += v;
      }
      if (read)
        DEBUG("k-means++: the filtered steps ran %llu exact chains for %llu (row, step) pairs\n", chains,
              (unsigned long long)job.N * (job.K - 2));
    }
  };

  int seed_plusplus() {
    uint32_t first_index = 0;
    RETERR(draw_first_seed(&first_index));
    RETERR(copy_sample_to_centroid(first_index, 0));
    INFO("performing kmeans++...\n");
    if (weighted)
      for (auto &s : shards)
        if (!s->wterms) RETERR(s->alloc(&s->wterms, s->length));
    KmppSeeding kpp(*this);
    return kpp.run();
  }

  int seed_afkmc2(uint32_t seed, uint32_t afk_m) {   // kmcuda.cc:337-396
    uint32_t m = afk_m;
    if (m == 0) {
      m = 200;
    } else if (m > N / 2) {
      INFO("afkmc2: m > %u is not supported (got %u)\n", N / 2, m);
      return kmcudaInvalidArguments;
    }
    uint32_t first_index = 0;
    RETERR(draw_first_seed(&first_index));
    INFO("afkmc2: calculating q (c0 = %u)... ", first_index / D);
    RETERR(copy_sample_to_centroid(first_index, 0));
    // the candidate kernels index rows globally: with several shards the rows are gathered on the first
    Shard &s0 = *shards[0];
    (void)hipSetDevice(s0.dev);
    hipStream_t st = s0.eng->stream_;
    const float *all = s0.samples;
    if (shards.size() > 1) {
      float *gathered = nullptr;
      RETERR(s0.alloc(&gathered, (size_t)N * D));
      RETERR(sync_all());
      for (auto &s : shards) {
        const hipError_t e = s->dev == s0.dev
            ? hipMemcpy(gathered + (size_t)s->offset * D, s->samples, (size_t)s->length * D * sizeof(float), hipMemcpyDeviceToDevice)
            : hipMemcpyPeer(gathered + (size_t)s->offset * D, s0.dev, s->samples, s->dev, (size_t)s->length * D * sizeof(float));
        if (e != hipSuccess) return kmcudaMemoryCopyError;
      }
      all = gathered;
    }
    float *qdev = nullptr, *rand_dev = nullptr, *mind_dev = nullptr;
    uint32_t *choice_dev = nullptr;
    RETERR(s0.alloc(&qdev, N));
    RETERR(s0.alloc(&rand_dev, m));
    RETERR(s0.alloc(&mind_dev, m));
    RETERR(s0.alloc(&choice_dev, m));
    if (hipMemsetAsync(choice_dev, 0, m * sizeof(uint32_t), st) != hipSuccess) return kmcudaRuntimeError;
    std::vector<float> q(N), rand_a(m), p_cand(m);
    std::vector<uint32_t> cand_ind(m);
    // q(x) = 1 / 2N + d(x, c1)^2 / (2 sum d^2), with c1 = sample (first_index / D): the reference
    // seeds q from THAT sample while centroid 0 is sample first_index (kmcuda.cc:356-362)
    if ((strict_h2 ? launch_h2_to_row(metric, all, N, D, all + (size_t)(first_index / D) * D, 0, 1, qdev, st)
                   : launch_afk_qdist(metric, all, N, D, all + (size_t)(first_index / D) * D, qdev, st)) != hipSuccess)
      return kmcudaRuntimeError;
    if (hipMemcpyAsync(q.data(), qdev, (size_t)N * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return kmcudaMemoryCopyError;
    const double dsum = butterfly_sum(q.data(), N);   // kmeans.cu:92-95 (warp sums, double accumulation)
    if (launch_afk_q(qdev, N, (float)dsum, st) != hipSuccess) return kmcudaRuntimeError;
    if (hipMemcpyAsync(q.data(), qdev, (size_t)N * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return kmcudaMemoryCopyError;
    INFO("done\n");
    for (uint32_t k = 1; k < K; k++) {
      seeding_progress(k);
      (void)hipSetDevice(s0.dev);
      if (launch_afk_random_step(m, seed, k, qdev, N, choice_dev, rand_dev, st) != hipSuccess ||
          (strict_h2 ? launch_h2_afk_min_dist(metric, m, k, all, D, choice_dev, s0.centroids, mind_dev, st)
                     : launch_afk_min_dist(metric, m, k, all, D, choice_dev, s0.centroids, mind_dev, st)) != hipSuccess)
        return kmcudaRuntimeError;
      if (hipMemcpyAsync(cand_ind.data(), choice_dev, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipMemcpyAsync(rand_a.data(), rand_dev, m * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipMemcpyAsync(p_cand.data(), mind_dev, m * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess)
        return kmcudaMemoryCopyError;
      float curr_prob = 0;   // the Metropolis-Hastings chain, kmcuda.cc:381-388
      uint32_t curr_ind = 0;
      for (uint32_t j = 0; j < m; j++) {
        const float cand_prob = p_cand[j] / q[cand_ind[j]];
        if (curr_prob == 0 || cand_prob / curr_prob > rand_a[j]) {
          curr_ind = j;
          curr_prob = cand_prob;
        }
      }
      RETERR(copy_sample_to_centroid(cand_ind[curr_ind], k));
    }
    return sync_all();
  }

  // runs fn(shard) for every shard -- on one host thread per shard when there are several, so that a
  // step that has to wait for its GPU (the first iterations' update reads an event count) does not hold
  // up the enqueueing for the other GPUs.  Returns the first non-zero code.
  int for_shards(const std::function<int(Shard &)> &fn) {
    if (shards.size() == 1) {
      (void)hipSetDevice(shards[0]->dev);
      return fn(*shards[0]);
    }
    if (workers.size() == 0) workers.start(shards.size());   // persistent: one thread per shard, for the job's lifetime
    const std::function<int(size_t)> each = [&](size_t i) {
      (void)hipSetDevice(shards[i]->dev);
      return fn(*shards[i]);
    };
    return workers.run(each);
  }

  // ---- the per-iteration collective: ONE all-reduce of [delta (fp64 K*D) | dcount K | counters 4] ----
  int allreduce_fused() {
    if (shards.size() == 1 && comms.empty()) return 0;
    const size_t len = reduce_len();   // (weighted: + the K cluster-weight deltas and the reassigned weight)
    if (!comms.empty()) {
      RETERR(collective_mark(true));
      if (rccl.GroupStart() != 0) return kmcudaRuntimeError;
      for (size_t i = 0; i < shards.size(); i++) {
        auto &s = shards[i];
        (void)hipSetDevice(s->dev);
        if (rccl.AllReduce(s->reduce, s->reduce, len, kNcclFloat64, kNcclSum, comms[i], s->eng->stream_) != 0)
          return kmcudaRuntimeError;
      }
      if (rccl.GroupEnd() != 0) return kmcudaRuntimeError;
      return collective_mark(false);
    }
    // several shards on ONE device (test hook KMCUDA_AMD_VIRTUAL_SHARDS): a fixed-order sum kernel on the first
    // shard's stream once every shard's buffer is written; the other streams go on when it is done.  No host wait:
    // the host loop is exercised exactly as with the real collective
    Shard &f = *shards[0];
    (void)hipSetDevice(f.dev);
    for (auto &s : shards) {
      if (hipEventRecord(s->ev_filled, s->eng->stream_) != hipSuccess) return kmcudaRuntimeError;
      if (s.get() != &f && hipStreamWaitEvent(f.eng->stream_, s->ev_filled, 0) != hipSuccess) return kmcudaRuntimeError;
    }
    RETERR(collective_mark(true));   // (behind the waits: the stand-in's own time, not the slowest shard's lag)
    if (launch_sum_buffers(reduce_ptrs_dev, (uint32_t)shards.size(), len, f.eng->stream_) != hipSuccess)
      return kmcudaRuntimeError;
    RETERR(collective_mark(false));
    if (hipEventRecord(ev_summed, f.eng->stream_) != hipSuccess) return kmcudaRuntimeError;
    for (auto &s : shards)
      if (s.get() != &f && hipStreamWaitEvent(s->eng->stream_, ev_summed, 0) != hipSuccess) return kmcudaRuntimeError;
    return 0;
  }

  // reference: check_changed, kmeans.cu:697-717.  Returns 1 to stop, 0 to go on, <0 error.
  // Reads the shards' device counters (one stream synchronisation per shard).
  int check_changed(int iter, float tolerance, bool print, uint32_t *passed_total = nullptr) {
    uint32_t overall_changed = 0, overall_passed = 0, pair_rows = 0, scan_rows = 0;
    for (auto &s : shards) {
      uint32_t c[4];
      if (s->eng->counters_read(c) != 0) return -kmcudaMemoryCopyError;
      overall_changed += c[0];
      overall_passed += c[2];
      scan_rows += c[1];
      pair_rows += c[3];
    }
    return judge_changed(iter, tolerance, print, overall_changed, overall_passed, pair_rows, scan_rows, passed_total);
  }

  // the same test from the REDUCED buffer's tail (the counters rode along in the iteration's all-reduce):
  // one 32-byte read on the first shard instead of a synchronisation per GPU
  int check_changed_reduced(int iter, float tolerance, bool print, uint32_t *passed_total = nullptr) {
    Shard &f = *shards[0];
    (void)hipSetDevice(f.dev);
    double tail[4], changed_w = 0.0;
    if (hipMemcpyAsync(tail, f.reduce + (size_t)K * D + K, sizeof(tail), hipMemcpyDeviceToHost, f.eng->stream_) != hipSuccess ||
        (weighted && hipMemcpyAsync(&changed_w, f.reduce + reduce_len() - 1, sizeof(double), hipMemcpyDeviceToHost,
                                    f.eng->stream_) != hipSuccess) ||
        hipStreamSynchronize(f.eng->stream_) != hipSuccess)
      return -kmcudaMemoryCopyError;
    return judge_changed(iter, tolerance, print, (uint32_t)tail[0], (uint32_t)tail[2], (uint32_t)tail[3], (uint32_t)tail[1],
                         passed_total, changed_w);
  }

  int judge_changed(int iter, float tolerance, bool print, uint32_t overall_changed, uint32_t overall_passed,
                    uint32_t pair_rows, uint32_t scan_rows, uint32_t *passed_total, double changed_weight = 0.0) {
    if (print && passed_total == nullptr)
      DEBUG("filter: %u rows settled by two exact chains, %u by a full exact scan\n", pair_rows, scan_rows);
    if (print && passed_total != nullptr)
      DEBUG("local filter: %u exact distances queued, %u wave flushes\n", pair_rows, scan_rows);
    if (passed_total) *passed_total = overall_passed;
    if (print) INFO("iteration %d: %u reassignments\n", iter, overall_changed);
    stamp(iter);
    for (auto &s : shards) s->eng->carry_policy_.note_changed(overall_changed);   // (how fast the run converges: engine.hpp)
    // (weighted: the reassigned weight against the total weight, in the same float arithmetic; the line above keeps
    //  reporting rows)
    if (weighted ? (float)changed_weight <= stop_threshold(tolerance) : overall_changed <= tolerance * N)
      return 1;  // counters are NOT zeroed on stop (kmeans.cu:707-709)
    for (auto &s : shards)
      if (s->eng->counters_reset(0) != 0) return -kmcudaRuntimeError;
    return 0;
  }

  // KMCUDA_AMD_TIMING: when the host learned an iteration's outcome (ms since the job was made; a measurement aid)
  const std::chrono::steady_clock::time_point born_ = std::chrono::steady_clock::now();
  void stamp(int iter) const {
    if (sw.timing)
      fprintf(stderr, "[timing]   iteration %d judged at %.3f ms\n", iter,
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - born_).count());
  }
  bool exact_update = false;  // KMCUDA_AMD_EXACT_UPDATE=1 or the strict half2 mode: the reference's serial Kahan chain (single shard)

  // The stop test of iteration `iter`, from where its numbers lie: the shards' counters under the strict update (no
  // reduce buffer) and for the unweighted test at the hand-over point (kmeans.cu:1058), otherwise the reduced buffer's
  // tail (weighted: the reassigned weight is in the stop iteration's reduced buffer, not in the counters)
  int judge(int iter, float tolerance, bool print, uint32_t *passed_total = nullptr, bool at_hand_over = false) {
    const bool from_counters = exact_update || (at_hand_over && !weighted);
    return from_counters ? check_changed(iter, tolerance, print, passed_total)
                         : check_changed_reduced(iter, tolerance, print, passed_total);
  }

  // the engines' carried-bounds flag, as kmamd_set_carry (engine.cpp) sets it: bounds left by earlier passes are void
  void set_carry(bool on) {
    for (auto &s : shards) {
      s->eng->carry_on_ = on;
      s->eng->carry_valid_ = false;
    }
  }
  // Default schedule: iteration number from which on a judged "goes on" starts the carried bounds (0: no such
  // start pending; carried_phase sets it at the hand-over point)
  int carry_after = 0;
  void maybe_start_carry(int judged_iter) {
    if (carry_after == 0 || judged_iter < carry_after) return;
    carry_after = 0;
    INFO("carrying per-sample distance bounds from pass to pass\n");
    set_carry(true);
  }

  // the update in three stream-ordered phases (reference: kmeans_adjust launch + peer exchange,
  // kmeans.cu:1002-1024): fill every shard's reduce buffer, ONE all-reduce, apply on every shard
  int fill_deltas() {
    const uint32_t kd = K * D;
    return for_shards([kd](Shard &s) {
      return s.eng->move_deltas(s.samples, s.prev, s.assignments, s.reduce, nullptr, s.reduce + kd);
    });
  }
  // stop_threshold >= 0: every shard's apply kernel evaluates the stop rule itself from the reduced counters (the
  // same words on every shard) and leaves everything untouched when it fires; report: the first shard's kernel
  // reports the outcome to its engine's pinned words (Engine::stop_report(seq) reads them)
  int apply_deltas(float stop_threshold = -1.f, bool report = false, uint32_t seq = 0) {
    const uint32_t kd = K * D;
    for (size_t i = 0; i < shards.size(); i++) {
      auto &s = shards[i];
      // (the next pass's centroid preparation rides in the same launch where it can: Engine::apply_prepare;
      // fp16x2 rounds the centroids to halves first, so there it cannot)
      if (fp16)
        RETERR(s->eng->apply_delta(s->reduce, nullptr, s->reduce + kd, s->centroids, s->ccounts, stop_threshold,
                                   report && i == 0, seq));
      else
        RETERR(s->eng->apply_prepare(s->reduce, s->reduce + kd, s->centroids, s->ccounts, stop_threshold,
                                     report && i == 0, seq));
    }
    return quantize_centroids();
  }

  int adjust() {
    if (exact_update) {
      Shard &s = *shards[0];
      RETERR(s.eng->adjust_exact(s.samples, s.prev, s.assignments, s.centroids, s.ccounts));
      return quantize_centroids();
    }
    RETERR(fill_deltas());
    RETERR(allreduce_fused());
    return apply_deltas();
  }

  // fp16x2: the reference keeps centroids in half2, i.e. every update is rounded to half
  int quantize_centroids() {
    if (!fp16) return 0;
    for (auto &s : shards) {
      (void)hipSetDevice(s->dev);
      if (launch_quantize_half(s->centroids, (size_t)K * D, s->eng->stream_) != hipSuccess) return kmcudaRuntimeError;
    }
    return 0;
  }

  // reference: prepare_mem, kmeans.cu:719-746
  int prepare_mem(bool resume) {
    for (auto &s : shards) {
      (void)hipSetDevice(s->dev);
      RETERR(s->eng->counters_reset(0));
      if (!resume) {
        hipStream_t st = s->eng->stream_;
        if (hipMemsetAsync(s->ccounts, 0, K * sizeof(uint32_t), st) != hipSuccess) return kmcudaRuntimeError;
        if (hipMemsetAsync(s->assignments, 0xff, (size_t)s->length * sizeof(uint32_t), st) != hipSuccess)
          return kmcudaRuntimeError;
        if (hipMemsetAsync(s->prev, 0xff, (size_t)s->length * sizeof(uint32_t), st) != hipSuccess)
          return kmcudaRuntimeError;
      }
    }
    return 0;
  }

  // reference: kmeans_cuda_lloyd, kmeans.cu:934-1026.  Per iteration: assignment on every shard, the
  // shards' move sums, ONE all-reduce that also carries the reassignment counters, the stop test on the
  // reduced counters (before the update, as kmeans.cu:991-1000), the update.
  //
  // The stop test is decided ON THE DEVICE by the update kernel (update.hip: apply_delta_kernel + StopCtl), so
  // the host enqueues iteration i + 1 before it has seen iteration i's count: the GPUs never wait for the 32-byte
  // round trip (on a 1M-row shard it is worth several percent of an iteration).  When the rule fires the update
  // kernel leaves everything untouched and raises a device flag that turns the already-enqueued next pass into
  // no-ops, so the state is exactly what the reference returns (assignments of the stop iteration, centroids one
  // update behind); the host reads the outcome one iteration late from pinned words and prints the same lines.
  //   leave:  asked after every iteration that goes on; true = "return BEFORE the next update" (the caller wants
  //           to start Yinyang from the reference's hand-over state).  It takes effect one iteration later: that
  //           iteration is judged by the host before its update, as in the reference.
  //   *left:  the loop returned for `leave`, not for the stop rule
  using LeaveFn = std::function<bool(int iter, uint32_t changed)>;
  //   after:  0 = a fresh run.  > 0: carry on after iteration `after`, whose stop test said "go on" and whose
  //           (reduced) move sums still sit in the reduce buffers: its update first, then iteration after + 1
  int lloyd(float tolerance, int *iterations, const LeaveFn *leave = nullptr, bool *left = nullptr, int after = 0) {
    if (after == 0) RETERR(prepare_mem(false));
    if (left) *left = false;
    // the samples do not change inside one kmeans_cuda() call: let the coarse filter stage keep its
    // centred half copy of the rows across the iterations (kmamd_set_row_cache, include/kmcuda_amd.h)
    for (auto &s : shards) {
      if (after == 0) {
        s->eng->row_cache_on_ = s->eng->row_cache_allowed_;
        s->eng->row_cache_valid_ = false;
      }
      RETERR(s->eng->stop_clear());
    }
    if (exact_update) {   // strict-parity mode: the reference's sequence, step by step
      if (after) RETERR(adjust());
      for (int iter = after + 1;; iter++) {
        for (auto &s : shards)
          RETERR(s->eng->lloyd_assign(s->samples, s->centroids, s->assignments, s->prev, false));
        const int status = judge(iter, tolerance, true);
        if (status < 0) return -status;
        stats.iterations++;
        if (status == 1) {
          if (iterations) *iterations = iter;
          return 0;
        }
        maybe_start_carry(iter);
        RETERR(adjust());
      }
    }
    const float threshold = stop_threshold(tolerance);   // the float product of kmeans.cu:707 (weighted: of the total weight)
    bool leave_next = false;
    int unjudged = 0;   // a speculative iteration whose outcome the host has not looked at yet
    if (after) {
      for (auto &s : shards) RETERR(s->eng->counters_reset(0));   // (the stop that ended the last run left it, kmeans.cu:707-709)
      RETERR(apply_deltas());
    }
    for (int iter = after + 1;; iter++) {
      const bool spec = speculate && !leave_next;
      RETERR(for_shards([](Shard &s) {
        const int rc = s.eng->lloyd_assign(s.samples, s.centroids, s.assignments, s.prev, false);
        if (rc) return rc;
        const uint32_t kd = s.eng->K_ * s.eng->D_;
        return s.eng->move_deltas(s.samples, s.prev, s.assignments, s.reduce, nullptr, s.reduce + kd);
      }));
      RETERR(allreduce_fused());
      if (spec) RETERR(apply_deltas(threshold, true, (uint32_t)iter));
      if (unjudged) {
        uint32_t changed = 0;
        const int status = judge_reported(unjudged, &changed);
        if (status < 0) return -status;
        if (status == 1) {   // the pass enqueued above found the flag raised: nothing was touched
          if (iterations) *iterations = unjudged;
          return 0;
        }
        if (leave && (*leave)(unjudged, changed)) leave_next = true;
        maybe_start_carry(unjudged);   // (the run has gone on past iteration `unjudged`)
        unjudged = 0;
      }
      if (spec) {
        unjudged = iter;
        continue;
      }
      const int status = judge(iter, tolerance, true);   // the host waits: one 32-byte read
      if (status < 0) return -status;
      stats.iterations++;
      if (status == 1 || leave_next) {
        if (left) *left = status != 1;
        if (iterations) *iterations = iter;
        return 0;
      }
      maybe_start_carry(iter);
      RETERR(apply_deltas(threshold));   // (the same decision once more on the device; zeroes the counter)
    }
  }

  // the outcome of speculative iteration `iter`, as the first shard's update kernel reported it.  1: stopped, 0: went on
  int judge_reported(int iter, uint32_t *changed) {
    uint32_t t[6];
    if (shards[0]->eng->stop_report((uint32_t)iter, t) != 0) {
      INFO("internal error: no report of iteration %d\n", iter);
      return -kmcudaRuntimeError;
    }
    DEBUG("filter: %u rows settled by two exact chains, %u by a full exact scan\n", t[3], t[1]);
    INFO("iteration %d: %u reassignments\n", iter, t[0]);
    stamp(iter);
    if (changed) *changed = t[0];
    for (auto &s : shards) s->eng->carry_policy_.note_changed(t[0]);
    stats.iterations++;
    return t[4] ? 1 : 0;
  }

  // ---- Yinyang (reference: kmeans_cuda_yy, kmeans.cu:1028-1263) ----
  // Clusters the K centroids into G groups: k-means++ (srand(0), kmeans.cu:1081-1084 passes seed 0)
  // followed by Lloyd at YINYANG_GROUP_TOLERANCE on the centroids themselves (kmeans.cu:1062-1100).
  // Runs as a nested single-GPU job whose "samples" are shard 0's centroid replica.
  int cluster_groups(uint32_t G, std::vector<uint32_t> *groups) {
    Shard &first = *shards[0];
    RETERR(first.eng->sync());
    PhaseClock clock(sw.timing);   // (its laps wait for nothing: the waits are the code's own)
    Job gjob;
    gjob.strict_h2 = strict_h2;   // (before setup: the engines take the flag there, and the strict update follows it)
    std::vector<int> one{first.dev};
    RETERR(gjob.setup(sw, one, 0, K, D, G, metric, verbosity, first.centroids, first.dev, first.eng->stream_));  // fp32 replica in place
    gjob.shards[0]->eng->side_stream_ = first.eng->side_stream_;   // (borrowed with the main one; may be null)
    clock.lap("group clustering, setup");
    gjob.fp16 = fp16;  // centroids_yy is half2 in the reference too (kmeans.cu:1084-1091)
    RETERR(gjob.init_centroids(kmcudaInitMethodPlusPlus, 0, nullptr, first.dev));
    if (sw.timing) RETERR(gjob.sync_all());
    clock.lap("group clustering, k-means++");
    RETERR(gjob.lloyd((float)kYinyangGroupTolerance, nullptr));
    RETERR(gjob.sync_all());
    clock.lap("group clustering, Lloyd");
    groups->resize(K);
    (void)hipSetDevice(first.dev);
    if (hipMemcpy(groups->data(), gjob.shards[0]->assignments, K * sizeof(uint32_t), hipMemcpyDeviceToHost) !=
        hipSuccess)
      return kmcudaMemoryCopyError;
    return 0;
  }

  // rand() as cluster_groups() leaves it: srand(0) (kmeans.cu:1081-1084 passes seed 0 to the nested k-means++), the
  // draws for its first seed -- a centroid whose first feature is not NaN, kmcuda.cc:265-270 -- and one draw per further
  // seed (kmcuda.cc:300)
  int replay_group_seeding_draws(uint32_t G) {
    Shard &first = *shards[0];
    srand(0);
    float smoke = NAN;
    while (smoke != smoke) {
      const uint32_t idx = rand() % K;
      (void)hipSetDevice(first.dev);
      RETERR(first.eng->sync());
      if (hipMemcpy(&smoke, first.centroids + (size_t)idx * D, sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
        return kmcudaMemoryCopyError;
    }
    for (uint32_t t = 1; t < G; t++) (void)rand();
    return 0;
  }

  int yinyang(float tolerance, uint32_t G, int iter, const std::vector<uint32_t> &groups) {
    for (auto &s : shards) {
      (void)hipSetDevice(s->dev);
      RETERR(s->eng->stop_clear());   // (the Lloyd phase's stop raised it; this phase decides on the host)
      RETERR(s->eng->yy_configure(G, groups.data()));
      int rc;
      if ((rc = s->alloc(&s->bounds, (size_t)s->length * (G + 1)))) return rc;
      if ((rc = s->alloc(&s->drifts, (size_t)K * D + K))) return rc;
      if ((rc = s->alloc(&s->gdrifts, G))) return rc;
      if ((rc = s->alloc(&s->passed, s->length))) return rc;
    }
    RETERR(sync_all());  // host vectors above go out of use
    RETERR(prepare_mem(true));
    bool refresh = true;
    // Per iteration (kmeans.cu:1112-1260): stop test on the filters' counters, bounds refresh when nearly every row
    // passed, the update, the drifts, the two filters.  With several shards the counters (reassigned, passed) ride
    // in the update's ONE all-reduce -- the shards' move sums are formed and reduced BEFORE the test, which then is
    // one 32-byte read on the first shard instead of a stream synchronisation per GPU (round 3: check_changed) --
    // and every shard's kernels are enqueued by its own worker thread (for_shards), as in lloyd().  The strict
    // update (one serial chain over all rows, single shard) has no reduce buffer and keeps the plain sequence.
    for (;; iter++) {
      if (!exact_update) {
        RETERR(fill_deltas());
        RETERR(allreduce_fused());
      }
      if (!refresh) {
        uint32_t passed_total = 0;
        const int status = judge(iter, tolerance, true, &passed_total);
        if (status < 0) return -status;
        if (status == 1) {
          if (verbosity > 1) {
            for (auto &s : shards) {
              uint32_t hs[6] = {0, 0, 0, 0, 0, 0};
              (void)hipSetDevice(s->dev);
              if (s->eng->yy_hint_stats(hs) == 0 && hs[0])
                printf("local filter with the second-best estimate: %u rows, %u of them handed to the plain kernel "
                       "(no estimate %u, bound not holding %u, candidate bound %u, second minimum %u)\n",
                       hs[0], hs[1], hs[2], hs[3], hs[4], hs[5]);
            }
          }
          return 0;
        }
        DEBUG("passed number: %u\n", passed_total);
        if (1.f - (passed_total + 0.f) / N < kYinyangRefreshEpsilon) refresh = true;  // kmeans.cu:1136-1138
      }
      if (refresh) {
        INFO("refreshing Yinyang bounds...\n");
        RETERR(for_shards([](Shard &s) { return s.eng->yy_init(s.samples, s.centroids, s.assignments, s.bounds); }));
        refresh = false;
      }
      const size_t kd_bytes = (size_t)K * D * sizeof(float);
      RETERR(for_shards([kd_bytes](Shard &s) {   // kmeans.cu:1159: keep the old centroids for the drifts
        return hipMemcpyAsync(s.drifts, s.centroids, kd_bytes, hipMemcpyDeviceToDevice, s.eng->stream_) == hipSuccess
                   ? 0 : (int)kmcudaMemoryCopyError;
      }));
      if (exact_update) RETERR(adjust());
      else RETERR(apply_deltas());
      RETERR(for_shards([](Shard &s) {
        int rc = s.eng->yy_drifts(s.centroids, s.drifts, s.gdrifts);
        if (rc) return rc;
        if ((rc = s.eng->counters_reset(2))) return rc;  // d_passed_number = 0, kmeans.cu:1225-1229
        if ((rc = s.eng->counters_reset(1))) return rc;  // statistics of the local filter (flushes, exact distances)
        if ((rc = s.eng->counters_reset(3))) return rc;
        return s.eng->yy_filters(s.samples, s.centroids, s.drifts, s.gdrifts, s.assignments, s.prev, s.bounds, s.passed);
      }));
      stats.iterations++;
    }
  }

  // ---- the schedule ----
  // The reference hands over from Lloyd to its bounds at 11 % reassignments whatever the data; its bounds refresh
  // (kmeans_yy_init: >= G exact chains per row) costs 38 assignment passes on this hardware and its filters more than a
  // pass per row that passes them (profiles/r2n_*, r3y_*): measured on both benchmark data sets it never pays.  The
  // default keeps the reference's sequence up to and including the hand-over point (group clustering, its progress
  // lines, its srand(0)) and then goes on with assignment passes that CARRY per-row bounds from pass to pass at no
  // refresh cost (lloyd_carry.hip).  Every pass either way is the reference's arithmetic.
  SchedulePlan plan_schedule(float tolerance, uint32_t yy_groups) const {
    using Yy = KmeansSwitches::Yy;
    using Carry = KmeansSwitches::Carry;
    SchedulePlan p;
    if (yy_groups == 0) p.lloyd_only = SchedulePlan::LloydOnly::too_few_clusters;   // kmeans.cu:1037-1050
    else if (kYinyangDraftReassignments <= tolerance) p.lloyd_only = SchedulePlan::LloydOnly::tolerance_too_high;
    if (p.lloyd_only != SchedulePlan::LloydOnly::no) return p;
    const Engine &e = *shards[0]->eng;
    const bool wide = e.DP_ == 0 && e.wide_dp_ != 0;   // D > 256: lloyd_wide.hip
    // KMCUDA_AMD_YY=reference: the reference's fixed schedule (Lloyd down to 11 % reassignments, then its bounds).
    // The strict parity modes keep the reference's schedule -- but KMCUDA_AMD_YY=carry: the default schedule also under
    // the strict update -- every pass is the reference's Lloyd arithmetic, so the whole call then equals the
    // reference's kmeans_cuda_lloyd bit for bit: the parity test of the carried bounds against the oracle end to end,
    // tests/test_gpu_carry.py.  The last term: the passes that carry bounds are the two-stage f16 filter's and the
    // streamed filter's (engine.cpp: carry_begin); a job on another filter keeps the reference's schedule.
    p.adaptive = sw.yy != Yy::reference && (!exact_update || (sw.yy == Yy::carry && !strict_h2)) &&
                 ((e.DP_ != 0 && e.filter_mode_ == 0) || wide);
    // (rows wider than 256 features: the streamed filter carries the bounds itself, up to 4096 features)
    p.carry = p.adaptive && sw.carry != Carry::off && (!wide || e.wide_dp_ <= 4096u);
    // The first carried pass only LEAVES bounds (and allocates them: 24 bytes per row); rows are spared from the
    // second one on.  A run that stops within a pass or two of the hand-over point never earns that back (round 4:
    // the 4M-row mixture at tolerance 0.01, one iteration after the hand-over, +12-16 %), and how long a run will
    // last cannot be read off its first counts (they fall by a factor of 4-8 per iteration, the tail by 1.1: an
    // extrapolation tried in round 5 switched the bounds off for the 37-iteration run,
    // profiles/r5e_configs_carry_extrapolation_rule_misfires.log).  So the bounds start once the host has SEEN the
    // run go on past an iteration after the hand-over (lloyd(), carry_after).  KMCUDA_AMD_CARRY=1: at once
    // (tests: every pass after the hand-over is then a carried one).
    p.carry_at_once = p.carry && sw.carry == Carry::on;
    // The groups are only ever USED by the reference's bounds (KMCUDA_AMD_YY=reference / the forced switch).  What a
    // caller can observe of their clustering besides -- its progress lines, and the C library's rand() state after
    // its srand(0) and draws -- is kept either way: a silent call (verbosity 0) that will not use the groups only
    // replays the draws (13 ms -> 0.05 ms at K = 1024, G = 102).
    p.cluster_groups_for_real = !p.adaptive || sw.hand_over_forced() || verbosity > 0;
    return p;
  }

  // Everything between seeding and the outputs.  `clock`: the entry point's laps.
  int run(float tolerance, uint32_t yy_groups, PhaseClock &clock) {
    const SchedulePlan plan = plan_schedule(tolerance, yy_groups);
    if (plan.lloyd_only != SchedulePlan::LloydOnly::no) {
      if (plan.lloyd_only == SchedulePlan::LloydOnly::too_few_clusters) INFO("too few clusters for this yinyang_t => Lloyd\n");
      else INFO("tolerance is too high (>= %.2f) => Lloyd\n", kYinyangDraftReassignments);
      return lloyd(tolerance, nullptr);
    }
    int iter = 0;
    RETERR(draft_lloyd(&iter));
    clock.lap("Lloyd down to 11 %% reassignments");
    const int st = judge(iter, tolerance, false, nullptr, true);   // kmeans.cu:1058
    if (st < 0) return -st;
    if (st == 1) return 0;
    // the reference's hand-over point: the K centroids are clustered into groups here (its progress lines are
    // part of what a caller sees, its srand(0) of what a caller's rand() sees) -- whichever schedule follows
    std::vector<uint32_t> groups;
    RETERR(hand_over_groups(plan, yy_groups, &groups));
    clock.lap("group clustering, whole");
    bool bounds = !plan.adaptive;
    if (plan.adaptive) {
      RETERR(carried_phase(plan, tolerance, &iter, &bounds));
      clock.lap("Lloyd after the hand-over point");
    }
    if (bounds) {
      RETERR(yinyang(tolerance, yy_groups, iter, groups));
      clock.lap("Yinyang");
    }
    return 0;
  }

  int draft_lloyd(int *iter) {
    INFO("running Lloyd until reassignments drop below %u\n", (uint32_t)(kYinyangDraftReassignments * N));
    return lloyd((float)kYinyangDraftReassignments, iter);
  }

  int hand_over_groups(const SchedulePlan &plan, uint32_t yy_groups, std::vector<uint32_t> *groups) {
    return plan.cluster_groups_for_real ? cluster_groups(yy_groups, groups) : replay_group_seeding_draws(yy_groups);
  }

  // The default schedule behind the hand-over point: Lloyd goes on from iteration *iter, whose update is still due,
  // with or without carried bounds.  *bounds: the run left for the reference's bounds (KMCUDA_AMD_YY_SWITCH), not
  // for the stop rule.  The engines' carry flags and carry_after are this phase's: set here, cleared here.
  int carried_phase(const SchedulePlan &plan, float tolerance, int *iter, bool *bounds) {
    INFO(plan.carry_at_once ? "Lloyd goes on, carrying per-sample distance bounds from pass to pass\n" : "Lloyd goes on\n");
    set_carry(plan.carry_at_once);
    carry_after = (plan.carry && !plan.carry_at_once) ? *iter + 1 : 0;
    const LeaveFn leave = [this](int, uint32_t changed) { return sw.hand_over_now(changed, N); };
    RETERR(lloyd(tolerance, iter, sw.hand_over_forced() ? &leave : nullptr, bounds, *iter));
    if (plan.carry && verbosity > 1) {
      unsigned long long spared = 0, paired = 0;
      for (auto &s : shards) {
        unsigned long long v = 0;
        if (s->eng->carry_stats(&v, nullptr) == 0) spared += v;
        if (s->eng->carry_pair_stats(&v) == 0) paired += v;
      }
      printf("carried bounds: %llu sample passes decided without looking at the sample\n", spared);
      if (paired) printf("carried pairs: %llu sample passes settled between two carried contenders\n", paired);
    }
    set_carry(false);
    carry_after = 0;
    return 0;
  }

  int gather_outputs(float *centroids, uint32_t *assignments, int32_t device_ptrs) {
    RETERR(sync_all());
    Shard &first = *shards[0];
    (void)hipSetDevice(first.dev);
    const void *cen_src = first.centroids;
    size_t cen_bytes = (size_t)K * D * sizeof(float);
    if (fp16) {  // K x D halves out
      uint16_t *hbuf = nullptr;
      int rc = first.alloc(&hbuf, (size_t)K * D);
      if (rc) return rc;
      if (launch_float_to_half(first.centroids, (size_t)K * D, hbuf, first.eng->stream_) != hipSuccess ||
          hipStreamSynchronize(first.eng->stream_) != hipSuccess)
        return kmcudaRuntimeError;
      cen_src = hbuf;
      cen_bytes = (size_t)K * D * sizeof(uint16_t);
    }
    if (device_ptrs < 0) {
      if (hipMemcpy(centroids, cen_src, cen_bytes, hipMemcpyDeviceToHost) != hipSuccess)
        return kmcudaMemoryCopyError;
      for (auto &s : shards) {
        (void)hipSetDevice(s->dev);
        if (hipMemcpy(assignments + s->offset, s->assignments, (size_t)s->length * sizeof(uint32_t),
                      hipMemcpyDeviceToHost) != hipSuccess)
          return kmcudaMemoryCopyError;
      }
    } else {
      if (hipMemcpyPeer(centroids, device_ptrs, cen_src, first.dev, cen_bytes) != hipSuccess)
        return kmcudaMemoryCopyError;
      for (auto &s : shards)
        if (hipMemcpyPeer(assignments + s->offset, device_ptrs, s->assignments, s->dev,
                          (size_t)s->length * sizeof(uint32_t)) != hipSuccess)
          return kmcudaMemoryCopyError;
    }
    return 0;
  }

  // reference: kmeans_cuda_calc_average_distance, kmeans.cu:1265-1300
  int average_distance(float *out) {
    INFO("calculating the average distance...\n");
    std::vector<float> host(N);
    for (auto &s : shards) {
      (void)hipSetDevice(s->dev);
      if ((strict_h2 ? launch_h2_member(metric, s->samples, s->length, D, s->centroids, s->assignments, K, s->dists,
                                        s->eng->stream_)
                     : launch_member_distances(metric, s->samples, s->length, D, s->centroids, s->assignments, K, s->dists,
                                               s->eng->stream_)) != hipSuccess)
        return kmcudaRuntimeError;
      // (weighted: sum(w d) / sum(w) -- the terms w * d, rounded to fp32, through the same sums)
      if (weighted && launch_kmpp_weigh(s->dists, s->weights, s->length, s->dists, nullptr, s->eng->stream_) != hipSuccess)
        return kmcudaRuntimeError;
      if (hipMemcpyAsync(host.data() + s->offset, s->dists, (size_t)s->length * sizeof(float), hipMemcpyDeviceToHost,
                         s->eng->stream_) != hipSuccess)
        return kmcudaMemoryCopyError;
    }
    RETERR(sync_all());
    *out = weighted ? (float)(butterfly_sum(host.data(), N) / weight_total) : (float)(butterfly_sum(host.data(), N) / N);
    return 0;
  }
};


// Once per process and device: the iteration kernels' code objects are loaded by a helper thread while the calling
// thread uploads the rows and seeds (they would otherwise load one by one in front of the first iteration: 24 ms of a
// 45-ms call on 4M rows).  Fire and forget: a launch that needs a code object the helper is still loading waits for it
// inside the runtime; the caller joins the helper before it returns (never a thread inside the runtime at process
// exit).  KMCUDA_AMD_PRELOAD=0: off (A/B).
struct PreloadThreads {
  std::vector<std::thread> threads;
  ~PreloadThreads() {
    for (auto &t : threads)
      if (t.joinable()) t.join();
  }
};
void preload_code_objects(int dev, PreloadThreads *keep, const KmeansSwitches &sw) {
  static std::mutex m;
  static std::vector<bool> done;
  {
    std::lock_guard<std::mutex> lock(m);
    if (done.size() <= (size_t)dev) done.resize(dev + 1, false);
    if (done[dev]) return;
    done[dev] = true;
  }
  if (!sw.preload) return;
  keep->threads.emplace_back([dev] {
    if (hipSetDevice(dev) != hipSuccess) return;
    (void)preload_update_code();
    (void)preload_lloyd_f16_code();
    (void)preload_lloyd_code();
    (void)preload_lloyd_carry_code();
    (void)preload_lloyd_duo_code();
    (void)hipGetLastError();
  });
}

int virtual_shards() { return kmeans_switches().virtual_shards; }   // (knn_cuda(): the one switch it shares)

// the reference's device-mask test (kmcuda.cc:37-41, :553-557)
bool device_mask_refused(uint32_t device) {
  int ndev = 0;
  (void)hipGetDeviceCount(&ndev);
  return ndev < 32 && device > (1u << ndev);
}

// device-pointer inputs: whatever the caller still has in flight on that GPU (any stream) must have
// landed before our own non-blocking streams read it -- the reference got this from the legacy
// default stream's implicit synchronisation
void sync_callers_device(int32_t device_ptrs) {
  if (device_ptrs >= 0 && hipSetDevice(device_ptrs) == hipSuccess) (void)hipDeviceSynchronize();
}

// reference: check_kmeans_args, kmcuda.cc:19-61 (same order), then what sample weights refuse -- all of it before any
// device is touched
int check_kmeans_args(const KmeansSwitches &sw, KMCUDAInitMethod init, float tolerance, float yinyang_t,
                      uint32_t samples_size, uint16_t features_size, uint32_t clusters_size, uint32_t device,
                      int32_t fp16x2, int32_t verbosity, const float *samples, const float *centroids,
                      const uint32_t *assignments, const float *sample_weights) {
  if (clusters_size < 2 || clusters_size == UINT32_MAX) return kmcudaInvalidArguments;
  if (features_size == 0) return kmcudaInvalidArguments;
  if (samples_size < clusters_size) return kmcudaInvalidArguments;
  if (device_mask_refused(device)) return kmcudaNoSuchDevice;
  if (samples == nullptr || centroids == nullptr || assignments == nullptr) return kmcudaInvalidArguments;
  if (tolerance < 0 || tolerance > 1) return kmcudaInvalidArguments;
  if (yinyang_t < 0 || yinyang_t > 0.5) return kmcudaInvalidArguments;
  if (!sample_weights) return kmcudaSuccess;
  // what restates the reference's own arithmetic has no weighted counterpart
  if (init == kmcudaInitMethodAFKMC2 || sw.exact_update || (fp16x2 && sw.fp16_strict)) {
    INFO("sample weights are not supported with afkmc2, KMCUDA_AMD_EXACT_UPDATE=1 or KMCUDA_AMD_FP16_STRICT=1\n");
    return kmcudaInvalidArguments;
  }
  if (init == kmcudaInitMethodParallel) {   // (weighted k-means|| does not exist: refused as afkmc2)
    INFO("sample weights are not supported with k-means||\n");
    return kmcudaInvalidArguments;
  }
  return kmcudaSuccess;
}

// init = k-means|| (seed_par_job.cpp): the stand-alone seeding writes `centroids` on the first device of the mask (the
// rows' own device in device-pointer mode), and the call goes on exactly as with imported centroids: *init becomes
// Import.  Host rows are uploaded twice, once by the seeding and once by the job.  Any other method: nothing happens.
int seed_parallel_first(KMCUDAInitMethod *init, const void *init_params, KMCUDADistanceMetric metric,
                        uint32_t samples_size, uint16_t features_size, uint32_t clusters_size, uint32_t seed,
                        int first_device, int32_t device_ptrs, int32_t fp16x2, int32_t verbosity, const float *samples,
                        float *centroids) {
  if (*init != kmcudaInitMethodParallel) return kmcudaSuccess;
  const auto *sp = static_cast<const kmamd_seed_parallel_params *>(init_params);
  INFO("performing k-means||...\n");
  RETERR(kmamd_kmeans_seed_parallel(metric, samples_size, fp16x2 ? (uint16_t)(2u * features_size) : features_size,
                                    clusters_size, sp ? sp->rounds : 0u, sp ? sp->oversampling : 0.f, seed,
                                    device_ptrs >= 0 ? device_ptrs : first_device, device_ptrs, fp16x2, verbosity, samples,
                                    centroids, nullptr, nullptr, 0, nullptr, nullptr, nullptr));
  kmx::g_verbosity = verbosity;
  *init = kmcudaInitMethodImport;
  return kmcudaSuccess;
}

// the run's statistics for kmamd_last_run_stats / kmamd_last_run_collective, once the loops are over
void publish_run_stats(Job &job, std::chrono::steady_clock::time_point t_loop) {
  job.stats.loop_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_loop).count();
  job.collective_collect();
  if (job.sw.update_trace)   // (a measurement aid: which way the updates went; nothing is printed inside the loop)
    for (auto &s : job.shards)
      fprintf(stderr, "[update] shard on device %d: %u radix, %u direct; loop %.4f s\n", s->dev, s->eng->ms_.n_radix, s->eng->ms_.n_direct,
              job.stats.loop_seconds);
  std::lock_guard<std::mutex> lock(g_last_run_mutex);
  g_last_run = job.stats;
}

}  // namespace

extern "C" {

KMCUDAResult kmeans_cuda(KMCUDAInitMethod init, const void *init_params, float tolerance, float yinyang_t,
                         KMCUDADistanceMetric metric, uint32_t samples_size, uint16_t features_size,
                         uint32_t clusters_size, uint32_t seed, uint32_t device, int32_t device_ptrs, int32_t fp16x2,
                         int32_t verbosity, const float *samples, float *centroids, uint32_t *assignments,
                         float *average_distance) {
  return static_cast<KMCUDAResult>(kmamd_kmeans_weighted(init, init_params, tolerance, yinyang_t, metric, samples_size,
                                                         features_size, clusters_size, seed, device, device_ptrs, fp16x2,
                                                         verbosity, samples, centroids, assignments, average_distance,
                                                         nullptr));
}

// kmeans_cuda() with per-row sample weights (include/kmcuda_amd.h); sample_weights == nullptr: kmeans_cuda() itself.
// The phases: arguments, devices, the k-means|| detour, set-up, seeding, the schedule (Job::run), statistics, outputs.
int kmamd_kmeans_weighted(int init_, const void *init_params, float tolerance, float yinyang_t, int metric_,
                          uint32_t samples_size, uint16_t features_size, uint32_t clusters_size, uint32_t seed,
                          uint32_t device, int32_t device_ptrs, int32_t fp16x2, int32_t verbosity, const float *samples,
                          float *centroids, uint32_t *assignments, float *average_distance,
                          const float *sample_weights) {
  KMCUDAInitMethod init = static_cast<KMCUDAInitMethod>(init_);
  const KMCUDADistanceMetric metric = static_cast<KMCUDADistanceMetric>(metric_);
  kmx::g_verbosity = verbosity;
  DEBUG("arguments: %d %p %.3f %.2f %d %u %u %u %u %u %d %d %p %p %p %p\n", init, init_params, tolerance, yinyang_t,
        metric, samples_size, (unsigned)features_size, clusters_size, seed, device, fp16x2, verbosity,
        (const void *)samples, (void *)centroids, (void *)assignments, (void *)average_distance);
  const KmeansSwitches sw = kmeans_switches();   // read here, once: nothing below looks at the environment
  RETERR(check_kmeans_args(sw, init, tolerance, yinyang_t, samples_size, features_size, clusters_size, device, fp16x2,
                           verbosity, samples, centroids, assignments, sample_weights));
  INFO("reassignments threshold: %u\n", uint32_t(tolerance * samples_size));
  const uint32_t yy_groups_size = yinyang_t * clusters_size;  // float product, truncated (kmcuda.cc:417)
  DEBUG("yinyang groups: %u\n", yy_groups_size);
  auto devs = setup_devices(device, verbosity);
  if (devs.empty()) return kmcudaNoSuchDevice;
  RETERR(seed_parallel_first(&init, init_params, metric, samples_size, features_size, clusters_size, seed, devs[0],
                             device_ptrs, fp16x2, verbosity, samples, centroids));
  sync_callers_device(device_ptrs);
  PreloadThreads preload;   // (joined when this call returns, whichever way)
  for (int d : devs) preload_code_objects(d, &preload, sw);
  // KMCUDA_AMD_TIMING=1: wall-clock laps of the call's phases on stderr (a measurement aid; each lap waits for the GPUs)
  PhaseClock clock(sw.timing);
  const auto t_begin = clock.t_lap;
  Job job;
  clock.wait = [&job] { (void)job.sync_all(); };
  job.fp16 = fp16x2 != 0;
  job.strict_h2 = job.fp16 && sw.fp16_strict;
  // fp16x2: features_size counts half2 pairs (kmcuda.h:107-108); internally one feature per half
  const uint32_t feats = fp16x2 ? 2u * features_size : features_size;
  RETERR(job.setup(sw, devs, sw.virtual_shards, samples_size, feats, clusters_size, metric, verbosity, samples,
                   device_ptrs, nullptr, sample_weights));
  clock.lap("set-up (engines, uploads)");
  if (job.exact_update && job.shards.size() > 1) {
    INFO("KMCUDA_AMD_EXACT_UPDATE needs all rows on one GPU (the reference's update order is global)\n");
    return kmcudaInvalidArguments;
  }
  const uint32_t afk_m = (init == kmcudaInitMethodAFKMC2 && init_params) ? *reinterpret_cast<const uint32_t *>(init_params) : 0;
  RETERR(job.init_centroids(init, seed, centroids, device_ptrs, afk_m));
  RETERR(job.sync_all());
  clock.lap("seeding");
  const auto t_loop = std::chrono::steady_clock::now();
  job.stats.setup_seconds = std::chrono::duration<double>(t_loop - t_begin).count();
  job.stats.shards = (uint32_t)job.shards.size();
  job.stats.rccl = job.comms.empty() ? 0u : (uint32_t)job.comms.size();
  RETERR(job.run(tolerance, yy_groups_size, clock));
  RETERR(job.sync_all());
  publish_run_stats(job, t_loop);
  clock.lap("loop end");
  if (average_distance) RETERR(job.average_distance(average_distance));
  RETERR(job.gather_outputs(centroids, assignments, device_ptrs));
  clock.lap("outputs");
  DEBUG("return kmcudaSuccess\n");
  return kmcudaSuccess;
}

KMCUDAResult knn_cuda(uint16_t k, KMCUDADistanceMetric metric, uint32_t samples_size, uint16_t features_size,
                      uint32_t clusters_size, uint32_t device, int32_t device_ptrs, int32_t fp16x2, int32_t verbosity,
                      const float *samples, const float *centroids, const uint32_t *assignments, uint32_t *neighbors) {
  kmx::g_verbosity = verbosity;
  DEBUG("arguments: %u %d %u %u %u %u %d %d %d %p %p %p %p\n", (unsigned)k, metric, samples_size,
        (unsigned)features_size, clusters_size, device, device_ptrs, fp16x2, verbosity, (const void *)samples,
        (const void *)centroids, (const void *)assignments, (void *)neighbors);
  // reference: check_knn_args, kmcuda.cc:537-570 (its result is ignored there, :583-584; we report it)
  if (k == 0) return kmcudaInvalidArguments;
  if (clusters_size < 2 || clusters_size == UINT32_MAX) return kmcudaInvalidArguments;
  if (features_size == 0) return kmcudaInvalidArguments;
  if (samples_size < clusters_size) return kmcudaInvalidArguments;
  if (device_mask_refused(device)) return kmcudaNoSuchDevice;
  if (!samples || !centroids || !assignments || !neighbors) return kmcudaInvalidArguments;
  auto devs = setup_devices(device, verbosity);
  if (devs.empty()) return kmcudaNoSuchDevice;
  sync_callers_device(device_ptrs);   // as kmeans_cuda
  KnnCorpus c;
  c.metric = metric; c.fp16 = fp16x2 != 0; c.N = samples_size; c.K = clusters_size;
  c.D = fp16x2 ? 2u * features_size : features_size;  // kmcuda.h:107-108
  c.samples = samples; c.centroids = centroids; c.assignments = assignments; c.device_ptrs = device_ptrs;
  RETERR(knn_job_run(devs, virtual_shards(), k, c, verbosity, neighbors));   // (knn_job.cpp)
  DEBUG("return kmcudaSuccess\n");
  return kmcudaSuccess;
}

int kmamd_last_run_stats(uint32_t *iterations, double *loop_seconds, double *setup_seconds, uint32_t *shards,
                         uint32_t *rccl_ranks) {
  std::lock_guard<std::mutex> lock(g_last_run_mutex);
  if (iterations) *iterations = g_last_run.iterations;
  if (loop_seconds) *loop_seconds = g_last_run.loop_seconds;
  if (setup_seconds) *setup_seconds = g_last_run.setup_seconds;
  if (shards) *shards = g_last_run.shards;
  if (rccl_ranks) *rccl_ranks = g_last_run.rccl;
  return kmcudaSuccess;
}

int kmamd_last_run_collective(double *milliseconds, uint32_t *count) {
  std::lock_guard<std::mutex> lock(g_last_run_mutex);
  if (milliseconds) *milliseconds = g_last_run.collective_ms;
  if (count) *count = g_last_run.collectives;
  return kmcudaSuccess;
}

}  // extern "C"
