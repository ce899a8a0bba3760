// host_job.hpp -- the host plumbing the chunked row calls share: kmamd_kmeans_assign (assign_job.cpp),
// kmamd_kmeans_assign_top (assign_top_job.cpp), kmamd_kmeans_seed_parallel (seed_par_job.cpp) and, for the arena alone,
// the k-NN files (knn_host.hpp).  The queries and added rows of the k-NN index stay off RowStage: SortedChunk::upload
// (knn_index.cpp) always copies, device to device too, into buffers its init() sizes together with everything else.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <functional>
#include <memory>
#include <vector>

#include "../../include/kmcuda.h"
#include "engine.hpp"

namespace kmx {

// error plumbing of the host job files: a result other than success returns at once
#define KNN_TRY(call) do { int rc__ = (call); if (rc__ != 0) return rc__; } while (false)
#define KMX_HIPRT(call) do { if ((call) != hipSuccess) return kmcudaRuntimeError; } while (false)
#define KMX_HIPCP(call) do { if ((call) != hipSuccess) return kmcudaMemoryCopyError; } while (false)

// KMCUDA_AMD_FP16_STRICT "set and non-zero": the reference's half2 arithmetic is asked for.  The one place that parses
// it -- the switch sets (kmeans_switches, knn_switches) and the calls that refuse it (rows_call_begin, the mini-batch
// model) all ask here.
inline bool fp16_strict_requested() {
  const char *v = getenv("KMCUDA_AMD_FP16_STRICT");
  return v && atoi(v) != 0;
}

// KMCUDA_AMD_TIMING: wall-clock laps of a call's phases on stderr (a measurement aid).  lap() first runs `wait` (what
// the lap has to wait for so that it measures finished work: the job's GPUs, a stream, or nothing where the code around
// it has waited already), then prints "[timing] <what>: <ms since the last lap> ms".  Switched off it does nothing.
struct PhaseClock {
  bool on = false;
  std::function<void()> wait;
  std::chrono::steady_clock::time_point t_lap = std::chrono::steady_clock::now();
  explicit PhaseClock(bool on_, std::function<void()> wait_ = nullptr) : on(on_), wait(std::move(wait_)) {}
  __attribute__((format(printf, 2, 3))) void lap(const char *fmt, ...) {
    if (!on) return;
    if (wait) wait();
    const auto t1 = std::chrono::steady_clock::now();
    char what[128];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(what, sizeof(what), fmt, ap);
    va_end(ap);
    fprintf(stderr, "[timing] %s: %.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t_lap).count());
    t_lap = t1;
  }
};

// The device buffers of one call (or of one prepared corpus: KnnShard) on one GPU and the pooled stream its work is
// enqueued on: everything alloc() hands out is freed with the arena, and the stream goes back to its pool (a null
// stream: nothing to release -- the owner enqueues on somebody else's).
struct DeviceArena {
  int dev = 0;
  hipStream_t stream = nullptr;
  std::vector<void *> owned;
  ~DeviceArena() {
    (void)hipSetDevice(dev);
    for (void *p : owned) (void)hipFree(p);
    pooled_stream_release(dev, stream);
  }
  template <typename T>
  int alloc(T **p, size_t count) {
    void *q = nullptr;
    if (hipMalloc(&q, count ? count * sizeof(T) : sizeof(T)) != hipSuccess) return kmcudaMemoryAllocationFailure;
    owned.push_back(q);
    *p = static_cast<T *>(q);
    return 0;
  }
  // frees one buffer of alloc() early (a no-op for anything else, e.g. a caller's buffer used in place)
  void release(const void *p) {
    for (size_t i = 0; i < owned.size(); i++)
      if (owned[i] == p) {
        (void)hipFree(owned[i]);
        owned.erase(owned.begin() + i);
        return;
      }
  }
  // brings `count` elements of a caller buffer onto this device (or uses it in place)
  template <typename T>
  int stage_in(const T *src, size_t count, int32_t device_ptrs, const T **dst) {
    if (device_ptrs >= 0 && device_ptrs == dev) {
      *dst = src;
      return 0;
    }
    T *buf = nullptr;
    int rc = alloc(&buf, count);
    if (rc) return rc;
    hipError_t e = device_ptrs < 0
                       ? hipMemcpyAsync(buf, src, count * sizeof(T), hipMemcpyHostToDevice, stream)
                       : hipMemcpyPeerAsync(buf, dev, src, device_ptrs, count * sizeof(T), stream);
    if (e != hipSuccess) return kmcudaMemoryCopyError;
    *dst = buf;
    return 0;
  }
};

// "Rows of the caller, fp32 on this device": a slice of a caller's row matrix (fp32 or halves, host memory or this
// device's) as the kernels read it.  reserve() allocates once for slices of up to rows_cap rows -- the fp32 buffer
// unless the rows are the device's own floats, the half buffer for host halves --, stage() enqueues one slice on the
// arena's stream: upload, widen, or nothing at all (device-resident fp32 rows are used in place).  A later stage()
// overwrites the buffers; the stream orders it behind the kernels that read them.
struct RowStage {
  DeviceArena *arena = nullptr;
  uint32_t D = 0;
  bool fp16 = false, host = true;
  float *rows32 = nullptr;
  uint16_t *rows16 = nullptr;

  int reserve(DeviceArena &a, size_t rows_cap, uint32_t D_, bool fp16_, bool host_) {
    arena = &a; D = D_; fp16 = fp16_; host = host_;
    if (host || fp16) KNN_TRY(a.alloc(&rows32, rows_cap * D));
    if (host && fp16) KNN_TRY(a.alloc(&rows16, rows_cap * D));
    return 0;
  }
  // where the halves of the slice from first_row on lie on the device once staged -- the caller's own buffer or the
  // upload, aligned or not --, null for fp32 rows (known before stage(): an engine made for the slice, whose init()
  // enqueues on the same stream, can be given them first)
  const void *halves_at(const void *src, size_t first_row) const {
    if (!fp16) return nullptr;
    return host ? rows16 : static_cast<const uint16_t *>(src) + first_row * D;
  }
  // rows [first_row, first_row + n) of src; *halves (optional): halves_at(src, first_row)
  int stage(const void *src, size_t first_row, size_t n, const float **rows, const void **halves = nullptr) {
    const hipStream_t st = arena->stream;
    const size_t at = first_row * D, count = n * D;
    const void *h = halves_at(src, first_row);
    if (fp16) {
      if (host)
        KMX_HIPCP(hipMemcpyAsync(rows16, static_cast<const uint16_t *>(src) + at, count * sizeof(uint16_t),
                                 hipMemcpyHostToDevice, st));
      KMX_HIPRT(launch_half_to_float(h, count, rows32, st));
      *rows = rows32;
    } else if (host) {
      KMX_HIPCP(hipMemcpyAsync(rows32, static_cast<const float *>(src) + at, count * sizeof(float),
                               hipMemcpyHostToDevice, st));
      *rows = rows32;
    } else {
      *rows = static_cast<const float *>(src) + at;
    }
    if (halves) *halves = h;
    return 0;
  }
};

// Rows per chunk of the assign calls: a chunk's staged fp32 rows stay within 4 GiB, as the index's chunks do
// (knn_index.cpp); KMCUDA_AMD_ASSIGN_CHUNK: rows per chunk (the tests force small chunks)
constexpr size_t kAssignChunkBytes = (size_t)4 << 30;
inline size_t assign_chunk_rows(uint32_t D) {
  size_t chunk = kAssignChunkBytes / ((size_t)D * sizeof(float));
  if (const char *v = getenv("KMCUDA_AMD_ASSIGN_CHUNK")) {
    const long long n = atoll(v);
    if (n > 0) chunk = (size_t)n;
  }
  return chunk < 1 ? 1 : chunk;
}

// The engine of a job's assignment passes, sized for what is at hand: get() keeps the engine it holds while (rows,
// clusters) stay what it was built for and otherwise drains the stream (the passes of the engine that goes) and builds
// a new one.  Halves reach the filter only where they lie 16-byte aligned.  Declare it after the arena whose stream it
// runs on: the engine must go first.
struct EngineSlot {
  std::unique_ptr<Engine> eng;
  uint32_t rows = 0, clusters = 0;

  int get(int device, uint32_t rows_, uint32_t D, uint32_t clusters_, int metric, hipStream_t st, const void *halves,
          Engine **out) {
    if (!eng || rows != rows_ || clusters != clusters_) {
      if (eng) KMX_HIPRT(hipStreamSynchronize(st));
      eng.reset(new Engine());
      KNN_TRY(eng->init(device, rows_, D, clusters_, metric, 0, st));
      rows = rows_; clusters = clusters_;
    }
    eng->half_rows_ = ((uintptr_t)halves & 15u) == 0 ? halves : nullptr;
    *out = eng.get();
    return 0;
  }
  void reset() { eng.reset(); }
};

// The common front of the three entry points, behind their own argument checks (K, m, rounds, null pointers): what is
// refused is refused before any device work, with the outputs untouched, and only then the device is looked for.
inline int rows_call_begin(int metric, uint32_t features_size, int32_t fp16x2, int device, int32_t device_ptrs,
                           int32_t verbosity, int max_device = INT_MAX) {
  if (metric != 0 && metric != 1) return kmcudaInvalidArguments;
  if (features_size == 0 || (fp16x2 && (features_size & 1u))) return kmcudaInvalidArguments;
  if (device < 0 || device > max_device || (device_ptrs >= 0 && device_ptrs != device)) return kmcudaInvalidArguments;
  // the reference's half2 arithmetic has no predict form (sample weights refuse it for the same reason)
  if (fp16x2 && fp16_strict_requested()) return kmcudaInvalidArguments;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) return kmcudaNoSuchDevice;
  if (hipSetDevice(device) != hipSuccess) return kmcudaNoSuchDevice;
  g_verbosity = verbosity;
  return kmcudaSuccess;
}

}  // namespace kmx
