// minibatch_job.cpp -- kmamd_minibatch_* of include/kmcuda_amd.h: mini-batch K-means (Sculley's per-centre learning
// rate, what scikit-learn's MiniBatchKMeans.partial_fit does) on a model that stays on the device between calls
// (DESIGN.md 4.14).
//
// The handle owns a DeviceArena with its pooled stream, an EngineSlot, the state -- K x D float32 centroids, K fp64
// cluster weights, the step counter -- and the buffers of one batch.  A step is what kmamd_kmeans_assign does with a
// chunk (host_job.hpp: RowStage, EngineSlot; assignments <- K, one filtered bit-exact assignment pass), then the CSR of
// the batch (launch_inverse_assignments) and ONE launch of minibatch_update (minibatch.hip), which sums every
// centroid's members and moves the centroid in place.  The engine is rebuilt only when a step's row count differs from
// the last one's.  fit() draws its batches by the stateless hash of hash_draw.hpp: on the device for a device-resident
// corpus (nothing is read back between the steps), by the same arithmetic on the host for a host corpus, gathered into
// one of two pinned buffers while the device works on the step before.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <thread>

#include "../../include/kmcuda_amd.h"
#include "hash_draw.hpp"
#include "host_job.hpp"

using namespace kmx;

// host threads of fit()'s gather from a host corpus: up to 8, never more than the machine's
static uint32_t gather_threads() {
  const unsigned hw = std::thread::hardware_concurrency();
  return hw == 0 ? 1u : (hw < 8 ? hw : 8u);
}

struct kmamd_minibatch {
  int metric = 0, device = 0, verbosity = 0;
  uint32_t D = 0, K = 0;
  DeviceArena w;     // the state, the batch buffers and the pooled stream (destroyed after the engine below)
  EngineSlot slot;   // sized for the last step's rows
  // ---- the state ----
  float *C = nullptr;
  double *W = nullptr;
  uint64_t t = 0;
  // ---- one batch: grown to the largest step seen ----
  size_t cap = 0, cap32 = 0, cap16 = 0;
  float *rows32 = nullptr, *wbuf = nullptr;
  uint16_t *rows16 = nullptr;
  uint32_t *asg = nullptr, *prev = nullptr, *inv = nullptr, *keys_tmp = nullptr, *vals_tmp = nullptr,
           *keys_sorted = nullptr, *offsets = nullptr;
  char *sort_temp = nullptr;
  size_t sort_bytes = 0;
  double *wcheck = nullptr;
  // ---- fit() on a host corpus: two pinned batches (rows, then weights) and the events of their uploads ----
  char *pinned[2] = {nullptr, nullptr};
  size_t pinned_bytes = 0;
  hipEvent_t uploaded[2] = {nullptr, nullptr};

  ~kmamd_minibatch() {
    (void)hipSetDevice(device);
    if (w.stream) (void)hipStreamSynchronize(w.stream);
    for (int b = 0; b < 2; b++) {
      if (pinned[b]) (void)hipHostFree(pinned[b]);
      if (uploaded[b]) (void)hipEventDestroy(uploaded[b]);
    }
  }

  template <typename T>
  int grow(T **p, size_t count) {
    if (*p) w.release(*p);
    *p = nullptr;
    return w.alloc(p, count);
  }

  // buffers for a step of n rows; need32: the fp32 rows are not the caller's own device buffer; need16: halves that
  // are not the caller's own device buffer
  int reserve(size_t n, bool need32, bool need16) {
    const bool more = n > cap || (need32 && n > cap32) || (need16 && n > cap16);
    if (more) KMX_HIPRT(hipStreamSynchronize(w.stream));   // (whatever still reads the buffers that go)
    if (n > cap) {
      KNN_TRY(grow(&wbuf, n));
      KNN_TRY(grow(&asg, n));
      KNN_TRY(grow(&prev, n));
      KNN_TRY(grow(&inv, n));
      KNN_TRY(grow(&keys_tmp, n));
      KNN_TRY(grow(&vals_tmp, n));
      KNN_TRY(grow(&keys_sorted, n));
      sort_bytes = sort_temp_bytes(n, K);
      KNN_TRY(grow(&sort_temp, sort_bytes + 16));
      cap = n;
    }
    if (need32 && n > cap32) {
      KNN_TRY(grow(&rows32, n * D));
      cap32 = n;
    }
    if (need16 && n > cap16) {
      KNN_TRY(grow(&rows16, n * D));
      cap16 = n;
    }
    return 0;
  }

  // the handle's row buffers as the RowStage of one call
  RowStage stage_view(bool fp16, bool host) {
    RowStage rs;
    rs.arena = &w; rs.D = D; rs.fp16 = fp16; rs.host = host;
    rs.rows32 = rows32; rs.rows16 = rows16;
    return rs;
  }

  // every weight finite and > 0?  (device weights; one host read)
  int weights_ok(const float *weights_dev, uint64_t n, bool *ok) {
    *ok = true;
    for (uint64_t at = 0; at < n && *ok; at += 0x80000000ull) {
      const uint32_t len = (uint32_t)(n - at < 0x80000000ull ? n - at : 0x80000000ull);
      double res[2] = {0.0, 0.0};
      KMX_HIPRT(launch_weights_check(weights_dev + at, len, wcheck, w.stream));
      KMX_HIPCP(hipMemcpyAsync(res, wcheck, sizeof(res), hipMemcpyDeviceToHost, w.stream));
      KMX_HIPRT(hipStreamSynchronize(w.stream));
      if (res[1] != 0.0) *ok = false;
    }
    return 0;
  }

  // one step on n staged rows (enqueued; `out`: n words on the device)
  int step_core(uint32_t n, const float *rows, const float *weights_dev, uint32_t *out) {
    const hipStream_t st = w.stream;
    KMX_HIPRT(launch_inverse_assignments(out, n, K, keys_tmp, vals_tmp, keys_sorted, inv, offsets, sort_temp,
                                         sort_bytes, st));
    KMX_HIPRT(launch_minibatch_update(metric, rows, weights_dev, inv, offsets, K, D, C, W, st));
    t++;
    return 0;
  }
  // assignments <- K ("no cluster"), then one pass: a row without a nearest centroid keeps K
  int assign(Engine *eng, uint32_t n, const float *rows, uint32_t *out) {
    KMX_HIPRT(hipMemsetD32Async((hipDeviceptr_t)out, (int)K, n, w.stream));
    return eng->lloyd_assign(rows, C, out, prev, false);
  }

  int step(uint32_t n, bool fp16, const void *rows, const float *weights, uint32_t *assignments, bool host) {
    const hipStream_t st = w.stream;
    KNN_TRY(reserve(n, host || fp16, host && fp16));
    const float *wdev = nullptr;
    if (weights) {   // a bad weight leaves C, W and t as they are: checked before anything else
      wdev = weights;
      if (host) {
        KMX_HIPCP(hipMemcpyAsync(wbuf, weights, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
        wdev = wbuf;
      }
      bool ok = true;
      KNN_TRY(weights_ok(wdev, n, &ok));
      if (!ok) return kmcudaInvalidArguments;
    }
    RowStage rs = stage_view(fp16, host);
    const float *rows_dev = nullptr;
    Engine *eng = nullptr;
    KNN_TRY(slot.get(device, n, D, K, metric, st, rs.halves_at(rows, 0), &eng));
    KNN_TRY(rs.stage(rows, 0, n, &rows_dev));
    uint32_t *out = (!host && assignments) ? assignments : asg;
    KNN_TRY(assign(eng, n, rows_dev, out));
    KNN_TRY(step_core(n, rows_dev, wdev, out));
    if (host && assignments)
      KMX_HIPCP(hipMemcpyAsync(assignments, out, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    KMX_HIPRT(hipStreamSynchronize(st));
    return kmcudaSuccess;
  }

  int fit(uint64_t N, bool fp16, const void *samples, const float *weights, uint32_t batch, uint32_t steps,
          uint32_t seed, bool host) {
    const hipStream_t st = w.stream;
    const size_t esz = fp16 ? sizeof(uint16_t) : sizeof(float), row_bytes = (size_t)D * esz;
    KNN_TRY(reserve(batch, true, fp16));
    if (weights && !host) {
      bool ok = true;
      KNN_TRY(weights_ok(weights, N, &ok));
      if (!ok) return kmcudaInvalidArguments;
    }
    if (host) {
      const size_t bytes = (size_t)batch * row_bytes + (size_t)batch * sizeof(float);
      if (bytes > pinned_bytes) {
        KMX_HIPRT(hipStreamSynchronize(st));
        for (int b = 0; b < 2; b++) {
          if (pinned[b]) (void)hipHostFree(pinned[b]);
          pinned[b] = nullptr;
          if (hipHostMalloc((void **)&pinned[b], bytes, hipHostMallocDefault) != hipSuccess) {
            pinned_bytes = 0;
            return kmcudaMemoryAllocationFailure;
          }
        }
        pinned_bytes = bytes;
      }
    }
    void *batch_rows = fp16 ? (void *)rows16 : (void *)rows32;
    for (uint32_t s = 0; s < steps; s++) {
      const uint32_t r = (uint32_t)t;   // the handle's running counter: fit(.., 10) twice is fit(.., 20)
      Engine *eng = nullptr;
      KNN_TRY(slot.get(device, batch, D, K, metric, st, fp16 ? rows16 : nullptr, &eng));
      if (host) {
        const int b = (int)(s & 1u);
        if (s >= 2) KMX_HIPRT(hipEventSynchronize(uploaded[b]));   // the upload that last read this buffer
        char *prow = pinned[b];
        float *pw = reinterpret_cast<float *>(pinned[b] + (size_t)batch * row_bytes);
        const char *src = static_cast<const char *>(samples);
        auto gather = [&](uint32_t j0, uint32_t j1) {
          for (uint32_t j = j0; j < j1; j++) {
            const uint64_t row = draw_row(hash_draw(seed, r, j), N);
            memcpy(prow + (size_t)j * row_bytes, src + row * row_bytes, row_bytes);
            if (weights) pw[j] = weights[row];
          }
        };
        // (a slot's row depends on (seed, r, j) alone: slices of the slots on a few threads where a batch is megabytes)
        const uint32_t nthreads = (size_t)batch * row_bytes >= ((size_t)4 << 20) ? gather_threads() : 1u;
        if (nthreads > 1) {
          std::vector<std::thread> pool;
          const uint32_t per = (batch + nthreads - 1) / nthreads;
          for (uint32_t k = 0; k < nthreads && k * per < batch; k++)
            pool.emplace_back(gather, k * per, std::min(batch, (k + 1) * per));
          for (std::thread &th : pool) th.join();
        } else {
          gather(0, batch);
        }
        KMX_HIPCP(hipMemcpyAsync(batch_rows, prow, (size_t)batch * row_bytes, hipMemcpyHostToDevice, st));
        if (weights) KMX_HIPCP(hipMemcpyAsync(wbuf, pw, (size_t)batch * sizeof(float), hipMemcpyHostToDevice, st));
        KMX_HIPRT(hipEventRecord(uploaded[b], st));
      } else {
        KMX_HIPRT(launch_minibatch_draw_gather(samples, N, D, fp16, weights, seed, r, batch, batch_rows, wbuf, st));
      }
      if (fp16) KMX_HIPRT(launch_half_to_float(rows16, (size_t)batch * D, rows32, st));
      KNN_TRY(assign(eng, batch, rows32, asg));
      KNN_TRY(step_core(batch, rows32, weights ? wbuf : nullptr, asg));
    }
    KMX_HIPRT(hipStreamSynchronize(st));
    return kmcudaSuccess;
  }
};

namespace {

// what step and fit refuse about their rows, before any device work
int rows_refused(const kmamd_minibatch *h, uint64_t n, int32_t fp16x2, int32_t device_ptrs) {
  if (!h) return kmcudaInvalidArguments;
  if (device_ptrs >= 0 && device_ptrs != h->device) return kmcudaInvalidArguments;
  if (fp16x2 && ((h->D & 1u) || fp16_strict_requested())) return kmcudaInvalidArguments;
  if (n > assign_chunk_rows(h->D)) return kmcudaInvalidArguments;
  return 0;
}

}  // namespace

extern "C" {

int kmamd_minibatch_create(kmamd_minibatch **out, int metric, uint32_t features, uint32_t clusters, int device,
                           int32_t device_ptrs, int32_t verbosity, const float *centroids,
                           const double *cluster_weights) {
  // ---- everything that is refused is refused here, before any device work ----
  if (!out) return kmcudaInvalidArguments;
  *out = nullptr;
  if (clusters < 2 || clusters >= 0x7FFFFFFFu || features > 0xFFFFu || !centroids) return kmcudaInvalidArguments;
  if (cluster_weights && device_ptrs < 0)
    for (uint32_t c = 0; c < clusters; c++)
      if (!(cluster_weights[c] >= 0.0) || isinf(cluster_weights[c])) return kmcudaInvalidArguments;
  KNN_TRY(rows_call_begin(metric, features, 0, device, device_ptrs, verbosity));
  if (device_ptrs >= 0) (void)hipDeviceSynchronize();   // the caller's writes, as kmamd_kmeans_assign
  std::unique_ptr<kmamd_minibatch> h(new kmamd_minibatch());
  h->metric = metric; h->device = device; h->verbosity = verbosity;
  h->D = features; h->K = clusters;
  h->w.dev = device;
  h->w.stream = pooled_stream_acquire(device);
  if (!h->w.stream) return kmcudaRuntimeError;
  const hipStream_t st = h->w.stream;
  const size_t cd = (size_t)clusters * features;
  KNN_TRY(h->w.alloc(&h->C, cd));
  KNN_TRY(h->w.alloc(&h->W, clusters));
  KNN_TRY(h->w.alloc(&h->offsets, (size_t)clusters + 2));
  KNN_TRY(h->w.alloc(&h->wcheck, weights_check_doubles()));
  for (int b = 0; b < 2; b++) KMX_HIPRT(hipEventCreateWithFlags(&h->uploaded[b], hipEventDisableTiming));
  const hipMemcpyKind kind = device_ptrs < 0 ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  KMX_HIPCP(hipMemcpyAsync(h->C, centroids, cd * sizeof(float), kind, st));
  if (cluster_weights) {
    KMX_HIPCP(hipMemcpyAsync(h->W, cluster_weights, (size_t)clusters * sizeof(double), kind, st));
    if (device_ptrs >= 0) {   // (weights on the device can only be looked at now; nothing has been handed out yet)
      std::vector<double> cw(clusters);
      KMX_HIPCP(hipMemcpyAsync(cw.data(), h->W, (size_t)clusters * sizeof(double), hipMemcpyDeviceToHost, st));
      KMX_HIPRT(hipStreamSynchronize(st));
      for (double v : cw)
        if (!(v >= 0.0) || isinf(v)) return kmcudaInvalidArguments;
    }
  } else {
    KMX_HIPRT(hipMemsetAsync(h->W, 0, (size_t)clusters * sizeof(double), st));
  }
  KMX_HIPRT(hipStreamSynchronize(st));
  *out = h.release();
  return kmcudaSuccess;
}

int kmamd_minibatch_step(kmamd_minibatch *h, uint32_t n_rows, int32_t fp16x2, const void *rows, const float *weights,
                         uint32_t *assignments, int32_t device_ptrs) {
  KNN_TRY(rows_refused(h, n_rows, fp16x2, device_ptrs));
  if (n_rows != 0 && !rows) return kmcudaInvalidArguments;
  if (n_rows == 0) {   // nothing but the counter
    h->t++;
    return kmcudaSuccess;
  }
  if (hipSetDevice(h->device) != hipSuccess) return kmcudaNoSuchDevice;
  g_verbosity = h->verbosity;
  if (device_ptrs >= 0) (void)hipDeviceSynchronize();
  return h->step(n_rows, fp16x2 != 0, rows, weights, assignments, device_ptrs < 0);
}

int kmamd_minibatch_fit(kmamd_minibatch *h, uint64_t samples_size, int32_t fp16x2, const void *samples,
                        const float *weights, uint32_t batch, uint32_t steps, uint32_t seed, int32_t device_ptrs) {
  KNN_TRY(rows_refused(h, batch, fp16x2, device_ptrs));
  if (samples_size == 0 || batch == 0 || !samples) return kmcudaInvalidArguments;
  if (weights && device_ptrs < 0)
    for (uint64_t s = 0; s < samples_size; s++)
      if (!(weights[s] > 0.f) || isinf(weights[s])) return kmcudaInvalidArguments;
  if (steps == 0) return kmcudaSuccess;
  if (hipSetDevice(h->device) != hipSuccess) return kmcudaNoSuchDevice;
  g_verbosity = h->verbosity;
  if (device_ptrs >= 0) (void)hipDeviceSynchronize();
  return h->fit(samples_size, fp16x2 != 0, samples, weights, batch, steps, seed, device_ptrs < 0);
}

int kmamd_minibatch_read(kmamd_minibatch *h, float *centroids, double *cluster_weights, uint64_t *steps_done,
                         int32_t device_ptrs) {
  if (!h || (device_ptrs >= 0 && device_ptrs != h->device)) return kmcudaInvalidArguments;
  if (steps_done) *steps_done = h->t;
  if (!centroids && !cluster_weights) return kmcudaSuccess;
  if (hipSetDevice(h->device) != hipSuccess) return kmcudaNoSuchDevice;
  const hipStream_t st = h->w.stream;
  const hipMemcpyKind kind = device_ptrs < 0 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  if (centroids) KMX_HIPCP(hipMemcpyAsync(centroids, h->C, (size_t)h->K * h->D * sizeof(float), kind, st));
  if (cluster_weights) KMX_HIPCP(hipMemcpyAsync(cluster_weights, h->W, (size_t)h->K * sizeof(double), kind, st));
  KMX_HIPRT(hipStreamSynchronize(st));
  return kmcudaSuccess;
}

void kmamd_minibatch_destroy(kmamd_minibatch *h) { delete h; }

}  // extern "C"
