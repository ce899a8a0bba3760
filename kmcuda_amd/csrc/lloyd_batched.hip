// lloyd_batched.hip -- K-means over many small independent problems in one launch train (kmamd_kmeans_batched,
// kmamd_kmeans_assign_batched; batched_job.cpp).  L2, fp32, 1 <= D <= 64.
//
//   batched_assign   grid = (row chunk, problem), the problem index running fastest.  A block stages its problem's
//                    centroid panel in LDS ONCE -- K8 x DP floats, zero padded (K8 = K rounded up to 8, DP the rung of
//                    BatchedWidths that holds D), and csqr[K8], the reference's sum of squares -- and then walks the row
//                    tiles of its chunk, one row per thread.  The row sits in registers; the panel is read as
//                    ds_read_b128 of ONE address per wave (a broadcast: no bank conflict at any stride), eight
//                    centroids' chains in flight per thread, each the reference's round-down-FMA Kahan dot over exactly
//                    D features, then RD(-2 prod + (0 + csqr)), strict `<` from FLT_MAX in ascending centroid order.
//                    There is no filter: at these widths the exact chain from LDS is the whole cost, and it decides alone.
//   batched_partial  the same (row chunk, problem) grid.  Thread t owns feature t % DP of the centroids c with
//                    c % (256 / DP) == t / DP: it walks the rows of a staged tile in ascending order and adds its
//                    feature of every member row to ITS fp64 cell in LDS -- one owner per cell, no atomics, a fixed order.
//                    The block writes one fp64 partial row per centroid and its member counts.
//   batched_finish   sums the partials of a problem in block order, moves the centroids that have members (one
//                    division in fp64, one rounding to fp32), and decides the problem's stop on the device.
// A problem that has stopped (stop[b] != 0: the pass it stopped at) costs its blocks one load: they return at once.
#include <float.h>
#include <math.h>

#include "exact.hpp"
#include "kernels.hpp"
#include "launch_dispatch.hpp"

namespace kmx {

namespace {

constexpr int kBtThreads = 256;              // one row per thread in batched_assign: a 256-row tile
constexpr uint32_t kBtNone = 0xFFFFFFFFu;
constexpr int kBtTileFloats = 2048;          // batched_partial: a staged tile is 2048 / DP rows of DP floats (8 KB)

__device__ __forceinline__ bool batched_stopped(const uint32_t *stop, uint32_t b, uint32_t pass) {
  if (!stop) return false;
  const uint32_t s = *reinterpret_cast<const volatile uint32_t *>(stop + b);
  return s != 0 && s < pass;
}

template <int DP, bool FULL>
__global__ __launch_bounds__(kBtThreads) void batched_assign_kernel(BatchedGeom g, const float *__restrict__ centroids,
                                                                    void *__restrict__ assignments, int codes_u8,
                                                                    float *__restrict__ dists, int vec4,
                                                                    uint32_t *__restrict__ changed,
                                                                    const uint32_t *__restrict__ stop, uint32_t pass) {
  const uint32_t b = blockIdx.x % g.B, chunk = blockIdx.x / g.B, t = threadIdx.x;
  if (batched_stopped(stop, b, pass)) return;
  const uint32_t D = FULL ? (uint32_t)DP : g.D, K = g.K, K8 = (K + 7u) & ~7u;
  extern __shared__ float4 batched_lds4[];
  float *panel = reinterpret_cast<float *>(batched_lds4);   // K8 x DP
  float *csqr = panel + (size_t)K8 * DP;                    // K8
  {
    const float *cen = centroids + (size_t)b * K * D;
    for (uint32_t i = t; i < K8 * DP; i += kBtThreads) {
      const uint32_t c = i / DP, f = i % DP;
      panel[i] = (c < K && f < D) ? cen[(size_t)c * D + f] : 0.f;
    }
    __syncthreads();
    for (uint32_t c = t; c < K8; c += kBtThreads) csqr[c] = kahan_dot(panel + c * DP, panel + c * DP, D);
    __syncthreads();
  }
  const uint64_t row0 = (uint64_t)chunk * g.R;
  const uint64_t rend = row0 + g.R < g.N ? row0 + g.R : g.N;
  uint32_t moved = 0;
  for (uint64_t row = row0 + t; row < rend; row += kBtThreads) {
    const float *xp = g.rows + row * g.row_stride + (uint64_t)b * g.prob_stride;
    float x[DP];
#pragma unroll
    for (int f0 = 0; f0 < DP; f0 += 4) {
      if (vec4) {   // D % 4 == 0 and every segment 16-byte aligned
        const float4 v = (uint32_t)f0 < D ? *reinterpret_cast<const float4 *>(xp + f0) : make_float4(0.f, 0.f, 0.f, 0.f);
        x[f0] = v.x; x[f0 + 1] = v.y; x[f0 + 2] = v.z; x[f0 + 3] = v.w;
      } else {
#pragma unroll
        for (int q = 0; q < 4; q++) x[f0 + q] = (uint32_t)(f0 + q) < D ? xp[f0 + q] : 0.f;
      }
    }
    float best = FLT_MAX;
    uint32_t arg = kBtNone;
    if (!(x[0] != x[0])) {   // kmeans.cu:312: a row whose first feature is NaN is not searched
      for (uint32_t c0 = 0; c0 < K8; c0 += 8) {
        float acc[8], corr[8];
#pragma unroll
        for (int j = 0; j < 8; j++) acc[j] = corr[j] = 0.f;
#pragma unroll
        for (int f0 = 0; f0 < DP; f0 += 4) {
          if (FULL || (uint32_t)f0 < D) {   // (uniform: the chain covers exactly D features)
            float4 cv[8];
#pragma unroll
            for (int j = 0; j < 8; j++) cv[j] = *reinterpret_cast<const float4 *>(panel + (c0 + j) * DP + f0);
#pragma unroll
            for (int q = 0; q < 4; q++) {
              if (FULL || (uint32_t)(f0 + q) < D) {
                float bq[8], y[8];
#pragma unroll
                for (int j = 0; j < 8; j++) bq[j] = q == 0 ? cv[j].x : q == 1 ? cv[j].y : q == 2 ? cv[j].z : cv[j].w;
                fma_rd8(x[f0 + q], bq, corr, y);
#pragma unroll
                for (int j = 0; j < 8; j++) kahan_fold(y[j], acc[j], corr[j]);
              }
            }
          }
        }
        // lloyd_distance<0>: RD(-2 prod + (0 + csqr)), the eight of the group under one rounding-mode window
        float cs[8], dist[8];
#pragma unroll
        for (int j = 0; j < 8; j++) cs[j] = 0.f + csqr[c0 + j];
        fma_rd8(-2.f, acc, cs, dist);
#pragma unroll
        for (int j = 0; j < 8; j++)
          if (c0 + j < K && dist[j] < best) {
            best = dist[j];
            arg = c0 + j;
          }
      }
    }
    const uint32_t a = arg == kBtNone ? K : arg;
    const uint64_t at = row * g.out_row_stride + (uint64_t)b * g.out_prob_stride;
    if (codes_u8) {
      static_cast<uint8_t *>(assignments)[at] = (uint8_t)a;
    } else {
      uint32_t *asg = static_cast<uint32_t *>(assignments);
      if (changed) {
        if (asg[at] != a) {
          asg[at] = a;
          moved++;
        }
      } else {
        asg[at] = a;
      }
    }
    if (dists) {
      float d2 = NAN;
      if (arg != kBtNone) {   // distance_vv<0>'s chain against the panel row
        const float *cp = panel + arg * DP;
        float acc = 0.f, corr = 0.f;
#pragma unroll
        for (int f = 0; f < DP; f++) {
          if (FULL || (uint32_t)f < D) {
            const float d = x[f] - cp[f];
            kahan_fold(fma_rd(d, d, corr), acc, corr);
          }
        }
        d2 = sqrtf(acc);
      }
      dists[at] = d2;
    }
  }
  if (changed) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) moved += __shfl_xor(moved, m, 64);
    if ((t & 63u) == 0 && moved) atomicAdd(changed + b, moved);   // an integer count: any order, the same sum
  }
}

template <int DP>
__global__ __launch_bounds__(kBtThreads) void batched_partial_kernel(BatchedGeom g,
                                                                     const uint32_t *__restrict__ assignments,
                                                                     double *__restrict__ psum,
                                                                     uint32_t *__restrict__ pcnt,
                                                                     const uint32_t *__restrict__ stop, uint32_t pass) {
  constexpr uint32_t UT = kBtTileFloats / DP, CLS = kBtThreads / DP;
  const uint32_t b = blockIdx.x % g.B, chunk = blockIdx.x / g.B, t = threadIdx.x;
  if (batched_stopped(stop, b, pass)) return;
  const uint32_t D = g.D, K = g.K, K8 = (K + 7u) & ~7u, cells = K8 * DP;
  extern __shared__ double batched_lds8[];
  double *acc = batched_lds8;                                  // K8 x DP
  float *xt = reinterpret_cast<float *>(acc + cells);          // UT x DP
  uint32_t *at = reinterpret_cast<uint32_t *>(xt + UT * DP);   // UT
  uint32_t *cnt = at + UT;                                     // K8
  for (uint32_t i = t; i < cells; i += kBtThreads) acc[i] = 0.0;
  for (uint32_t c = t; c < K8; c += kBtThreads) cnt[c] = 0;
  const uint64_t row0 = (uint64_t)chunk * g.R;
  const uint64_t rend = row0 + g.R < g.N ? row0 + g.R : g.N;
  const uint32_t cls = t / DP, f = t % DP;
  for (uint64_t base = row0; base < rend; base += UT) {
    __syncthreads();   // the previous tile is consumed (first round: the cells are zeroed)
    for (uint32_t e = t; e < UT * DP; e += kBtThreads) {
      const uint64_t row = base + e / DP;
      const uint32_t fe = e % DP;
      xt[e] = (row < rend && fe < D) ? g.rows[row * g.row_stride + (uint64_t)b * g.prob_stride + fe] : 0.f;
    }
    for (uint32_t r = t; r < UT; r += kBtThreads) {
      const uint64_t row = base + r;
      const uint32_t a = row < rend ? assignments[row * g.out_row_stride + (uint64_t)b * g.out_prob_stride] : kBtNone;
      at[r] = a < K ? a : kBtNone;
    }
    __syncthreads();
#pragma unroll 4
    for (uint32_t r = 0; r < UT; r++) {
      const uint32_t a = at[r];
      if (a != kBtNone && (a & (CLS - 1u)) == cls) {
        acc[a * DP + f] += (double)xt[r * DP + f];
        if (f == 0) cnt[a]++;
      }
    }
  }
  __syncthreads();
  const size_t slot = (size_t)b * g.G + chunk;
  for (uint32_t i = t; i < cells; i += kBtThreads) psum[slot * cells + i] = acc[i];
  for (uint32_t c = t; c < K8; c += kBtThreads) pcnt[slot * K8 + c] = cnt[c];
}

__global__ __launch_bounds__(kBtThreads) void batched_finish_kernel(BatchedGeom g, uint32_t DP,
                                                                    const double *__restrict__ psum,
                                                                    const uint32_t *__restrict__ pcnt,
                                                                    float *__restrict__ centroids,
                                                                    uint32_t *__restrict__ changed,
                                                                    uint32_t *__restrict__ stop, uint32_t pass,
                                                                    uint32_t max_iter, float tolerance) {
  const uint32_t b = blockIdx.y, K8 = (g.K + 7u) & ~7u, cells = K8 * DP;
  if (batched_stopped(stop, b, pass)) return;   // (this pass's own mark, stop[b] == pass, stops nobody here)
  const uint32_t i = blockIdx.x * kBtThreads + threadIdx.x;
  if (i < cells) {
    const uint32_t c = i / DP, f = i % DP;
    if (c < g.K && f < g.D) {
      double sum = 0.0;
      uint32_t n = 0;
      for (uint32_t s = 0; s < g.G; s++) {   // block order
        const size_t slot = (size_t)b * g.G + s;
        sum += psum[slot * cells + i];
        n += pcnt[slot * K8 + c];
      }
      if (n) centroids[((size_t)b * g.K + c) * g.D + f] = (float)(sum / (double)n);   // no members: the bits stay
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint32_t moved = changed[b];
    changed[b] = 0;
    if ((double)moved <= (double)tolerance * (double)g.N || pass >= max_iter) stop[b] = pass;
  }
}

__global__ __launch_bounds__(kBtThreads) void batched_gather_kernel(BatchedGeom g, const uint32_t *__restrict__ picks,
                                                                    float *__restrict__ centroids) {
  const uint64_t i = (uint64_t)blockIdx.x * kBtThreads + threadIdx.x, total = (uint64_t)g.B * g.K * g.D;
  if (i >= total) return;
  const uint32_t f = (uint32_t)(i % g.D), b = (uint32_t)(i / ((uint64_t)g.K * g.D));
  centroids[i] = g.rows[(uint64_t)picks[i / g.D] * g.row_stride + (uint64_t)b * g.prob_stride + f];
}

__global__ __launch_bounds__(kBtThreads) void batched_fill_kernel(uint32_t *__restrict__ p, uint64_t n, uint32_t v) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBtThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBtThreads)
    p[i] = v;
}

}  // namespace

size_t batched_partial_lds_bytes(uint32_t K, uint32_t DP) {
  const size_t K8 = (K + 7u) & ~7u;
  return K8 * DP * sizeof(double) + kBtTileFloats * sizeof(float) + (kBtTileFloats / DP) * sizeof(uint32_t) +
         K8 * sizeof(uint32_t);
}

hipError_t launch_batched_assign(const BatchedGeom &g, const float *centroids, void *assignments, bool codes_u8,
                                 float *dists, uint32_t *changed, const uint32_t *stop, uint32_t pass, hipStream_t st) {
  if (g.N == 0) return hipSuccess;
  const uint32_t DP = batched_dp_for(g.D), K8 = (g.K + 7u) & ~7u;
  const size_t lds = ((size_t)K8 * DP + K8) * sizeof(float);
  const bool vec4 = (g.D & 3u) == 0 && ((g.row_stride | g.prob_stride) & 3u) == 0 && (((uintptr_t)g.rows) & 15u) == 0;
  return with_width<BatchedWidths>(DP, [&](auto W) {
    return with_flag(g.D == DP, [&](auto F) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&batched_assign_kernel<W(), F()>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL((batched_assign_kernel<W(), F()>), dim3(g.B * g.G), dim3(kBtThreads), lds, st, g, centroids,
                         assignments, (int)codes_u8, dists, (int)vec4, changed, stop, pass);
      return hipGetLastError();
    });
  });
}

hipError_t launch_batched_update(const BatchedGeom &g, const uint32_t *assignments, double *psum, uint32_t *pcnt,
                                 float *centroids, uint32_t *changed, uint32_t *stop, uint32_t pass, uint32_t max_iter,
                                 float tolerance, hipStream_t st) {
  const uint32_t DP = batched_dp_for(g.D), K8 = (g.K + 7u) & ~7u;
  const size_t lds = batched_partial_lds_bytes(g.K, DP);
  const hipError_t e = with_width<BatchedWidths>(DP, [&](auto W) {
    const hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void *>(&batched_partial_kernel<W()>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e1 != hipSuccess) return e1;
    hipLaunchKernelGGL((batched_partial_kernel<W()>), dim3(g.B * g.G), dim3(kBtThreads), lds, st, g, assignments, psum,
                       pcnt, stop, pass);
    return hipGetLastError();
  });
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(batched_finish_kernel, dim3((K8 * DP + kBtThreads - 1) / kBtThreads, g.B), dim3(kBtThreads), 0, st,
                     g, DP, psum, pcnt, centroids, changed, stop, pass, max_iter, tolerance);
  return hipGetLastError();
}

hipError_t launch_batched_gather(const BatchedGeom &g, const uint32_t *picks, float *centroids, hipStream_t st) {
  const uint64_t total = (uint64_t)g.B * g.K * g.D;
  hipLaunchKernelGGL(batched_gather_kernel, dim3((uint32_t)((total + kBtThreads - 1) / kBtThreads)), dim3(kBtThreads), 0,
                     st, g, picks, centroids);
  return hipGetLastError();
}

hipError_t launch_batched_fill(uint32_t *p, uint64_t n, uint32_t v, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const uint64_t blocks = (n + kBtThreads - 1) / kBtThreads;
  hipLaunchKernelGGL(batched_fill_kernel, dim3((uint32_t)(blocks < 65536 ? blocks : 65536)), dim3(kBtThreads), 0, st, p,
                     n, v);
  return hipGetLastError();
}

}  // namespace kmx
