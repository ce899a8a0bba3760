// assign_top.hip -- the kernels of kmamd_kmeans_assign_top (assign_top_job.cpp): for every row the m
// nearest centroids, ordered by (key ascending, centroid index ascending), where the key is the value one
// kmamd_lloyd_assign pass compares -- L2: RD(-2 prod + (0 + csqr)), angular: the clamp rule on the Kahan product with
// the C library's acosf restated (exact.hpp: angular_from_prod_libm) -- and a centroid qualifies iff key < FLT_MAX.
//
//   assign_top_exact    every key of a row in the reference's arithmetic, one wave per row over the transposed panel
//                       (lloyd_exact_kernel's layout), the best m kept in a list that lives one entry per lane
//   assign_top_scores   rows x centroids^T on the f32 matrix cores with the centred panel of centroid_prep
//                       (lloyd_filter_kernel's tile loop); writes a sub-chunk's score matrix once and, per row, the
//                       bound 2E, the clamp limits and the NaN-first-feature flag
//   assign_top_select   one wave per row over that matrix: the m-th best score v_m, then the exact key of every
//                       contender (score >= cut) and the best m of them; rows the superset argument does not cover go
//                       to a list for assign_top_exact
//   assign_top_dist     distance(row, centroid) per slot, as kmamd_kmeans_assign reports it
// No floating-point atomics anywhere; the only atomics are integer counters (exact keys evaluated: one add per wave;
// the hand-over list's cursor, whose order no output depends on).
#include <math.h>

#include "exact.hpp"
#include "filter_common.hpp"
#include "kernels.hpp"

namespace kmx {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr float kTopFltMax = 3.402823466e+38f;
constexpr uint32_t kTopNone = 0xFFFFFFFFu;
// Angular: the margin on the product that keeps the ROUNDED angles of two products in the order of the products.
// |acos'| >= 1 on (-1, 1), so products more than d apart have angles more than d apart; the restated acosf errs by
// less than one last place of its result, at most 2^-22 on [2, 4): d >= 2 * 2^-22 = 4.8e-7 suffices.
constexpr float kTopAcosMargin = 1.0e-6f;

template <int METRIC>
__device__ __forceinline__ float top_key(float csqr, float prod) {
  if (METRIC == 0) return fma_rd(-2.f, prod, 0.f + csqr);
  return angular_from_prod_libm(prod);
}

__device__ __forceinline__ bool key_less(float ka, uint32_t ia, float kb, uint32_t ib) {
  return ka < kb || (ka == kb && ia < ib);
}

// The wave's best-m list: lane j holds the j-th entry by (key, index), (+inf, kTopNone) while empty.  Every lane
// offers at most one candidate (ok); the ones in front of the m-th entry are inserted one at a time: the lanes behind
// the insertion point take their left neighbour's entry.  Wave-uniform control flow (the mask is a ballot).
__device__ __forceinline__ void top_admit(float key, uint32_t idx, bool ok, uint32_t m, int lane, float &lk,
                                          uint32_t &li) {
  float tk = __shfl(lk, (int)m - 1);
  uint32_t ti = __shfl(li, (int)m - 1);
  unsigned long long mask = __ballot(ok && key_less(key, idx, tk, ti));
  while (mask) {
    const int b = __builtin_ctzll(mask);
    mask &= mask - 1;
    const float k = __shfl(key, b);
    const uint32_t i = __shfl(idx, b);
    const bool ins = key_less(k, i, tk, ti);   // the m-th entry may have moved since the ballot
    const float uk = __shfl_up(lk, 1);
    const uint32_t ui = __shfl_up(li, 1);
    const bool front = ins && key_less(k, i, lk, li);
    const bool front_left = lane > 0 && key_less(k, i, uk, ui);
    if (front) {
      lk = front_left ? uk : k;
      li = front_left ? ui : i;
    }
    tk = __shfl(lk, (int)m - 1);
    ti = __shfl(li, (int)m - 1);
  }
}

__device__ __forceinline__ void top_emit(uint32_t *__restrict__ top, uint64_t s, uint32_t m, uint32_t K, int lane,
                                         uint32_t li) {
  if ((uint32_t)lane < m) top[s * m + (uint32_t)lane] = li == kTopNone ? K : li;
}

// ---------------------------------------------------------------------------------------
// 1. assign_top_exact: rows == nullptr: every row of [0, N); else rows[0 .. *nrows).
// ---------------------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(256) void assign_top_exact_kernel(
    const float *__restrict__ samples, uint32_t N, uint32_t D, const float *__restrict__ ct,
    const float *__restrict__ csqr, uint32_t K, uint32_t Kt, uint32_t m, const uint32_t *__restrict__ rows,
    const uint32_t *__restrict__ nrows, uint32_t *__restrict__ top, unsigned long long *__restrict__ evaluated) {
  constexpr int CH = 4;   // chains per lane: centroids cbase + 64 j + lane
  constexpr int GF = 8;   // features per load group, the next group in flight during the current one's chain
  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t total = rows ? *nrows : N;
  unsigned long long keys_done = 0;
  for (uint64_t ri = (uint64_t)blockIdx.x * 4 + wave; ri < total; ri += (uint64_t)gridDim.x * 4) {
    const uint32_t s = __builtin_amdgcn_readfirstlane(rows ? rows[ri] : (uint32_t)ri);
    const float *x = samples + (size_t)s * D;   // wave-uniform address
    float lk = INFINITY;
    uint32_t li = kTopNone;
    if (!(x[0] != x[0])) {
      keys_done += K;
      for (uint32_t cbase = 0; cbase < K; cbase += 64 * CH) {
        float acc[CH], corr[CH];
        const float *cp[CH];
#pragma unroll
        for (int j = 0; j < CH; j++) {
          acc[j] = 0.f;
          corr[j] = 0.f;
          // a column beyond the panel reads column `lane` instead; its result is dropped below (c < K)
          const uint32_t col = cbase + 64 * j + lane;
          cp[j] = ct + (col < Kt ? col : (uint32_t)lane);
        }
        auto load_group = [&](uint32_t f0, float (&xf)[GF], float (&cv)[GF][CH]) {
#pragma unroll
          for (int q = 0; q < GF; q++) {
            xf[q] = x[f0 + q];
#pragma unroll
            for (int j = 0; j < CH; j++) cv[q][j] = cp[j][(size_t)(f0 + q) * Kt];
          }
        };
        auto fold_group = [&](const float (&xf)[GF], float (&cv)[GF][CH]) {
#pragma unroll
          for (int q = 0; q < GF; q++) {
            float y[CH];
            fma_rd4(xf[q], cv[q], corr, y);
#pragma unroll
            for (int j = 0; j < CH; j++) kahan_fold(y[j], acc[j], corr[j]);
          }
        };
        uint32_t f = 0;
        if (D >= GF) {
          float xa[GF], ca[GF][CH], xb[GF], cb[GF][CH];
          load_group(0, xa, ca);
          for (; f + 2 * GF <= D; f += 2 * GF) {
            load_group(f + GF, xb, cb);
            fold_group(xa, ca);
            if (f + 3 * GF <= D) load_group(f + 2 * GF, xa, ca);
            fold_group(xb, cb);
          }
          if (f + GF <= D) {   // an odd number of groups: the last one is already loaded
            fold_group(xa, ca);
            f += GF;
          }
        }
        for (; f < D; f++) {
          const float xf = x[f];
          float cv[CH], y[CH];
#pragma unroll
          for (int j = 0; j < CH; j++) cv[j] = cp[j][(size_t)f * Kt];
          fma_rd4(xf, cv, corr, y);
#pragma unroll
          for (int j = 0; j < CH; j++) kahan_fold(y[j], acc[j], corr[j]);
        }
#pragma unroll
        for (int j = 0; j < CH; j++) {
          const uint32_t c = cbase + 64 * j + lane;
          const float key = top_key<METRIC>(c < K ? csqr[c] : 0.f, acc[j]);
          top_admit(key, c, c < K && key < kTopFltMax, m, lane, lk, li);
        }
      }
    }
    top_emit(top, s, m, K, lane, li);
  }
  if (lane == 0 && keys_done) atomicAdd(evaluated, keys_done);
}

// ---------------------------------------------------------------------------------------
// 2. assign_top_scores: lloyd_filter_kernel's operand layout and tile loop (lloyd.hip); what leaves the accumulators
// is the score itself.  Lane (col, h) holds, for row col of its wave, the scores of centroids
// t*32 + (r&3) + 8*(r>>2) + 4*h: four consecutive centroids per register quad, one 16-byte store each.
// meta[s] = (2E, clamp hi, clamp lo, first feature is NaN)
// ---------------------------------------------------------------------------------------
template <int DP, bool FAST>
__global__ __launch_bounds__(256, 2) void assign_top_scores_kernel(
    const float *__restrict__ samples, uint32_t N, uint32_t D, const float *__restrict__ cfil,
    const float *__restrict__ bias, const float *__restrict__ mu, uint32_t K_pad, const uint32_t *__restrict__ stats,
    float eps, int angular, float *__restrict__ scores, float4 *__restrict__ meta) {
  constexpr int NK = DP / 2;
  constexpr int LDW = DP + 4;
  constexpr int TILE = 32 * LDW;
  constexpr int NST = (8 * DP + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  auto tile_ptr = [&](int buf) { return lds + buf * TILE; };
  auto bias_ptr = [&](int buf) { return lds + 2 * TILE + buf * 32; };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int col = lane & 31;
  const int h = lane >> 5;
  const uint64_t s = (uint64_t)blockIdx.x * 128u + wave * 32u + col;
  const bool live = s < N;

  float xb[NK];
  float xo2 = 0.f, xm = 0.f, xma = 0.f;
  if (FAST) {
    const f32x4 *src = reinterpret_cast<const f32x4 *>(samples + (size_t)(live ? s : 0) * D + h * NK);
    const f32x4 *msrc = reinterpret_cast<const f32x4 *>(mu + h * NK);
#pragma unroll
    for (int j = 0; j < NK / 4; j++) {
      const f32x4 v = src[j], mm = msrc[j];
      const float vs[4] = {v.x, v.y, v.z, v.w}, ms[4] = {mm.x, mm.y, mm.z, mm.w};
#pragma unroll
      for (int q = 0; q < 4; q++) {
        xo2 = fmaf(vs[q], vs[q], xo2);
        xm = fmaf(vs[q], ms[q], xm);
        xma = fmaf(fabsf(vs[q]), fabsf(ms[q]), xma);
        xb[4 * j + q] = live ? vs[q] - ms[q] : 0.f;
      }
    }
  } else {
    const float *src = samples + (size_t)(live ? s : 0) * D;
#pragma unroll
    for (int j = 0; j < NK; j++) {
      const uint32_t f = h * NK + j;
      const float v = (live && f < D) ? src[f] : 0.f;
      const float mf = (f < D) ? mu[f] : 0.f;
      xo2 = fmaf(v, v, xo2);
      xm = fmaf(v, mf, xm);
      xma = fmaf(fabsf(v), fabsf(mf), xma);
      xb[j] = (live && f < D) ? v - mf : 0.f;
    }
  }
  if (!live) xo2 = 0.f;
  float xn2 = 0.f;
#pragma unroll
  for (int j = 0; j < NK; j++) xn2 = fmaf(xb[j], xb[j], xn2);
  xn2 += __shfl_xor(xn2, 32);
  xo2 += __shfl_xor(xo2, 32);
  xm += __shfl_xor(xm, 32);
  xma += __shfl_xor(xma, 32);
  const float x0 = __shfl(xb[0], col);   // feature 0 lives in the lower half-wave (NaN - mu = NaN)

  f32x4 stage[NST];
  float bstage = 0.f;
  auto stage_load = [&](uint32_t tile) {
    const float *src = cfil + (size_t)tile * 32 * DP;
#pragma unroll
    for (int i = 0; i < NST; i++) {
      const int q = tid + i * 256;
      if (q < 8 * DP) stage[i] = reinterpret_cast<const f32x4 *>(src)[q];
    }
    if (tid < 32) bstage = bias[tile * 32 + tid];
  };
  auto stage_store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NST; i++) {
      const int q = tid + i * 256;
      if (q < 8 * DP) {
        const int row = q / (DP / 4), c4 = q % (DP / 4);
        *reinterpret_cast<f32x4 *>(tile_ptr(buf) + row * LDW + c4 * 4) = stage[i];
      }
    }
    if (tid < 32) bias_ptr(buf)[tid] = bstage;
  };

  const uint32_t ntiles = K_pad / 32;
  stage_load(0);
  stage_store(0);
  __syncthreads();
  float *srow = scores + (size_t)(live ? s : 0) * K_pad + 4 * h;
  for (uint32_t t = 0; t < ntiles; t++) {
    const int buf = t & 1;
    if (t + 1 < ntiles) stage_load(t + 1);
    f32x16 acc;
    {
      const float *bb = bias_ptr(buf) + 4 * h;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const f32x4 b4 = *reinterpret_cast<const f32x4 *>(bb + 8 * g);
        acc[4 * g + 0] = b4.x;
        acc[4 * g + 1] = b4.y;
        acc[4 * g + 2] = b4.z;
        acc[4 * g + 3] = b4.w;
      }
    }
    const float *arow = tile_ptr(buf) + col * LDW + h * NK;
#pragma unroll
    for (int j = 0; j < NK / 4; j++) {
      const f32x4 a4 = *reinterpret_cast<const f32x4 *>(arow + 4 * j);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, xb[4 * j + 0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, xb[4 * j + 1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, xb[4 * j + 2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, xb[4 * j + 3], acc, 0, 0, 0);
    }
    if (live) {
#pragma unroll
      for (int g = 0; g < 4; g++) {
        f32x4 o;
        o.x = acc[4 * g + 0];
        o.y = acc[4 * g + 1];
        o.z = acc[4 * g + 2];
        o.w = acc[4 * g + 3];
        *reinterpret_cast<f32x4 *>(srow + (size_t)t * 32 + 8 * g) = o;
      }
    }
    if (t + 1 < ntiles) stage_store(buf ^ 1);
    __syncthreads();
  }

  // the bound of lloyd_filter_kernel, without its angular tie slack: the select kernel adds its own
  const float cmaxc = sqrtf(__uint_as_float(stats[0])) * 1.000001f;
  const float bmaxc = __uint_as_float(stats[1]);
  const float cmaxo = sqrtf(__uint_as_float(stats[2])) * 1.000001f;
  const float xn = sqrtf(xn2) * 1.0001f, xo = sqrtf(xo2) * 1.0001f;
  const float e_mfma = 2.0f * eps * (xn * cmaxc + bmaxc);
  const float e_ref = 5.9604645e-8f * (12.0f * xo * cmaxo + 4.0f * cmaxo * cmaxo);
  const float thr = 2.0f * (e_mfma + e_ref) * 1.001f;
  const ClampLimits lim = clamp_limits(angular != 0, xm, dot_error(DP, xma), 0.5f * thr + kTopAcosMargin);
  if (live && h == 0) meta[s] = make_float4(thr, lim.hi, lim.lo, (x0 != x0) ? 1.f : 0.f);
}

// ---------------------------------------------------------------------------------------
// 3. assign_top_select: one wave per row of the sub-chunk.
//   pass 1  v_m = the m-th largest score among the centroids the panel holds (score > -inf), in a wave-wide sorted list
//   pass 2  the contenders -- score >= cut = min(v_m, hi) - 2E (- the acos margin), and every centroid the panel left
//           out (score -inf: a NaN / inf / overflowing centroid, which the exact key judges) -- are queued in LDS, 64
//           at a time get one exact chain per lane, and the best m by (key, index) are kept
// The row goes to the hand-over list instead (row0 + s, for assign_top_exact) when the superset argument of DESIGN.md
// 4.11 does not cover it: a NaN or +inf score or bound, angular with v_m not provably above -1, or a contender of the
// panel whose exact key does not qualify (the bound speaks of keys the reference computes without overflow).
// ---------------------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(256) void assign_top_select_kernel(
    const float *__restrict__ samples, uint32_t n, uint32_t D, const float *__restrict__ centroids,
    const float *__restrict__ csqr, uint32_t K, uint32_t K_pad, uint32_t m, const float *__restrict__ scores,
    const float4 *__restrict__ meta, uint32_t row0, uint32_t *__restrict__ top, uint32_t *__restrict__ fb_rows,
    uint32_t *__restrict__ fb_count, unsigned long long *__restrict__ evaluated) {
  __shared__ uint32_t queue_all[4][128];
  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  volatile uint32_t *queue = queue_all[wave];
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  unsigned long long keys_done = 0;
  for (uint64_t ri = (uint64_t)blockIdx.x * 4 + wave; ri < n; ri += (uint64_t)gridDim.x * 4) {
    const uint32_t s = __builtin_amdgcn_readfirstlane((uint32_t)ri);
    const float4 mt = meta[s];
    const float *sc = scores + (size_t)s * K_pad;
    const float *x = samples + (size_t)s * D;
    float lk = INFINITY;
    uint32_t li = kTopNone;
    if (mt.w != 0.f) {   // NaN first: no cluster in every slot
      top_emit(top, s, m, K, lane, li);
      continue;
    }
    // ---- pass 1: v_m ----
    float lv = -INFINITY, vm = -INFINITY;
    bool bad = !(mt.x < INFINITY);
    for (uint32_t cb = 0; cb < K; cb += 64) {
      const uint32_t c = cb + lane;
      const float v = c < K ? sc[c] : -INFINITY;
      bad = bad || v != v || v == INFINITY;
      unsigned long long mask = __ballot(v > vm);
      while (mask) {
        const int b = __builtin_ctzll(mask);
        mask &= mask - 1;
        const float vb = __shfl(v, b);
        const float up = __shfl_up(lv, 1);
        const bool front = vb > vm && vb > lv;
        const bool front_left = lane > 0 && vb > up;
        if (front) lv = front_left ? up : vb;
        vm = __shfl(lv, (int)m - 1);
      }
    }
    float cut = -INFINITY;   // fewer than m scores: every centroid is a contender
    if (vm > -INFINITY) {
      cut = fminf(vm, mt.y) - mt.x - (METRIC == 0 ? 0.f : kTopAcosMargin);
      if (METRIC != 0) bad = bad || !(vm > mt.z);
      bad = bad || cut != cut;
    }
    bool hand_over = __ballot(bad) != 0ull;
    // ---- pass 2: the contenders' exact keys ----
    if (!hand_over) {
      uint32_t qn = 0;
      bool unq = false;
      auto flush = [&](uint32_t cnt) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const bool mine = (uint32_t)lane < cnt;
        const uint32_t c = mine ? queue[lane] : 0u;
        float key = INFINITY;
        if (mine) {
          key = top_key<METRIC>(csqr[c], chain_vv<1>(x, centroids + (size_t)c * D, D));
          if (cut > -INFINITY && sc[c] > -INFINITY && !(key < kTopFltMax)) unq = true;
        }
        keys_done += cnt;
        top_admit(key, c, mine && key < kTopFltMax, m, lane, lk, li);
      };
      for (uint32_t cb = 0; cb < K; cb += 64) {
        const uint32_t c = cb + lane;
        const float v = c < K ? sc[c] : NAN;
        const bool cont = v >= cut || v == -INFINITY;
        const unsigned long long mask = __ballot(cont);
        if (!mask) continue;
        if (cont) queue[qn + (uint32_t)__popcll(mask & lt_mask)] = c;
        qn += (uint32_t)__popcll(mask);
        if (qn >= 64) {
          flush(64);
          const uint32_t rest = qn - 64;   // < 64
          const uint32_t moved = (uint32_t)lane < rest ? queue[64 + lane] : 0u;
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          if ((uint32_t)lane < rest) queue[lane] = moved;
          qn = rest;
        }
      }
      if (qn) flush(qn);
      hand_over = __ballot(unq) != 0ull;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    if (hand_over) {
      if (lane == 0) fb_rows[atomicAdd(fb_count, 1u)] = row0 + s;
    } else {
      top_emit(top, s, m, K, lane, li);
    }
  }
  if (lane == 0 && keys_done) atomicAdd(evaluated, keys_done);
}

// ---------------------------------------------------------------------------------------
// 4. assign_top_dist: dists[s * m + j] = distance(row s, centroid top[s * m + j]) in chain_vv's order, as
// assigned_distance_kernel (assign_dist.hip) computes it; NaN for "no cluster".  One thread per slot.
// ---------------------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(256) void assign_top_dist_kernel(const float *__restrict__ samples, uint64_t slots,
                                                              uint32_t D, const float *__restrict__ centroids,
                                                              uint32_t K, uint32_t m, const uint32_t *__restrict__ top,
                                                              float *__restrict__ dists) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < slots; p += (uint64_t)gridDim.x * 256) {
    const uint32_t a = top[p];
    float d = NAN;
    if (a < K) {
      const float acc = chain_vv<METRIC>(samples + (p / m) * D, centroids + (size_t)a * D, D);
      d = METRIC == 0 ? sqrtf(acc) : angular_from_prod_libm(acc);
    }
    dists[p] = d;
  }
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
hipError_t launch_assign_top_exact(int metric, const float *samples, uint32_t N, uint32_t D, const float *ct,
                                   const float *csqr, uint32_t K, uint32_t Kt, uint32_t m, const uint32_t *rows,
                                   const uint32_t *nrows, uint32_t *top, unsigned long long *evaluated,
                                   hipStream_t st) {
  if (N == 0) return hipSuccess;
  uint32_t grid = wave_row_grid(N);
  if (rows && grid > 4096u) grid = 4096u;   // a list: few rows as a rule, the grid strides over it
  return with_metric(metric, [&](auto M) {
    hipLaunchKernelGGL((assign_top_exact_kernel<M()>), dim3(grid), dim3(256), 0, st, samples, N, D, ct, csqr, K, Kt, m,
                       rows, nrows, top, evaluated);
    return hipGetLastError();
  });
}

hipError_t launch_assign_top_filter(const AssignTopFilter &a, const float *samples, uint32_t n, uint32_t row0,
                                    uint32_t *top, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const hipError_t e = with_width<FilterWidths>(a.DP, [&](auto DP) {
    return with_flag(a.D == (uint32_t)DP() && (((uintptr_t)samples) & 15u) == 0, [&](auto FAST) {
      const size_t lds_bytes = (2 * 32 * (DP() + 4) + 64) * sizeof(float);
      // (per launch: the attribute belongs to the current device's copy of the kernel)
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&assign_top_scores_kernel<DP(), FAST()>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL((assign_top_scores_kernel<DP(), FAST()>), dim3((n + 127u) / 128u), dim3(256), lds_bytes, st,
                         samples, n, a.D, a.cfil, a.bias, a.mu, a.K_pad, a.stats, a.eps, a.metric, a.scores, a.meta);
      return hipGetLastError();
    });
  });
  if (e != hipSuccess) return e;
  return with_metric(a.metric, [&](auto M) {
    hipLaunchKernelGGL((assign_top_select_kernel<M()>), dim3(wave_row_grid(n)), dim3(256), 0, st, samples, n, a.D,
                       a.centroids, a.csqr, a.K, a.K_pad, a.m, a.scores, a.meta, row0, top, a.fb_rows, a.fb_count,
                       a.evaluated);
    return hipGetLastError();
  });
}

hipError_t launch_assign_top_distances(int metric, const float *samples, uint32_t N, uint32_t D,
                                       const float *centroids, uint32_t K, uint32_t m, const uint32_t *top,
                                       float *dists, hipStream_t st) {
  if (N == 0) return hipSuccess;
  const uint64_t slots = (uint64_t)N * m, blocks = (slots + 255) / 256;
  const dim3 grid((uint32_t)(blocks < kWaveRowGridMax ? blocks : kWaveRowGridMax)), block(256);
  return with_metric(metric, [&](auto M) {
    hipLaunchKernelGGL((assign_top_dist_kernel<M()>), grid, block, 0, st, samples, slots, D, centroids, K, m, top, dists);
    return hipGetLastError();
  });
}

}  // namespace kmx
