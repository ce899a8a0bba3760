// assign_top_wide.hip -- the score kernel of kmamd_kmeans_assign_top for rows wider than 256 features.
//
// assign_top_scores_kernel (assign_top.hip) keeps 32 rows per wave resident in registers, which ends at 256 features.
// Here neither operand is resident: rows and the centred centroid panel both stream through LDS in 32-feature chunks,
// as in lloyd_wide.hip, and what leaves the kernel is what the register kernel leaves -- scores[row][K_pad] and
// meta[row] = (2E, clamp hi, clamp lo, first feature is NaN) -- so assign_top_select_kernel and everything behind it
// are shared.
//
//   block   256 threads = 4 waves, 128 rows; loops over the 128-centroid panels of K_pad
//   wave    a 64 x 64 sub-tile (rows wr * 64, centroids wc * 64) as 2 x 2 accumulators of v_mfma_f32_32x32x2_f32,
//           seeded with the bias: 64 accumulator registers
//   chunk   32 features of 128 rows (centred on their way into LDS) and of 128 panel rows, double-buffered: the next
//           chunk's 8 global 16-byte loads per thread are in flight under this chunk's 64 MFMAs per wave
//   LDS     rows of 36 words (32 + 4: 16-byte reads of 32 consecutive rows touch every bank group once);
//           2 buffers x 2 operands x 128 x 36 x 4 = 73,728 bytes: two blocks per CU
// MFMA orientation as in assign_top_scores_kernel: A = centroids, B = rows, so lane (col, h) holds for row col four
// consecutive centroids per register quad.  The contraction index is permuted inside a chunk (both operands alike): at
// step 4 j + q the lower half-wave supplies feature 4 j + q, the upper one feature 16 + 4 j + q, so that a lane reads
// 16-byte words.
// The last panel: K_pad is a multiple of 32, not of 128; its missing 32-centroid tiles are neither loaded, multiplied
// nor stored.  The row quantities of the bound (|x - mu|^2, |x|^2, x.mu, sum |x_f mu_f|) are summed by the staging
// threads while the first panel's chunks pass through, 8 threads per row.
// No floating-point atomics, no atomics at all.
#include <math.h>

#include "filter_common.hpp"
#include "kernels.hpp"

namespace kmx {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr float kTopAcosMarginWide = 1.0e-6f;   // assign_top.hip: kTopAcosMargin
constexpr int kWideChunk = 32;                  // features per chunk
constexpr int kWideLd = kWideChunk + 4;         // words per LDS row
constexpr int kWideTile = 128 * kWideLd;        // words per operand tile
constexpr size_t kWideLdsBytes = 2 * 2 * kWideTile * sizeof(float);

// one chunk of a wave's sub-tile: NT = the 32-centroid tiles of the wave that exist in this panel
template <int NT>
__device__ __forceinline__ void wide_chunk_mfma(const float *__restrict__ xt, const float *__restrict__ ct,
                                                f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const f32x4 b0 = *reinterpret_cast<const f32x4 *>(xt + 4 * j);
    const f32x4 b1 = *reinterpret_cast<const f32x4 *>(xt + 32 * kWideLd + 4 * j);
    const f32x4 a0 = *reinterpret_cast<const f32x4 *>(ct + 4 * j);
    f32x4 a1 = a0;
    if (NT > 1) a1 = *reinterpret_cast<const f32x4 *>(ct + 32 * kWideLd + 4 * j);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[q], b0[q], acc[0][0], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[q], b1[q], acc[1][0], 0, 0, 0);
      if (NT > 1) {
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[q], b0[q], acc[0][1], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[q], b1[q], acc[1][1], 0, 0, 0);
      }
    }
  }
}

// FAST: D % 4 == 0 and 16-byte aligned rows.  DPW = D rounded up to the chunk: the width of cfil's rows and of mu.
template <bool FAST>
__global__ __launch_bounds__(256, 2) void assign_top_scores_wide_kernel(
    const float *__restrict__ samples, uint32_t N, uint32_t D, uint32_t DPW, const float *__restrict__ cfil,
    const float *__restrict__ bias, const float *__restrict__ mu, uint32_t K_pad, const uint32_t *__restrict__ stats,
    float eps, int angular, float *__restrict__ scores, float4 *__restrict__ meta) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  auto rows_ptr = [&](int buf) { return lds + buf * 2 * kWideTile; };
  auto panel_ptr = [&](int buf) { return lds + buf * 2 * kWideTile + kWideTile; };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31, h = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const uint64_t row0 = (uint64_t)blockIdx.x * 128u;
  const uint32_t nch = DPW / kWideChunk, npanels = (K_pad + 127u) / 128u;

  // ---- staging: thread (sr, sf) moves features [sf, sf + 4) of tile rows sr + 32 i, of both operands ----
  const int sr = tid >> 3, sf = (tid & 7) * 4;
  f32x4 xs[4], cs[4], mus;
  float xn2[4], xo2[4], xm[4], xma[4], x0[4];
#pragma unroll
  for (int i = 0; i < 4; i++) xn2[i] = xo2[i] = xm[i] = xma[i] = x0[i] = 0.f;

  auto stage_load = [&](uint32_t panel, uint32_t ch) {
    const uint32_t f = ch * kWideChunk + sf;   // < DPW
    mus = *reinterpret_cast<const f32x4 *>(mu + f);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint64_t s = row0 + sr + 32 * i;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (s < N) {
        const float *src = samples + (size_t)s * D + f;
        if (FAST) {
          if (f < D) v = *reinterpret_cast<const f32x4 *>(src);
        } else {
#pragma unroll
          for (int q = 0; q < 4; q++)
            if (f + q < D) v[q] = src[q];
        }
      }
      xs[i] = v;
      const uint32_t c = panel * 128u + sr + 32 * i;
      f32x4 cv = {0.f, 0.f, 0.f, 0.f};
      if (c < K_pad) cv = *reinterpret_cast<const f32x4 *>(cfil + (size_t)c * DPW + f);
      cs[i] = cv;
    }
  };
  // (first: a chunk of panel 0, whose rows also feed the bound's sums; mu is zero beyond D, as the loaded row is)
  auto stage_store = [&](int buf, bool first, uint32_t ch) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const bool live = row0 + sr + 32 * i < N;
      const f32x4 v = xs[i];
      f32x4 xc;
#pragma unroll
      for (int q = 0; q < 4; q++) xc[q] = live ? v[q] - mus[q] : 0.f;
      if (first) {
        // the two norms in two levels (4 terms, then one add per chunk): a relative error of at most
        // (D / 32 + 6) 2^-24 <= 1.3e-4 at any width, half of it on the norm: inside the formulas' 1.0001
        float o2 = 0.f, n2 = 0.f;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          o2 = fmaf(v[q], v[q], o2);
          n2 = fmaf(xc[q], xc[q], n2);
          xm[i] = fmaf(v[q], mus[q], xm[i]);
          xma[i] = fmaf(fabsf(v[q]), fabsf(mus[q]), xma[i]);
        }
        xo2[i] += o2;
        xn2[i] += n2;
        if (ch == 0 && sf == 0) x0[i] = v[0];
      }
      *reinterpret_cast<f32x4 *>(rows_ptr(buf) + (sr + 32 * i) * kWideLd + sf) = xc;
      *reinterpret_cast<f32x4 *>(panel_ptr(buf) + (sr + 32 * i) * kWideLd + sf) = cs[i];
    }
  };

  // ---- the wave's tiles of a panel: how many exist, their bias into the accumulators, their scores out ----
  f32x16 acc[2][2];
  auto tiles_of = [&](uint32_t panel) -> int {
    const uint32_t c0 = panel * 128u + wc * 64u;
    return c0 >= K_pad ? 0 : (K_pad - c0 >= 64u ? 2 : 1);
  };
  auto seed = [&](uint32_t panel, int nt) {
#pragma unroll
    for (int tc = 0; tc < 2; tc++) {
      if (tc < nt) {
        const float *bb = bias + panel * 128u + wc * 64u + tc * 32u + 4 * h;
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const f32x4 b4 = *reinterpret_cast<const f32x4 *>(bb + 8 * g);
#pragma unroll
          for (int e = 0; e < 4; e++) acc[0][tc][4 * g + e] = acc[1][tc][4 * g + e] = b4[e];
        }
      }
    }
  };
  auto emit = [&](uint32_t panel, int nt) {
#pragma unroll
    for (int tr = 0; tr < 2; tr++) {
      const uint64_t s = row0 + wr * 64u + tr * 32u + col;
      if (s >= N) continue;
      float *srow = scores + (size_t)s * K_pad + panel * 128u + wc * 64u + 4 * h;
#pragma unroll
      for (int tc = 0; tc < 2; tc++) {
        if (tc < nt) {
#pragma unroll
          for (int g = 0; g < 4; g++) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; e++) o[e] = acc[tr][tc][4 * g + e];
            *reinterpret_cast<f32x4 *>(srow + tc * 32 + 8 * g) = o;
          }
        }
      }
    }
  };

  // ---- one stream of (panel, chunk) stages: load the next, multiply this one, store the next, barrier ----
  stage_load(0, 0);
  stage_store(0, true, 0);
  __syncthreads();
  uint32_t panel = 0, ch = 0;
  int buf = 0, nt = tiles_of(0);
  seed(0, nt);
  const uint32_t total = nch * npanels;
  for (uint32_t st = 0; st < total; st++) {
    const bool last_chunk = ch + 1 == nch, more = st + 1 < total;
    const uint32_t npanel = last_chunk ? panel + 1 : panel, nchunk = last_chunk ? 0 : ch + 1;
    if (more) stage_load(npanel, nchunk);
    const float *xt = rows_ptr(buf) + (wr * 64 + col) * kWideLd + h * 16;
    const float *ct = panel_ptr(buf) + (wc * 64 + col) * kWideLd + h * 16;
    if (nt == 2) wide_chunk_mfma<2>(xt, ct, acc);
    else if (nt == 1) wide_chunk_mfma<1>(xt, ct, acc);
    if (last_chunk) {
      emit(panel, nt);
      if (more) {
        nt = tiles_of(npanel);
        seed(npanel, nt);
      }
    }
    if (more) stage_store(buf ^ 1, npanel == 0, nchunk);
    __syncthreads();
    panel = npanel;
    ch = nchunk;
    buf ^= 1;
  }

  // ---- meta: the row sums live in 8 consecutive lanes; the bound of assign_top_scores_kernel, formula for formula ----
#pragma unroll
  for (int i = 0; i < 4; i++) {
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) {
      xn2[i] += __shfl_xor(xn2[i], off);
      xo2[i] += __shfl_xor(xo2[i], off);
      xm[i] += __shfl_xor(xm[i], off);
      xma[i] += __shfl_xor(xma[i], off);
    }
  }
  if (sf != 0) return;
  const float cmaxc = sqrtf(__uint_as_float(stats[0])) * 1.000001f;
  const float bmaxc = __uint_as_float(stats[1]);
  const float cmaxo = sqrtf(__uint_as_float(stats[2])) * 1.000001f;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint64_t s = row0 + sr + 32 * i;
    if (s >= N) continue;
    const float xn = sqrtf(xn2[i]) * 1.0001f, xo = sqrtf(xo2[i]) * 1.0001f;
    const float e_mfma = 2.0f * eps * (xn * cmaxc + bmaxc);
    const float e_ref = 5.9604645e-8f * (12.0f * xo * cmaxo + 4.0f * cmaxo * cmaxo);
    const float thr = 2.0f * (e_mfma + e_ref) * 1.001f;
    const ClampLimits lim =
        clamp_limits(angular != 0, xm[i], dot_error((int)DPW, xma[i]), 0.5f * thr + kTopAcosMarginWide);
    meta[s] = make_float4(thr, lim.hi, lim.lo, (x0[i] != x0[i]) ? 1.f : 0.f);
  }
}

hipError_t launch_assign_top_scores_wide(const AssignTopFilter &a, const float *samples, uint32_t n, hipStream_t st) {
  if (a.DP % kWideChunk != 0 || a.DP < a.D) return hipErrorInvalidValue;
  return with_flag((a.D & 3u) == 0 && (((uintptr_t)samples) & 15u) == 0, [&](auto FAST) {
    // (per launch: the attribute belongs to the current device's copy of the kernel)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&assign_top_scores_wide_kernel<FAST()>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWideLdsBytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((assign_top_scores_wide_kernel<FAST()>), dim3((n + 127u) / 128u), dim3(256), kWideLdsBytes, st,
                       samples, n, a.D, a.DP, a.cfil, a.bias, a.mu, a.K_pad, a.stats, a.eps, a.metric, a.scores,
                       a.meta);
    return hipGetLastError();
  });
}

}  // namespace kmx
