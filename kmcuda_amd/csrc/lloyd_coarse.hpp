// lloyd_coarse.hpp -- stage 1 of the default Lloyd assignment filter (lloyd_f16.hip has the story; reference:
// src/kmeans.cu:293-364), as a template shared by two translation units: lloyd_f16.hip instantiates the plain
// pass, lloyd_carry.hip the passes that carry per-row distance bounds from one iteration to the next -- both through
// the one launcher at the end of this file (launch_lloyd_coarse_t).
#pragma once
#include <hip/hip_fp16.h>
#include <stdlib.h>

#include "exact.hpp"
#include "filter_common.hpp"
#include "kernels.hpp"

// KMX_ABL: timing-only ablations for scripts/coarse_harness.hip (WRONG results; never defined in the library build;
// what each part of the kernel costs on one box: DESIGN.md 4.5, profiles/r6c_*).
//   1 no LDS-DMA behind super-tile 0   2 rows from 64 blocks' worth of the cache (L2 resident)   4 no bookkeeping
//   8 no decision epilogue   16 no barrier per super-tile
#ifndef KMX_ABL
#define KMX_ABL 0
#endif

namespace kmx {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------------------
// Stage 1: ONE f16 MFMA per 16 features (hi.hi only).  What shaped the kernel (DESIGN.md 4.5,
// profiles/r1e..r1k): a wave owns 64 rows (two B-operand sets) so each A fragment read from LDS feeds
// two MFMAs; blocks are 4 waves, one per SIMD, two blocks per CU, so one block's bookkeeping runs under
// the other's MFMAs; the accumulator register number travels in the low 4 mantissa bits of the score
// (<= 16 ulp, part of the bound), the tile index is noted once per tile; tiles arrive by LDS-DMA
// (global_load_lds_dwordx4: no staging registers, no ds_write issue slots) with the bank swizzle
// (16-byte chunk j of row r sits in slot j ^ (r & 15) of its half row) applied to the SOURCE address
// and again by the fragment reads.
// ---------------------------------------------------------------------------------------
template <int P>
struct TileParity { static constexpr int value = P; };   // (which of a lane's two trackers a tile's scores go into)
// hand-issued LDS fragment read + counted wait (see lloyd_coarse2_kernel)
__device__ __forceinline__ f16x8 lds_frag_issue(uint32_t addr) {
  f16x8 f;
  asm volatile("ds_read_b128 %0, %1" : "=v"(f) : "v"(addr) : "memory");
  return f;
}
template <int OFF>
__device__ __forceinline__ f16x8 lds_frag_issue_off(uint32_t addr) {   // (a constant byte offset in the instruction)
  f16x8 f;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(f) : "v"(addr), "n"(OFF) : "memory");
  return f;
}
template <int N>
__device__ __forceinline__ void lds_frag_wait(f16x8 &f) {
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(f) : "n"(N));
}
// Two 32x32x16 B fragments of a 32-row set, pieces j and j' (lane (col, h): row col, chunk (h, j)), into two 16x16x32
// ones: lanes 16-31 of the first trade places with lanes 0-15 of the second, lanes 48-63 with lanes 32-47
// (v_permlane16_swap_b32: the odd 16-lane rows of its first operand with the even rows of its second).  Afterwards the
// first holds rows 0-15, the second rows 16-31, lane (n, g) of either the k-chunk (h0, j), (h0, j'), (h1, j), (h1, j')
// for g = 0, 1, 2, 3.
__device__ __forceinline__ void frag_swap16(f16x8 &p, f16x8 &q) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4 a = __builtin_bit_cast(u32x4, p), b = __builtin_bit_cast(u32x4, q);
#pragma unroll
  for (int d = 0; d < 4; d++) {
    const auto r = __builtin_amdgcn_permlane16_swap(a[d], b[d], false, false);
    a[d] = r[0];
    b[d] = r[1];
  }
  p = __builtin_bit_cast(f16x8, a);
  q = __builtin_bit_cast(f16x8, b);
}

// 4 waves x 64 rows per block, 2 independent blocks per CU (2 x 67 KB of LDS).  (Tried and dropped:
// one 8-wave block per CU run as a ping-pong -- the waves sharing a SIMD, read from HW_ID, alternate
// MFMA and bookkeeping phases between workgroup barriers; 65 barriers per block made it 20 % slower.)
// CACHED: the B operands come from the engine's row cache (row_cache_kernel below) instead of the rows.
// NSET: 32-row operand sets per wave -- 2 up to 256 features; 1 for 512 (the halves of 64 rows x 512
// features would be the whole register file), with each A fragment feeding one MFMA again.
// SHAPE: the MFMA.  32 = v_mfma_f32_32x32x16_f16 -- a k-step is 16 features, one A fragment (32 centroids) feeds NSET
// products of 32 x 32.  16 = v_mfma_f32_16x16x32_f16 at the same wave tile (NSET 2 only: 64 rows x 32 centroids) -- a
// k-step is 32 features, two A fragments (centroids 0-15, 16-31 of the tile) feed four products of 16 x 16 each: the
// same fragment read per 64 MFMA cycles and the same 32 accumulator registers, but on random halves the chip holds a
// higher clock under its power limit with the smaller shape.  The row cache keeps the 32x32x16 operand
// order (the Yinyang sweeps read it too): the operands are rearranged in registers once per block (frag_swap16).
// CARRY (lloyd_carry.hip; 0 = the plain pass, nothing below exists in it): 1 = every row, and the pass leaves per-row
// distance bounds behind -- an upper bound of the distance to the row's centroid, a lower bound of the distance to
// every other finite centroid, both read off the best and second-best coarse scores it has anyway; 2 = the same over
// the rows of cy.row_list only (the rows whose bounds, moved by the centroids' drifts, no longer certify their
// assignment: carry_skip_kernel), gathered from the rows like stage 2 does, with the row cache's measured norms.
template <int DP, bool HALF_ROWS, bool FAST, bool CACHED, int NSET, int CARRY = 0, int SHAPE = 32>
__global__ __launch_bounds__(256, 2) void lloyd_coarse2_kernel(
    const void *__restrict__ rows, const float *__restrict__ xmeta, uint32_t N, uint32_t D, const float *__restrict__ panelhi,
    const float *__restrict__ bias, const float *__restrict__ mu, uint32_t K_pad, uint32_t K,
    const uint32_t *__restrict__ stats, float eps, float tie_slack, uint32_t *__restrict__ assignments,
    uint32_t *__restrict__ assignments_prev, uint32_t *__restrict__ undecided, float *__restrict__ und_thr,
    uint32_t *__restrict__ counters, CarryArgs cy, uint32_t *__restrict__ duo = nullptr) {
  static_assert(CARRY == 0 || CARRY == 1 || CARRY == 2, "CARRY");
  static_assert(CARRY != 2 || !CACHED, "listed rows are gathered from the rows, not streamed from the row cache");
  static_assert(SHAPE == 32 || (SHAPE == 16 && NSET == 2 && DP >= 32), "16x16x32: two row sets, 32 features per k-step");
  constexpr bool S16 = SHAPE == 16;
  constexpr int NKH = DP / 2;
  constexpr int KS = NKH / 8;               // k-steps = 16-byte chunks per half row
  constexpr int ROWB = DP * 2;              // bytes of one LDS row (DP hi halves)
  constexpr int SUPB = 64 * ROWB;           // one super-tile: 64 centroids
  constexpr int NP = SUPB / 1024;           // 1-KB LDS-DMA pieces per super-tile
  constexpr int SWM = (KS < 16 ? KS : 16) - 1;
  typedef __attribute__((address_space(3))) unsigned char lds_byte;
  extern __shared__ __attribute__((aligned(1024))) unsigned char lds2[];
  if (counters[kStopFlag] != 0u) return;   // the run has stopped on the device (apply_delta_kernel): touch nothing
  // raw LDS byte addresses (the fragment address is built with XOR: needs the 1-KB aligned base)
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_byte *)lds2;
  if (lds0 & 1023u) __builtin_trap();
  const uint32_t bias0 = lds0 + 2 * SUPB;   // 2 x 64 floats
  constexpr uint32_t BIASB = 512u;

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), col = lane & 31, h = lane >> 5;
  constexpr int WV = 4;
  constexpr bool TWO = NSET == 2;
  uint32_t total = N;
  if constexpr (CARRY == 2) total = __builtin_amdgcn_readfirstlane(*cy.n_list);
  if constexpr (CARRY != 0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (cy.host_report) {   // how long this pass's list was: the host sizes later passes by it
        volatile uint32_t *hr = cy.host_report;
        hr[0] = cy.n_list ? *cy.n_list : 0xFFFFFFFFu;   // (a pass without bounds to move has no list to report)
        hr[1] = cy.seq;
      }
      if constexpr (CARRY == 2) {   // the rows this pass does not look at (statistics: kmamd_carry_stats)
        // counters[3]: the pairs carry_skip_kernel has queued (stage 2 has not added its own yet)
        const uint32_t paired = cy.l3 ? counters[3] : 0u;
        *reinterpret_cast<unsigned long long *>(counters + kCarrySkipped) += (unsigned long long)(N - total - paired);
        *reinterpret_cast<unsigned long long *>(counters + kCarryPaired) += (unsigned long long)paired;
      }
    }
  }
  if constexpr (CARRY == 2) {
    if (blockIdx.x * (128u * NSET) >= total) return;   // (block-uniform, in front of every barrier and DMA)
  }
  // The listed pass's grid follows the host's ESTIMATE of the list (an earlier pass's length): the blocks stride over
  // the list, whose length only the device knows -- a cluster that dies, say, "drifts" by its whole centred norm (its
  // zeroed panel row against the old one: the maximum drift every row is charged; a drift that is not finite counts as
  // +inf) and can list every row in one pass, its own rows always (carry_skip_kernel: finite[a]).
  // Every other instantiation makes one trip (its block index is its 128 NSET rows).
  for (uint32_t blk = blockIdx.x;;) {
  blk = __builtin_amdgcn_readfirstlane(blk);
  const uint32_t posA = blk * (128u * NSET) + wave * (32u * NSET) + col, posB = posA + 32u;
  const bool liveA = posA < total, liveB = TWO && posB < total;
  uint32_t sA = posA, sB = posB;
  if constexpr (CARRY == 2) {
    sA = liveA ? cy.row_list[posA] : 0u;
    sB = liveB ? cy.row_list[posB] : 0u;
  }

  f16x8 xa[KS], xb[TWO ? KS : 1];
  float xn2a = 0.f, x0a = 0.f, xn2b = 0.f, x0b = 0.f;
  // x.mu and sum |x_f mu_f| per row: score + x.mu = the product, which the angular metric clamps (filter_common.hpp)
  float xdma = 0.f, xdmb = 0.f, xaba = 0.f, xabb = 0.f;
  // both rows of a lane per k-step, sharing the mean chunk.  Lanes without a row read row 0: an MFMA
  // column only feeds its own outputs and theirs are never committed, so nothing is masked.
  auto load_chunk = [&](uint32_t s, bool live, int j, float (&xv)[8]) {
    const size_t row = (size_t)(live ? s : 0);
    if (FAST && HALF_ROWS) {
      const f16x8 raw = reinterpret_cast<const f16x8 *>(reinterpret_cast<const _Float16 *>(rows) + row * DP + h * NKH)[j];
#pragma unroll
      for (int q = 0; q < 8; q++) xv[q] = (float)raw[q];
    } else if (FAST) {
      const f32x4 *src = reinterpret_cast<const f32x4 *>(reinterpret_cast<const float *>(rows) + row * DP + h * NKH);
      const f32x4 a = src[2 * j], b = src[2 * j + 1];
      xv[0] = a.x; xv[1] = a.y; xv[2] = a.z; xv[3] = a.w;
      xv[4] = b.x; xv[5] = b.y; xv[6] = b.z; xv[7] = b.w;
    } else {
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const uint32_t f = h * NKH + 8 * j + q;
        float v = 0.f;
        if (f < D) v = HALF_ROWS ? (float)reinterpret_cast<const _Float16 *>(rows)[row * D + f]
                                 : reinterpret_cast<const float *>(rows)[row * D + f];
        xv[q] = v;
      }
    }
  };
  auto centre = [&](const float (&xv)[8], const float (&mm)[8], f16x8 &hi, float &xn2) {
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const float xc = xv[q] - mm[q];
      hi[q] = (_Float16)xc;
      xn2 = fmaf(xc, xc, xn2);
    }
  };
  // Rows arrive in at most two batches of 8 k-steps, every load of a batch issued before the first
  // use: issued k-step by k-step the prologue is 8 dependent HBM round trips (~20 us of an 80-us
  // block), and the other block's LDS-DMA pieces queue behind those misses in the in-order texture path.
  // The mean comes from LDS (staged by DMA with super-tile 0): an ordinary global load would drain vmcnt.
  constexpr int BJ = KS > 8 ? 8 : KS;
  const uint32_t mu_lds = bias0 + BIASB + 64;
  auto load_rows = [&]() {
    if constexpr (CACHED) {
      // rows = the row cache: per 32-row block KS pieces of 64 lanes x 16 bytes, already centred halves
      // in operand order -> 2 KS fully coalesced 1-KB loads per wave straight into the operand
      // registers, no conversion; the norms wait in xmeta until the decision
      const f16x8 *c = reinterpret_cast<const f16x8 *>(rows) + ((size_t)((KMX_ABL & 2) ? (blockIdx.x & 63u) : blockIdx.x) * (4 * NSET) + wave * NSET) * (KS * 64) + lane;
#pragma unroll
      for (int j = 0; j < KS; j++) xa[j] = c[j * 64];
#pragma unroll
      for (int j = 0; j < (TWO ? KS : 0); j++) xb[j] = c[(KS + j) * 64];
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      return;
    }
#pragma unroll
    for (int j0 = 0; j0 < KS; j0 += BJ) {
      float va[BJ][8], vb[TWO ? BJ : 1][8];
#pragma unroll
      for (int jj = 0; jj < BJ; jj++) load_chunk(sA, liveA, j0 + jj, va[jj]);
#pragma unroll
      for (int jj = 0; jj < (TWO ? BJ : 0); jj++) load_chunk(sB, liveB, j0 + jj, vb[jj]);
      __builtin_amdgcn_sched_barrier(0);
      if (j0 == 0) {  // the mean (and super-tile 0) landed, visible to every wave
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
#pragma unroll
      for (int jj = 0; jj < BJ; jj++) {
        const int j = j0 + jj;
        float mm[8];
        const f32x4 m0 = *reinterpret_cast<const __attribute__((address_space(3))) f32x4 *>((uintptr_t)(mu_lds + (h * NKH + 8 * j) * 4));
        const f32x4 m1 = *reinterpret_cast<const __attribute__((address_space(3))) f32x4 *>((uintptr_t)(mu_lds + (h * NKH + 8 * j + 4) * 4));
        mm[0] = m0.x; mm[1] = m0.y; mm[2] = m0.z; mm[3] = m0.w;
        mm[4] = m1.x; mm[5] = m1.y; mm[6] = m1.z; mm[7] = m1.w;
        centre(va[jj], mm, xa[j], xn2a);
        if constexpr (TWO) centre(vb[jj], mm, xb[j], xn2b);
        if (j == 0) { x0a = va[0][0]; if constexpr (TWO) x0b = vb[0][0]; }
        asm volatile("" : "+v"(xa[j]));  // convert NOW: hipcc parks the fp32 values in scratch otherwise
        if constexpr (TWO) asm volatile("" : "+v"(xb[j]));
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    xn2a += __shfl_xor(xn2a, 32); x0a = __shfl(x0a, col);
    xn2b += __shfl_xor(xn2b, 32); x0b = __shfl(x0b, col);
  };

  // ---- LDS-DMA staging of super-tile sp into buffer buf ----
  const uint32_t nsuper = (K_pad + 63) / 64;
  const float *biashi = reinterpret_cast<const float *>(reinterpret_cast<const unsigned char *>(panelhi) + (size_t)nsuper * SUPB);
  // linear byte P of the super-tile image lands in LDS at P; it is fetched from source byte
  // P ^ (((P / ROWB) & SWM) << 4): the 16-byte chunk index XORed with the row's low bits (inside a
  // half row, SWM < KS).  Recomputed per piece from one opaque register -- as loop invariants the
  // per-piece addresses cost 30 VGPRs the MFMA loop needs.
  auto stage_piece = [&](uint32_t sp, int buf, int p) {
    uint32_t P0 = (uint32_t)lane * 16u;
    asm volatile("" : "+v"(P0));
    const unsigned char *src = reinterpret_cast<const unsigned char *>(panelhi) + (size_t)sp * SUPB;
    const uint32_t P = (uint32_t)p * 1024u + P0;
    const uint32_t from = P ^ (((P / ROWB) & SWM) << 4);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + from),
                                     (__attribute__((address_space(3))) void *)(uintptr_t)(lds0 + buf * SUPB + p * 1024), 16, 0, 0);
  };
  // the 64 biases of the super-tile (clamped copy behind the panel): one 4-byte DMA.  No ordinary
  // global load lives in the loop: hipcc waits vmcnt(0) at its first use, draining the DMA
  const uint32_t mybias = bias0;
  auto stage_bias = [&](uint32_t sp, int buf) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(biashi + sp * 64u + lane),
                                     (__attribute__((address_space(3))) void *)(uintptr_t)(mybias + buf * 256), 4, 0, 0);
  };
  auto stage_issue = [&](uint32_t sp, int buf, int nw, int me) {   // nw waves share the pieces, I am number me
    for (int p = me; p < NP; p += nw) stage_piece(sp, buf, p);
    if (me == 0) stage_bias(sp, buf);
  };

  {  // the mean -> LDS: DP floats = DP / 4 sixteen-byte lanes
    constexpr int MUP = (DP * 4 + 1023) / 1024;   // 1-KB pieces
    if (wave < MUP && lane * 16 < DP * 4 - wave * 1024)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(reinterpret_cast<const unsigned char *>(mu) + wave * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void *)(uintptr_t)(mu_lds + wave * 1024), 16, 0, 0);
  }
  stage_issue(0, 0, WV, wave);
  load_rows();   // waits for the DMA above and closes with a barrier after its first batch
  if constexpr (S16) {   // 16x16x32: xa[2 p + R] / xb[2 p + R] = rows 16 R .. 16 R + 15 of set A / B at k-step p
#pragma unroll
    for (int p = 0; p < KS / 2; p++) {
      frag_swap16(xa[2 * p], xa[2 * p + 1]);
      frag_swap16(xb[2 * p], xb[2 * p + 1]);
    }
  }

  // FOUR top-2 trackers per row, not two: a lane keeps one for the even tiles and one for the odd tiles (the two
  // halves of the wave see different centroids of a tile anyway).  Same work per score -- a tile's scores go into
  // its parity's tracker -- and at the end the best of every quarter is known WITH its index: when the row's
  // contenders sit in different quarters (3 cases of 4), stage 2 need not sweep the centroids again to find them.
  float v1a[2] = {-INFINITY, -INFINITY}, v2a[2] = {-INFINITY, -INFINITY}, v1b[2] = {-INFINITY, -INFINITY}, v2b[2] = {-INFINITY, -INFINITY};
  uint32_t tba[2] = {0, 0}, tbb[2] = {0, 0};
  // 16x16x32: ONE tracker per row, four rows per lane -- lane (n, g) = (lane & 15, lane >> 4) holds row n of the wave's
  // 16-row blocks q = 0..3 (set A: 0, 1; set B: 2, 3) and sees centroids 4g..4g+3 and 16+4g..16+4g+3 of every tile, so
  // the four lane groups are the four quarters
  float w1[4], w2[4];   // (unused by 32x32x16)
  uint32_t wt[4];
#pragma unroll
  for (int q = 0; q < 4; q++) { w1[q] = w2[q] = -INFINITY; wt[q] = 0; }
  // fragment address of k-step j: rowbase ^ swizzle ^ (16 j); (row, half) part fixed per lane.  16x16x32: lane (m, g)
  // reads centroid m (of the half tile) at the chunk its lane group holds in B -- half g >> 1, chunk 2 p + (g & 1) of
  // k-step p: rowbase ^ swizzle ^ (32 p); sixteen lanes read one chunk of 16 rows, 16 distinct 16-byte slots
  const uint32_t fragbase =
      S16 ? lds0 + (uint32_t)(lane & 15) * ROWB + (uint32_t)h * (KS * 16) + (uint32_t)(((((lane >> 4) & 1) ^ (lane & 15)) & SWM) * 16)
          : lds0 + (uint32_t)col * ROWB + (uint32_t)h * (KS * 16) + (uint32_t)((col & SWM) * 16);
  // max(v1, pk) as med3(v1, pk, +inf): fmaxf() costs a canonicalising v_max per operand on top
  float pinf = INFINITY;
  asm volatile("" : "+s"(pinf));
  auto pack = [&](float v, int r) { return __uint_as_float((__float_as_uint(v) & 0xFFFFFFF0u) | (uint32_t)r); };
  // two scores at once: the new second = max(second, median(best, a, b)), the new best = max3(best, a, b):
  // 3 ops for the pair + 2 packs.  v_max3 only sees PACKED values (results of VALU ops the compiler
  // scheduled itself), never an MFMA result: the MFMA -> VALU read hazard stays the compiler's business
  auto book2 = [&](float a, float b, int r, float &v1, float &v2) {
    const float pa = pack(a, r), pb = pack(b, r + 1);
    const float m = __builtin_amdgcn_fmed3f(v1, pa, pb);
    v2 = __builtin_amdgcn_fmed3f(v2, m, pinf);
    float t;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(t) : "v"(v1), "v"(pa), "v"(pb));
    v1 = t;
  };
  auto lds_f4 = [](uint32_t addr) {
    return *reinterpret_cast<const __attribute__((address_space(3))) f32x4 *>((uintptr_t)addr);
  };
  auto load_bias = [&](uint32_t biasaddr, f32x16 &b) {
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const f32x4 b4 = lds_f4(biasaddr + (8 * g + 4 * h) * 4);
      b[4 * g + 0] = b4.x; b[4 * g + 1] = b4.y; b[4 * g + 2] = b4.z; b[4 * g + 3] = b4.w;
    }
  };
  // One tile: 2 x KS MFMAs (each A fragment feeds both row sets), then the top-2 bookkeeping of its
  // 2 x 16 scores on the VALU.  The two waves a SIMD holds belong to DIFFERENT blocks (4 waves per
  // block, one per SIMD), so they are not in step: one's bookkeeping runs under the other's MFMAs.
  // (Double-buffered accumulators with the bookkeeping interleaved in-wave need ~230 registers: the
  // B operands spill, measured slower.)
  // Fragment reads are issued by hand, PD k-steps ahead, with counted waits: while an LDS-DMA is in
  // flight hipcc turns every wait on a fragment into lgkmcnt(0), i.e. it waits for the read it
  // has just issued.  (LDS returns in order: lgkmcnt(n) = all but the youngest n reads landed.)
  constexpr int PD = KS <= 3 ? KS - 1 : 3;   // (every other depth spills the B operands at D = 256)
  auto frag_wait = [&](int j, f16x8 &f) {
    constexpr int kMaxBehind = PD;
    const int behind = (KS - 1 - j) < kMaxBehind ? (KS - 1 - j) : kMaxBehind;  // younger reads in flight
    if (behind == 7) lds_frag_wait<7>(f);
    else if (behind == 6) lds_frag_wait<6>(f);
    else if (behind == 5) lds_frag_wait<5>(f);
    else if (behind == 4) lds_frag_wait<4>(f);
    else if (behind == 3) lds_frag_wait<3>(f);
    else if (behind == 2) lds_frag_wait<2>(f);
    else if (behind == 1) lds_frag_wait<1>(f);
    else lds_frag_wait<0>(f);
  };
  // the next super-tile's LDS-DMA pieces, one at a time in the shadow of the MFMAs: issued
  // back to back the four waves' 32 pieces queue up in the texture path and hold up the wave
  // (all of them during the super-tile's FIRST tile: the second one's 32 MFMAs cover the flight.  Issued from
  // the bookkeeping phase instead -- the other block's MFMAs would cover the issue -- the kernel is 2 % slower:
  // 3.51 against 3.44 ms on the same box, profiles/r3d_*)
  auto stage_after = [&](int j, bool stage, uint32_t sp_next, int buf_next) {
    constexpr int SPREAD = KS >= 8 ? KS / 8 : 1;            // a piece every SPREAD k-steps
    if (!(KMX_ABL & 1) && stage && (j % SPREAD) == SPREAD / 2 && j / SPREAD < 8) {
      const int slot = j / SPREAD;                           // 0..7
      for (int p = slot * 4 + wave; p < NP; p += 32) stage_piece(sp_next, buf_next, p);
      if (slot == 0 && wave == 0) stage_bias(sp_next, buf_next);
    }
  };
  // 16x16x32: the same LDS reads (KS per tile, read j = half tile j & 1 of k-step j >> 1), each feeding four products
  // of 16 cycles (the wave's four 16-row blocks) instead of two of 32; accumulator i of half tile b in lane group g is
  // centroid 16 b + 4 g + i, packed as index 4 b + i
  auto tile_pass16 = [&](uint32_t ldsbase, uint32_t biasaddr, uint32_t t, bool stage, uint32_t sp_next, int buf_next) {
    const int g = lane >> 4;
    f32x4 acc[2][4];
#pragma unroll
    for (int b = 0; b < 2; b++) {
      const f32x4 b4 = lds_f4(biasaddr + (16 * b + 4 * g) * 4);
#pragma unroll
      for (int q = 0; q < 4; q++) acc[b][q] = b4;
    }
    uint32_t fb = fragbase + ldsbase;
    asm volatile("" : "+v"(fb));
    auto issue = [&](int j) {   // (half tile 1 sits 16 rows further: the instruction's offset)
      const uint32_t a = fb ^ (uint32_t)((j >> 1) * 32);
      return (j & 1) ? lds_frag_issue_off<16 * ROWB>(a) : lds_frag_issue(a);
    };
    f16x8 fr[PD + 1];
#pragma unroll
    for (int j = 0; j < PD; j++) fr[j] = issue(j);
#pragma unroll
    for (int j = 0; j < KS; j++) {
      if (j + PD < KS) fr[(j + PD) % (PD + 1)] = issue(j + PD);
      f16x8 &f = fr[j % (PD + 1)];
      frag_wait(j, f);
      const int b = j & 1, p = j >> 1;
      acc[b][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f, xa[2 * p], acc[b][0], 0, 0, 0);
      acc[b][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f, xa[2 * p + 1], acc[b][1], 0, 0, 0);
      acc[b][2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f, xb[2 * p], acc[b][2], 0, 0, 0);
      acc[b][3] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f, xb[2 * p + 1], acc[b][3], 0, 0, 0);
      stage_after(j, stage, sp_next, buf_next);
    }
    float w1_in[4];
#pragma unroll
    for (int q = 0; q < 4; q++) w1_in[q] = w1[q];
    if (KMX_ABL & 4) {
#pragma unroll
      for (int q = 0; q < 4; q++) { w1[q] = fmaxf(w1[q], acc[0][q][0]); w2[q] = fmaxf(w2[q], acc[1][q][3]); }
    } else {
#pragma unroll
      for (int b = 0; b < 2; b++)
#pragma unroll
        for (int i = 0; i < 4; i += 2)
#pragma unroll
          for (int q = 0; q < 4; q++) book2(acc[b][q][i], acc[b][q][i + 1], 4 * b + i, w1[q], w2[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; q++) wt[q] = (w1[q] != w1_in[q]) ? t : wt[q];
  };
  auto tile_pass = [&](uint32_t ldsbase, uint32_t biasaddr, uint32_t t, bool stage, uint32_t sp_next, int buf_next, auto parity) {
    constexpr int PAR = decltype(parity)::value;
    if constexpr (S16) {
      tile_pass16(ldsbase, biasaddr, t, stage, sp_next, buf_next);
      return;
    }
    f32x16 accA, accB;
    load_bias(biasaddr, accA);
    accB = accA;
    // (the 1-KB aligned tile base adds into bits the XOR never touches.)  Opaque on purpose: left
    // visible, the KS addresses are hoisted out of the tile loop and the B operands spill instead
    uint32_t fb = fragbase + ldsbase;
    asm volatile("" : "+v"(fb));
    f16x8 fr[PD + 1];
#pragma unroll
    for (int j = 0; j < PD; j++) fr[j] = lds_frag_issue(fb ^ (uint32_t)(j * 16));
#pragma unroll
    for (int j = 0; j < KS; j++) {
      if (j + PD < KS) fr[(j + PD) % (PD + 1)] = lds_frag_issue(fb ^ (uint32_t)((j + PD) * 16));
      f16x8 &f = fr[j % (PD + 1)];
      frag_wait(j, f);
      accA = __builtin_amdgcn_mfma_f32_32x32x16_f16(f, xa[j], accA, 0, 0, 0);
      if constexpr (TWO) accB = __builtin_amdgcn_mfma_f32_32x32x16_f16(f, xb[j], accB, 0, 0, 0);
      stage_after(j, stage, sp_next, buf_next);
    }
    const float v1a_in = v1a[PAR], v1b_in = v1b[PAR];
    if (KMX_ABL & 4) {
      v1a[PAR] = fmaxf(v1a[PAR], accA[0]); v2a[PAR] = fmaxf(v2a[PAR], accA[15]);
      if constexpr (TWO) { v1b[PAR] = fmaxf(v1b[PAR], accB[0]); v2b[PAR] = fmaxf(v2b[PAR], accB[15]); }
    } else {
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        book2(accA[r], accA[r + 1], r, v1a[PAR], v2a[PAR]);
        if constexpr (TWO) book2(accB[r], accB[r + 1], r, v1b[PAR], v2b[PAR]);
      }
    }
    tba[PAR] = (v1a[PAR] != v1a_in) ? t : tba[PAR];
    tbb[PAR] = (v1b[PAR] != v1b_in) ? t : tbb[PAR];
  };

  for (uint32_t sp = 0; sp < nsuper; sp++) {
    const int buf = sp & 1;
    const bool stage = sp + 1 < nsuper;
    const uint32_t base = buf * SUPB, bb = mybias + buf * 256;
    tile_pass(base, bb, 2 * sp, stage, sp + 1, buf ^ 1, TileParity<0>());
    tile_pass(base + 32 * ROWB, bb + 128, 2 * sp + 1, false, sp + 1, buf ^ 1, TileParity<1>());
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (!(KMX_ABL & 16)) __syncthreads();
  }
  if (KMX_ABL & 8) {   // (keep the sweep alive, skip the epilogue)
    float keep = 0.f;
    uint32_t keept = 0;
#pragma unroll
    for (int q = 0; q < (S16 ? 4 : 1); q++) { keep += w1[q] + w2[q]; keept += wt[q]; }
    if (v1a[0] + v2a[0] + v1b[0] + v2b[0] + v1a[1] + v2a[1] + v1b[1] + v2b[1] + keep == 1.2345f) assignments[0] = tba[0] + tbb[0] + tba[1] + tbb[1] + keept;
    return;
  }

  // |coarse score - reference score| <= E_c: the f32-accumulated hi.hi products (gamma_{DP+1}), the
  // dropped lo terms (|a_lo| <= 2^-11 |a|: (2^-10 + 2^-22) ||x'|| C'max), half underflow, the 4 index
  // bits packed into each score (<= 16 ulp of a score of magnitude <= ||x'|| C'max (1 + 2^-10) +
  // B'max), + E_ref.  Rows or panels with a centred norm near the half range could hold inf halves:
  // never decided here.
  const float cmaxc = sqrtf(__uint_as_float(stats[0])) * 1.000001f;
  const float bmaxc = __uint_as_float(stats[1]);
  const float cmaxo = sqrtf(__uint_as_float(stats[2])) * 1.000001f;
  const float mu_norm = (CACHED || CARRY == 2) ? xmeta[2 * (((size_t)N + 255) / 256 * 256)] : cmaxo;
  const float dcmax = sqrtf(__uint_as_float(stats[5])) * 1.000001f;   // max ||c' - hi(c')||; inf = no bound
  const float u = 5.9604645e-8f;
  uint32_t und_count = 0, changed_count = 0, duo_count = 0;
  unsigned long long uma = 0, umb = 0, dma = 0, dmb = 0;
  bool unda = false, undb = false, duoa = false, duob = false;
  uint32_t d1a = 0, d2a = 0, d1b = 0, d2b = 0;
  float dra = 0.f, drb = 0.f;
  // rows whose contenders are known by index (DUO) leave on a list of their own (lloyd_duo.hip; in a carried pass the
  // duo kernel also leaves the bounds / pair certificates stage 2 would have: the record carries the best score of
  // all the other centroids)
  const bool want_duo = duo != nullptr;
  const bool angular = tie_slack > 0.f;   // (engine.cpp: the angular metric's plateau slack; 0 under L2)
  // xdm = x.mu, xab >= sum |x_f mu_f| (< 0: not summed here -- the row cache's record: ||x|| ||mu|| bounds it)
  // the four quarters' bests of a row with their centroids; everything else the row has seen scored at most `others`.
  // 32x32x16: the quarters are (even / odd tiles) x (half-wave), the row's two lanes col and col + 32
  auto quarters32 = [&](const float (&q1)[2], const float (&q2)[2], const uint32_t (&qt)[2], float (&kq)[4],
                        uint32_t (&jq)[4], float &others) {
    auto index_of = [&](float v, uint32_t tb, uint32_t hh) {
      const uint32_t r = __float_as_uint(v) & 15u;
      return tb * 32u + (r & 3u) + 8u * (r >> 2) + 4u * hh;
    };
    kq[0] = q1[0]; kq[1] = q1[1]; kq[2] = __shfl_xor(q1[0], 32); kq[3] = __shfl_xor(q1[1], 32);
    jq[0] = index_of(kq[0], qt[0], h); jq[1] = index_of(kq[1], qt[1], h);
    jq[2] = __shfl_xor(jq[0], 32); jq[3] = __shfl_xor(jq[1], 32);
    const float mine2 = fmaxf(q2[0], q2[1]);
    others = fmaxf(mine2, __shfl_xor(mine2, 32));
  };
  // 16x16x32: the quarters are the four lane groups.  Transposed so that every lane finishes ONE row: lane (n, g) takes
  // row block g (wave row 16 g + n = set h, row col -- its own lane in the 32x32x16 layout of the row state), and round
  // r brings in quarter g ^ r: every lane sends the tracker of block (its g) ^ r to lane xor 16 r
  auto quarters16 = [&](float (&kq)[4], uint32_t (&jq)[4], float &others) {
    const int g = lane >> 4;
    float o[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int gq = g ^ r;
      auto pick = [&](const auto (&a)[4]) {
        const auto lo = (gq & 1) ? a[1] : a[0], hi = (gq & 1) ? a[3] : a[2];
        return (gq & 2) ? hi : lo;
      };
      float v = pick(w1), v2 = pick(w2);
      uint32_t tb = pick(wt);
      if (r) { v = __shfl_xor(v, 16 * r); v2 = __shfl_xor(v2, 16 * r); tb = __shfl_xor(tb, 16 * r); }
      const uint32_t ri = __float_as_uint(v) & 15u;   // 4 b + i
      kq[r] = v;
      o[r] = v2;
      jq[r] = tb * 32u + 16u * (ri >> 2) + 4u * (uint32_t)gq + (ri & 3u);
    }
    others = fmaxf(fmaxf(o[0], o[1]), fmaxf(o[2], o[3]));
  };
  auto finish = [&](uint32_t s, bool mine, const float (&kq)[4], const uint32_t (&jq)[4], float others, float xn2,
                    float x0, float dx2, float xdm, float xab, bool &und, unsigned long long &um, float &cut, bool &is_duo,
                    unsigned long long &dm, uint32_t &dc1, uint32_t &dc2, float &drest) {
    const bool insane = (x0 != x0);  // kmeans.cu:312
    // the four quarters' bests, sorted
    float k0 = kq[0], k1 = kq[1], k2 = kq[2], k3 = kq[3];
    uint32_t j0 = jq[0], j1 = jq[1], j2 = jq[2], j3 = jq[3];
    auto order = [](float &a, uint32_t &ia, float &b, uint32_t &ib) {   // a >= b afterwards (a stays in front on ties)
      const bool g = b > a;
      const float ta = g ? b : a, tb2 = g ? a : b;
      const uint32_t ja = g ? ib : ia, jb = g ? ia : ib;
      a = ta; b = tb2; ia = ja; ib = jb;
    };
    order(k0, j0, k1, j1); order(k2, j2, k3, j3); order(k0, j0, k2, j2); order(k1, j1, k3, j3); order(k1, j1, k2, j2);
    float v1 = k0;
    const uint32_t i1 = j0;
    const float v2 = fmaxf(k1, others);   // the row's second-best coarse score
    // ||x|| <= ||x'|| + ||mu||, and ||mu|| <= Cmax while mu is the mean of the current centroids
    // (with the row cache mu is frozen: its norm is stored behind the per-row records)
    const float xn = sqrtf(xn2) * 1.0001f, xo = (xn + mu_norm) * 1.0001f;
    // operand rounding: x'.c' - hi(x').hi(c') = x'.dc + dx.c' - dx.dc with dx = x' - hi(x'), dc likewise,
    // bounded by Cauchy-Schwarz on MEASURED residual norms (row cache / centroid_panelhi_kernel; about
    // half the worst case 2^-11 ||.||, which the uncached path uses for its rows)
    const float dx = dx2 >= 0.f ? sqrtf(dx2) * 1.0001f : 4.8829e-4f * xn;
    const float e_c = 2.0f * eps * (xn * cmaxc + bmaxc) + (xn * dcmax + dx * cmaxc + dx * dcmax) * 1.001f +
                      6e-8f * sqrtf((float)DP) * (xn + cmaxc) + 2.0e-6f * (1.001f * xn * cmaxc + bmaxc);
    const float e_ref = u * (12.0f * xo * cmaxo + 4.0f * cmaxo * cmaxo);
    const float thr = 2.0f * (e_c + e_ref) * 1.001f + tie_slack;
    const bool in_range = (xn < 6.0e4f) && (cmaxc < 6.0e4f) && (v1 > -1.0e38f) && (i1 < K);
    // angular: no centroid but the best may reach the clamp at product 1, the best not the one at -1 (filter_common.hpp)
    const ClampLimits lim = clamp_limits(angular, xdm, dot_error(DP, xab >= 0.f ? xab : xo * mu_norm), 0.5f * thr);
    const bool certain = insane || (in_range && ((v1 - v2) > thr) && (v2 < lim.hi) && (v1 > lim.lo));  // NaN anywhere => not certain
    bool changed = false;
    if (mine && certain) changed = commit_row(s, insane ? K : i1, assignments, assignments_prev);
    und = mine && !certain;
    is_duo = false;
    {
      // undecided, a usable cut-off (below), and only the two best quarters' bests reach it: stage 2's answer -- the
      // contenders are j0 and j1 -- without its sweep.  (The scores compared are the packed ones stage 1 decides on
      // itself: e_c covers the index bits.)
      float c0 = in_range ? v1 - thr : __builtin_nanf("");
      if (angular) c0 = (lim.hi == lim.hi) ? fminf(c0, lim.hi) : __builtin_nanf("");
      is_duo = want_duo && und && (k1 >= c0) && (k2 < c0) && (others < c0) && (j1 < K);   // (NaN cut-off: no)
      if (is_duo) und = false;
      dc1 = j0; dc2 = j1; drest = fmaxf(k2, others);
    }
    if constexpr (CARRY != 0) {
      // d(x, c)^2 = ||x - mu||^2 - 2 s(c) with s(c) the exact score; |v - s(c)| <= e_c for every centroid (packed
      // index bits included), xn2 within 2 eps of ||x - mu||^2 (an fp32 sum of DP squares of rounded differences).
      // Every centroid other than i1 scored <= v2.  A row that stage 2 / the settle kernels decide may end on another
      // contender than i1: its lower bound is void (0: the next pass looks at it again); ub stays valid, the final
      // centroid being the reference's nearest (carried bounds).
      if (mine && cy.angular) {
        // the certified gap of the scores (= products up to a term constant in c): what is left of it after the
        // centroids' moves is what carry_skip_kernel tests
        // (and the room of the others' products below 1 / of the best one's above -1, which the same drifts use up:
        //  carry_skip_kernel charges the two sides' moves separately, each at least 0)
        const float e = e_c * 1.001f;
        float gapv = (certain && !insane && in_range)
                         ? fminf(fminf((v1 - e) - (v2 + e), lim.hi - v2), v1 - lim.lo) * 0.999999f : -INFINITY;
        if (!(gapv == gapv)) gapv = -INFINITY;
        cy.ub[s] = gapv;
        if (cy.l3) cy.l3[s] = 0.f;   // (no pair statement)
      } else if (mine) {
        float ubv = INFINITY, lbv = 0.f;
        if (!insane && in_range) {
          const float e = e_c * 1.001f;
          const float d2u = fmaxf(xn2 * (1.0f + 2.0f * eps) - 2.0f * (v1 - e), 0.f);
          const float d2l = xn2 * (1.0f - 2.0f * eps) - 2.0f * (v2 + e);
          const float geo = 2.4e-7f * (xn + cmaxc);
          ubv = sqrtf(d2u) * 1.000001f + geo;
          if (certain && d2l > 0.f) lbv = fmaxf(sqrtf(d2l) * 0.999999f - geo, 0.f);
          if (!(ubv == ubv)) ubv = INFINITY;
          if (!(lbv == lbv)) lbv = 0.f;
        }
        cy.ub[s] = ubv;
        cy.lb[s] = lbv;
        if (cy.l3) cy.l3[s] = 0.f;   // (no pair statement; stage 2 writes one for the rows it settles between two)
      }
    }
    // what the refine stage may drop: a centroid whose coarse score is below best - thr cannot be the
    // reference's nearest (both scores are within thr / 2 of the reference's); NaN = no such statement
    // (angular: nor one whose product may reach 1 -- every such centroid ties with the best at distance 0)
    cut = in_range ? v1 - thr : __builtin_nanf("");
    if (angular) cut = (lim.hi == lim.hi) ? fminf(cut, lim.hi) : __builtin_nanf("");
    const unsigned long long cm = __ballot(changed);
    um = __ballot(und);
    dm = __ballot(is_duo);
    changed_count += (uint32_t)__popcll(cm);
    und_count += (uint32_t)__popcll(um);
    duo_count += (uint32_t)__popcll(dm);
  };
  float dx2a = -2.f, dx2b = -2.f;   // -2: not measured (no row cache) -> the worst case 2^-11 ||x'||
  if constexpr (CACHED || CARRY == 2) {   // (the listed pass runs beside a valid row cache: its records hold for these rows)
    const float2 ma = reinterpret_cast<const float2 *>(xmeta)[sA], mb = reinterpret_cast<const float2 *>(xmeta)[TWO ? sB : sA];
    xn2a = ma.x; dx2a = ma.y; xn2b = mb.x; dx2b = mb.y;
    x0a = (ma.y == -1.f) ? __builtin_nanf("") : 0.f;
    x0b = (mb.y == -1.f) ? __builtin_nanf("") : 0.f;
    xaba = xabb = -1.f;
    if (angular) {   // x.mu: the third table of the row cache (row_cache_kernel)
      const float *xdot = xmeta + 2 * (((size_t)N + 255) / 256 * 256) + 2;
      xdma = xdot[sA];
      xdmb = xdot[TWO ? sB : sA];
    }
  } else if (angular) {   // no record: the rows once more (a loop of its own, the L2 passes keep their registers)
    const uint32_t fb = (uint32_t)(h * NKH), fe = min(fb + (uint32_t)NKH, D);
    if (fb < fe) {
      if constexpr (HALF_ROWS) {
        row_dot_mu(reinterpret_cast<const _Float16 *>(rows) + (size_t)(liveA ? sA : 0u) * D, mu, fb, fe, xdma, xaba);
        if constexpr (TWO) row_dot_mu(reinterpret_cast<const _Float16 *>(rows) + (size_t)(liveB ? sB : 0u) * D, mu, fb, fe, xdmb, xabb);
      } else {
        row_dot_mu(reinterpret_cast<const float *>(rows) + (size_t)(liveA ? sA : 0u) * D, mu, fb, fe, xdma, xaba);
        if constexpr (TWO) row_dot_mu(reinterpret_cast<const float *>(rows) + (size_t)(liveB ? sB : 0u) * D, mu, fb, fe, xdmb, xabb);
      }
    }
    xdma += __shfl_xor(xdma, 32); xaba += __shfl_xor(xaba, 32);
    xdmb += __shfl_xor(xdmb, 32); xabb += __shfl_xor(xabb, 32);
  }
  float cuta, cutb = 0.f;
  float kq[4], oth;
  uint32_t jq[4];
  if constexpr (S16) {   // one row per lane: set h, row col; it goes on the lists as "A"
    quarters16(kq, jq, oth);
    const bool mine = h ? liveB : liveA;
    sA = h ? sB : sA;
    finish(sA, mine, kq, jq, oth, h ? xn2b : xn2a, h ? x0b : x0a, h ? dx2b : dx2a, h ? xdmb : xdma, h ? xabb : xaba, unda, uma,
           cuta, duoa, dma, d1a, d2a, dra);
  } else {   // the lanes of half 0 finish both sets' rows
    quarters32(v1a, v2a, tba, kq, jq, oth);
    finish(sA, h == 0 && liveA, kq, jq, oth, xn2a, x0a, dx2a, xdma, xaba, unda, uma, cuta, duoa, dma, d1a, d2a, dra);
    if constexpr (TWO) {
      quarters32(v1b, v2b, tbb, kq, jq, oth);
      finish(sB, h == 0 && liveB, kq, jq, oth, xn2b, x0b, dx2b, xdmb, xabb, undb, umb, cutb, duob, dmb, d1b, d2b, drb);
    }
  }
  // ONE pair of global atomics per block, not three per wave: the counters share a cache line, same-address
  // atomics are served one at a time by L2 (measured round 2: 11 ns each in a kernel that did nothing else), and
  // 125 K waves per launch all arrive with theirs at the end of the same scheduling round
  __shared__ uint32_t blk_und[WV], blk_changed[WV], blk_duo[WV], blk_base, blk_duo_base;
  if (lane == 0) {
    blk_und[wave] = und_count;
    blk_changed[wave] = changed_count;
    blk_duo[wave] = duo_count;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tu = 0, tc = 0, td = 0;
#pragma unroll
    for (int w = 0; w < WV; w++) {
      tu += blk_und[w];
      tc += blk_changed[w];
      td += blk_duo[w];
    }
    if (tc) atomicAdd(&counters[0], tc);
    blk_base = tu ? atomicAdd(&counters[4], tu) : 0u;
    blk_duo_base = td ? atomicAdd(&counters[kDuoCount], td) : 0u;
  }
  __syncthreads();
  if (duo_count) {   // (row, contender, contender, the best score of all the others)
    uint32_t base = blk_duo_base;
    for (int w = 0; w < wave; w++) base += blk_duo[w];
    const unsigned long long below = (1ull << lane) - 1ull;
    if (duoa) {
      const uint32_t at = base + (uint32_t)__popcll(dma & below);
      reinterpret_cast<uint4 *>(duo)[at] = make_uint4(sA, d1a, d2a, __float_as_uint(dra));
    }
    if (duob) {
      const uint32_t at = base + (uint32_t)__popcll(dma) + (uint32_t)__popcll(dmb & below);
      reinterpret_cast<uint4 *>(duo)[at] = make_uint4(sB, d1b, d2b, __float_as_uint(drb));
    }
  }
  if (und_count) {
    uint32_t base = blk_base;
    for (int w = 0; w < wave; w++) base += blk_und[w];
    const unsigned long long below = (1ull << lane) - 1ull;
    if (unda) {
      const uint32_t at = base + (uint32_t)__popcll(uma & below);
      undecided[at] = sA;
      und_thr[at] = cuta;
    }
    if (undb) {
      const uint32_t at = base + (uint32_t)__popcll(uma) + (uint32_t)__popcll(umb & below);
      undecided[at] = sB;
      und_thr[at] = cutb;
    }
  }
  if constexpr (CARRY != 2) {
    break;
  } else {
    blk += gridDim.x;
    if ((uint64_t)blk * (128u * NSET) >= total) break;   // (block-uniform)
    __syncthreads();   // the tiles, the mean and the block sums in LDS belong to the next trip from here on
  }
  }
}

// The launcher of lloyd_coarse2_kernel.  CARRY = false: the plain pass (MODE 0) over `rows`, or over the row cache
// where there is one.  CARRY = true: a pass that leaves bounds in cy -- every row, streamed from the row cache (MODE 1,
// cy.row_list == nullptr), or the listed rows, gathered from `rows` (MODE 2)
template <bool CARRY>
static hipError_t launch_lloyd_coarse_t(const LloydArgs &a, const void *rows, bool half_rows, const void *xcache,
                                        const float *xmeta, const void *panelhi, uint32_t *undecided, float *und_thr,
                                        const CarryArgs &cy, uint32_t rows_hint, uint32_t *duo, hipStream_t st) {
  return with_width<LloydF16Widths>(a.DP, [&](auto W) {
    constexpr int DP = W(), NSET = DP <= 256 ? 2 : 1;
    const size_t lds_bytes = 2 * 64 * (size_t)(DP * 2) + 512 + 64 + (size_t)DP * 4;
    const uint32_t rows_per_block = 128u * NSET;
    uint32_t grid = (a.N + rows_per_block - 1) / rows_per_block;
    const bool listed = CARRY && cy.row_list, cached = CARRY ? !listed : xcache != nullptr;
    if (listed) {
      // blocks past the (device-side) end of the list leave at once; the grid follows the host's estimate of the
      // list so that a short list does not dispatch N / 256 of them (the kernel strides: a list longer than the
      // estimate costs time, never rows.  KMCUDA_AMD_CARRY_GRID caps the grid -- the tests' way of making every
      // block take several trips)
      if (rows_hint != 0xFFFFFFFFu) {
        const uint32_t want = rows_hint / rows_per_block + rows_hint / (4 * rows_per_block) + 64;
        if (want < grid) grid = want;
      }
      if (const char *v = getenv("KMCUDA_AMD_CARRY_GRID")) {
        const long cap = atol(v);
        if (cap > 0 && (uint32_t)cap < grid) grid = (uint32_t)cap;
      }
    }
    // 16x16x32 with two row sets (DP 32..256); DP 16 (one k-step of 32 features does not fit) and 512 keep 32x32x16,
    // and so does the listed pass at 256 features: with the gathered rows' conversion 16x16x32 spills there
    constexpr bool kS16 = NSET == 2 && DP >= 32;
    auto launch = [&](auto MODE, auto H, auto F, auto C) {
      return with_flag(kS16 && a.coarse_mfma != 32, [&](auto S16) {
        constexpr int SHAPE = (S16() && kS16 && !(MODE() == 2 && DP >= 256)) ? 16 : 32;
        hipLaunchKernelGGL((lloyd_coarse2_kernel<DP, H(), F(), C(), NSET, MODE(), SHAPE>), dim3(grid), dim3(256), lds_bytes,
                           st, cached ? xcache : rows, xmeta, a.N, a.D, reinterpret_cast<const float *>(panelhi), a.bias,
                           a.mu, a.K_pad, a.K, a.stats, a.eps, a.tie_slack, a.assignments, a.assignments_prev, undecided,
                           und_thr, a.counters, cy, duo);
        return hipGetLastError();
      });
    };
    if (cached)
      return launch(std::integral_constant<int, CARRY ? 1 : 0>{}, std::false_type{}, std::true_type{}, std::true_type{});
    return with_flag(half_rows, [&](auto H) {
      return with_flag(a.D == (uint32_t)DP, [&](auto F) {
        return launch(std::integral_constant<int, CARRY ? 2 : 0>{}, H, F, std::false_type{});
      });
    });
  });
}

}  // namespace kmx
