// knn_rerank.hip -- exact re-ranking of per-query candidate lists (kmamd_knn_rerank, knn_rerank_job.cpp; DESIGN.md
// 4.23): for query q the k smallest keys bits(d) << 32 | id over the candidates id = candidates[q][j] < N, with
// d = sqrtf(chain_vv<0>(queries[q], rows[id])) -- the reference's L2 distance (metric_abstraction.h:59-72), the bits
// kmeans_predict and the k-NN index return.  One kernel, one launch: gather, chain and selection in a block, no
// partial keys and no merge.
//
// Split.     A 256-thread block owns whole queries.  R <= 256: QB = 256 / R queries per step, thread t the pair
//            (query t / R, candidate t % R); lanes from QB * R on own no pair and issue no loads.  R > 256: one query,
//            its candidates in passes of 256.  The grid is bounded and strides over the steps (wave_row_grid's bound).
// Gather.    assigned_distance_kernel's tile scheme (assign_dist.hip): chunks of 32 features, 8 lanes fetch one
//            128-byte line of one candidate row with 16-byte loads into registers, a 36-float LDS row stride, the next
//            chunk's loads issued before the current chunk's chain.  The block's queries are staged per chunk in a
//            second tile of QB rows; the lanes of one query read the same address there (a broadcast).
//            Rows the 16-byte loads cannot serve (D % 4 != 0, a base off 16 bytes) take chain_vv per thread.
// Chain.     One serial chain per thread from LDS in chain_vv's order: fma_rd on the difference, kahan_fold.
// Selection. Every thread leaves its canonical key (NaN 0x7FC00000 behind +inf, -0 as +0; ~0 for no candidate) in
//            LDS -- across the passes of R > 256, at most 8 KB.  Behind a barrier a thread ranks its key among its
//            query's R keys (smaller keys plus equal keys at earlier positions; the lanes of a query read the same
//            word) and writes it to slot `rank` when rank < k; slots from the valid count on get the padding.  No
//            sort network, no atomics; R^2 compares per query.
#include <math.h>

#include "exact.hpp"
#include "kernels.hpp"

namespace kmx {

constexpr int kRrBlock = 256;                   // pairs per pass: one candidate row per thread
constexpr int kRrStride = 36;                   // floats per tile row (conflict-free b128 reads by consecutive rows)
constexpr uint64_t kRrNoKey = ~0ull;            // above every key: a candidate id is at most 2^32 - 3
constexpr uint32_t kRrNanBits = 0x7FC00000u;
constexpr uint32_t kRrNoId = 0xFFFFFFFFu;

uint32_t knn_rerank_query_block(uint32_t R) { return R == 0 || R > (uint32_t)kRrBlock ? 1u : kRrBlock / R; }

// row tile, query tile, keys, the pass's candidate ids
size_t knn_rerank_lds_bytes(uint32_t R) {
  const size_t QB = knn_rerank_query_block(R);
  return (kRrBlock + QB) * kRrStride * sizeof(float) + QB * R * sizeof(uint64_t) + kRrBlock * sizeof(uint32_t);
}

// TILED: D % 4 == 0 and both bases 16-byte aligned (the launcher looks)
template <bool TILED>
__global__ __launch_bounds__(kRrBlock) void knn_rerank_kernel(const float *__restrict__ queries, uint32_t Q,
                                                              const float *__restrict__ rows, uint32_t N, uint32_t D,
                                                              const uint32_t *__restrict__ candidates, uint32_t R,
                                                              uint32_t k, uint32_t QB, uint32_t *__restrict__ indices,
                                                              float *__restrict__ distances) {
  extern __shared__ float4 rr_lds4[];
  float *rtile = reinterpret_cast<float *>(rr_lds4);                      // 256 x 36: the pass's candidate rows
  float *qtile = rtile + kRrBlock * kRrStride;                            // QB x 36: the step's queries
  uint64_t *keys = reinterpret_cast<uint64_t *>(qtile + QB * kRrStride);  // QB x R
  uint32_t *cid = reinterpret_cast<uint32_t *>(keys + (size_t)QB * R);    // 256; kRrNoId: no row to read
  const uint32_t t = threadIdx.x;
  const uint32_t npass = (R + kRrBlock - 1) / kRrBlock, nchunk = (D + 31) / 32;
  const uint32_t ql = R <= (uint32_t)kRrBlock ? t / R : 0u, jl = R <= (uint32_t)kRrBlock ? t - ql * R : t;
  const uint32_t qrow = ql < QB ? ql : 0u;   // a lane without a pair runs the chain on row 0 of the query tile
  const uint64_t steps = ((uint64_t)Q + QB - 1) / QB;
  for (uint64_t step = blockIdx.x; step < steps; step += gridDim.x) {
    const uint64_t q0 = step * QB, q = q0 + ql;
    const bool mine = ql < QB && q < Q;
    for (uint32_t pass = 0; pass < npass; pass++) {
      const uint32_t j = jl + pass * kRrBlock;
      __syncthreads();   // the previous pass's tiles and cid[], the previous step's keys are done with
      uint32_t id = kRrNoId;
      if (mine && j < R) {
        id = candidates[q * R + j];
        if (id >= N) id = kRrNoId;
      }
      cid[t] = id;
      float acc = 0.f, corr = 0.f;
      if (!TILED) {
        if (id != kRrNoId) acc = chain_vv<0>(queries + q * D, rows + (size_t)id * D, D);
      } else {
        __syncthreads();
        float4 rstage[8], qstage[8];
        auto fetch = [&](uint32_t ch) {
#pragma unroll
          for (int s = 0; s < 8; s++) {
            const uint32_t p = t + kRrBlock * s, r = p >> 3, f = ch * 32 + (p & 7u) * 4, a = cid[r];
            rstage[s] = (a != kRrNoId && f < D) ? *reinterpret_cast<const float4 *>(rows + (size_t)a * D + f)
                                                : make_float4(0.f, 0.f, 0.f, 0.f);
          }
#pragma unroll
          for (int s = 0; s < 8; s++) {
            const uint32_t p = t + kRrBlock * s, r = p >> 3, f = ch * 32 + (p & 7u) * 4;
            if (p < QB * 8)   // block-uniform for s >= 1: false unless QB > 32 s
              qstage[s] = (q0 + r < Q && f < D) ? *reinterpret_cast<const float4 *>(queries + (q0 + r) * D + f)
                                                : make_float4(0.f, 0.f, 0.f, 0.f);
          }
        };
        fetch(0);
        for (uint32_t ch = 0; ch < nchunk; ch++) {
          if (ch) __syncthreads();   // the previous chunk has been consumed
#pragma unroll
          for (int s = 0; s < 8; s++) {
            const uint32_t p = t + kRrBlock * s, r = p >> 3, c4 = p & 7u;
            *reinterpret_cast<float4 *>(&rtile[r * kRrStride + c4 * 4]) = rstage[s];
            if (p < QB * 8) *reinterpret_cast<float4 *>(&qtile[r * kRrStride + c4 * 4]) = qstage[s];
          }
          __syncthreads();
          if (ch + 1 < nchunk) fetch(ch + 1);
          const uint32_t fmax = D - ch * 32 < 32u ? D - ch * 32 : 32u;   // multiple of 4
          for (uint32_t c4 = 0; c4 * 4 < fmax; c4++) {
            const float4 xv = *reinterpret_cast<const float4 *>(&qtile[qrow * kRrStride + c4 * 4]);
            const float4 yv = *reinterpret_cast<const float4 *>(&rtile[t * kRrStride + c4 * 4]);
            const float aa[4] = {xv.x, xv.y, xv.z, xv.w}, bb[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
              const float d = aa[e] - bb[e];
              kahan_fold(fma_rd(d, d, corr), acc, corr);
            }
          }
        }
      }
      if (mine && j < R) {
        const float d = sqrtf(acc);
        const uint32_t bits = d != d ? kRrNanBits : d == 0.f ? 0u : __float_as_uint(d);
        keys[ql * R + j] = id != kRrNoId ? (uint64_t)bits << 32 | id : kRrNoKey;
      }
    }
    __syncthreads();
    if (!mine) continue;   // no barrier below
    const uint64_t *own = keys + ql * R;
    for (uint32_t j = jl; j < R; j += kRrBlock) {
      const uint64_t key = own[j];
      uint32_t rank = 0, valid = 0;
      for (uint32_t i = 0; i < R; i++) {
        const uint64_t other = own[i];
        rank += (other < key || (other == key && i < j)) ? 1u : 0u;
        valid += other != kRrNoKey ? 1u : 0u;
      }
      if (key != kRrNoKey && rank < k) {
        indices[q * k + rank] = (uint32_t)key;
        distances[q * k + rank] = __uint_as_float((uint32_t)(key >> 32));
      }
      if (valid + j < k) {   // k <= R: positions [0, k - valid) fill the slots no candidate does
        indices[q * k + valid + j] = kRrNoId;
        distances[q * k + valid + j] = __uint_as_float(kRrNanBits);
      }
    }
  }
}

hipError_t launch_knn_rerank(const float *queries, uint32_t Q, const float *rows, uint32_t N, uint32_t D,
                             const uint32_t *candidates, uint32_t R, uint32_t k, uint32_t *indices, float *distances,
                             hipStream_t st) {
  if (Q == 0) return hipSuccess;
  const uint32_t QB = knn_rerank_query_block(R);
  const size_t lds = knn_rerank_lds_bytes(R);
  const uint64_t steps = ((uint64_t)Q + QB - 1) / QB;
  const dim3 grid((uint32_t)(steps < kWaveRowGridMax ? steps : kWaveRowGridMax)), block(kRrBlock);
  const bool tiled = (D & 3u) == 0 && ((((uintptr_t)queries) | ((uintptr_t)rows)) & 15u) == 0;
  return with_flag(tiled, [&](auto T) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&knn_rerank_kernel<T()>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((knn_rerank_kernel<T()>), grid, block, lds, st, queries, Q, rows, N, D, candidates, R, k, QB,
                       indices, distances);
    return hipGetLastError();
  });
}

}  // namespace kmx
