// pq_select.hpp -- what the two scans over product-quantiser codes share (pq_scan.hip: every row, DESIGN.md 4.21;
// ivfpq_scan.hip: the rows of probed lists, 4.22): a row's code bytes into registers, the table read of one byte, and
// the selection -- per query (or pair) of a block's tile an LDS buffer of `cap` >= 2k keys (bits(d) << 32 | id, NaN
// canonical), a count and a threshold key that every lane holds in registers.  A lane appends a key only below the
// threshold (one LDS integer atomic per wave and query, by ballot); a buffer that fills is sorted by the block
// (bitonic), cut to its k smallest keys and lowers the threshold; lanes that found no room try again against the new
// threshold.  The compare is on the whole 64-bit key, so what is kept is the k smallest keys whatever order the lanes
// arrived in.  Blocks of kPqThreads threads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kmx {

constexpr int kPqThreads = 256;                  // one row per thread and step, a 256-row tile
constexpr uint64_t kPqNoKey = ~0ull;             // above every key: bits(d) is at most the canonical NaN's
constexpr uint32_t kPqNanBits = 0x7FC00000u;
constexpr uint32_t kPqLdsPerCu = 160u << 10;     // gfx950

// the M code bytes of row `row` (zeros for a lane without a row) into w[0 .. 16): byte m is bits 8 (m % 4) of w[m / 4]
template <bool VEC>
__device__ __forceinline__ void pq_load_codes(const uint8_t *__restrict__ codes, uint64_t row, bool have, uint32_t M,
                                              bool dwords, uint32_t (&w)[16]) {
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = 0;
  if (!have) return;
  const uint8_t *p = codes + row * M;
  if (VEC) {   // M is a multiple of 16 and the matrix 16-byte aligned
#pragma unroll
    for (int g = 0; g < 4; g++)
      if ((uint32_t)g * 16 < M) {
        const uint4 v = reinterpret_cast<const uint4 *>(p)[g];
        w[g * 4] = v.x; w[g * 4 + 1] = v.y; w[g * 4 + 2] = v.z; w[g * 4 + 3] = v.w;
      }
  } else if (dwords) {   // M a multiple of 4 and the matrix 4-byte aligned
#pragma unroll
    for (int i = 0; i < 16; i++)
      if ((uint32_t)i * 4 < M) w[i] = reinterpret_cast<const uint32_t *>(p)[i];
  } else {
#pragma unroll
    for (int m = 0; m < 64; m++)
      if ((uint32_t)m < M) w[m / 4] |= (uint32_t)p[m] << (8 * (m % 4));
  }
}

template <int QT>
__device__ __forceinline__ void pq_lookup(const float *__restrict__ e, float (&v)[QT]) {
  if (QT == 2) {
    const float2 a = *reinterpret_cast<const float2 *>(e);
    v[0] = a.x; v[1] = a.y;
  } else {
#pragma unroll
    for (int j = 0; j < QT / 4; j++) {
      const float4 a = reinterpret_cast<const float4 *>(e)[j];
      v[j * 4] = a.x; v[j * 4 + 1] = a.y; v[j * 4 + 2] = a.z; v[j * 4 + 3] = a.w;
    }
  }
}

// acc[q] = sum_m T[m][byte m of w][q], m ascending from the m = 0 term; T is M x 256 x QT in LDS
template <int QT, bool VEC>
__device__ __forceinline__ void pq_score(const float *__restrict__ T, const uint32_t (&w)[16], uint32_t M,
                                         float (&acc)[QT]) {
#pragma unroll
  for (int grp = 0; grp < 4; grp++)
    if ((uint32_t)grp * 16 < M) {
#pragma unroll
      for (int b = 0; b < 16; b++) {
        const int m = grp * 16 + b;
        if (VEC || (uint32_t)m < M) {
          const uint32_t code = (w[m / 4] >> (8 * (m % 4))) & 0xFFu;
          float v[QT];
          pq_lookup<QT>(T + ((size_t)m * 256 + code) * QT, v);
#pragma unroll
          for (int q = 0; q < QT; q++) acc[q] = m == 0 ? v[q] : acc[q] + v[q];
        }
      }
    }
}

constexpr int kPqFillLoads = 16;   // table entries a thread keeps in flight per group of pq_fill_tables

// The tables of a block's pairs out of per-query lines in global memory (the non-residual IVF scans):
// lines[query][m][256] of E -- a float, or a uint16_t that holds a half -- complete to column 255.  pid[q]: the pair of
// slot q < live, its query pid[q] / nprobe; a slot without a pair gets `inf`.  Thread t owns column t: it loads the QT
// entries of 16 / QT sub-spaces, issues the next group's loads, and hands this group's to put(m, e) -- which stores the
// QT adjacent entries T[m][t][0..QT) with one wide LDS write.  The lines are indexed in 32 bits: the host keeps a
// chunk's within 2^27 entries.  One barrier, at the end.
template <int QT, typename E, typename Put>
__device__ __forceinline__ void pq_fill_tables(const E *__restrict__ lines, const uint32_t *pid, uint32_t live,
                                               uint32_t nprobe, uint32_t M, E inf, uint32_t t, Put put) {
  constexpr int G = kPqFillLoads / QT;
  uint32_t at[QT];   // the index of (query of slot q, m = 0, column t)
#pragma unroll
  for (int q = 0; q < QT; q++) at[q] = (uint32_t)q < live ? (pid[q] / nprobe * M) * 256u + t : 0u;
  E e[G][QT], en[G][QT];
  auto load = [&](uint32_t m0, E (&v)[G][QT]) {
#pragma unroll
    for (int i = 0; i < G; i++) {
      const uint32_t m = m0 + i;
#pragma unroll
      for (int q = 0; q < QT; q++) v[i][q] = m < M && (uint32_t)q < live ? lines[at[q] + m * 256u] : inf;
    }
  };
  load(0, en);
  for (uint32_t m0 = 0; m0 < M; m0 += G) {
#pragma unroll
    for (int i = 0; i < G; i++)
#pragma unroll
      for (int q = 0; q < QT; q++) e[i][q] = en[i][q];
    load(m0 + G, en);   // in flight over this group's stores
#pragma unroll
    for (int i = 0; i < G; i++)
      if (m0 + i < M) put(m0 + i, e[i]);
  }
  __syncthreads();
}

// The block sorts the buffers named in `need` (cnt[q] keys each, the rest padded) and keeps their k smallest keys.
template <int QT>
__device__ __forceinline__ void pq_reduce(uint64_t *buf, uint64_t *thr, uint32_t *cnt, uint32_t cap, uint32_t k,
                                          uint32_t need, uint32_t t) {
#pragma unroll
  for (int q = 0; q < QT; q++)
    if (need >> q & 1u) {
      const uint32_t n = cnt[q] < cap ? cnt[q] : cap;
      for (uint32_t j = n + t; j < cap; j += kPqThreads) buf[q * cap + j] = kPqNoKey;
    }
  __syncthreads();
  for (uint32_t size = 2; size <= cap; size <<= 1)
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll
      for (int q = 0; q < QT; q++)
        if (need >> q & 1u)
          for (uint32_t i = t; i < cap / 2; i += kPqThreads) {
            const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
            const uint64_t a = buf[q * cap + lo], b = buf[q * cap + hi];
            if ((a > b) == ((lo & size) == 0)) {
              buf[q * cap + lo] = b;
              buf[q * cap + hi] = a;
            }
          }
      __syncthreads();
    }
  if (t < (uint32_t)QT && (need >> t & 1u)) {
    const uint32_t n = cnt[t] < cap ? cnt[t] : cap, kept = n < k ? n : k;
    cnt[t] = kept;
    thr[t] = kept >= k ? buf[t * cap + k - 1] : kPqNoKey;
  }
  __syncthreads();
}

// One step of the block: every lane offers key[q] for the queries named in `todo` (a lane without a row names none).
// limit[] is every lane's copy of thr[]; `full` holds the number of the round in which a buffer last filled.
template <int QT>
__device__ __forceinline__ void pq_append(uint64_t *buf, uint64_t *thr, uint32_t *cnt, uint32_t *full, uint32_t cap,
                                          uint32_t k, uint32_t t, const uint64_t (&key)[QT], uint32_t todo,
                                          uint64_t (&limit)[QT], uint32_t &round) {
  const uint32_t lane = t & 63u;
  for (;;) {
    round++;
#pragma unroll
    for (int q = 0; q < QT; q++) {
      const bool mine = todo >> q & 1u;
      const uint64_t mask = __ballot(mine);
      if (mask) {
        const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1u, n = (uint32_t)__popcll(mask);
        uint32_t at = 0;
        if (lane == leader) at = atomicAdd(cnt + q, n);
        at = (uint32_t)__shfl((int)at, (int)leader, 64);
        const uint32_t pos = at + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (mine && pos < cap) {
          buf[q * cap + pos] = key[q];
          todo &= ~(1u << q);
        }
        if (lane == leader && at + n >= cap) *full = round;
      }
    }
    __syncthreads();
    // a later round can only write a larger number, and only after every thread has left this one
    if (*reinterpret_cast<volatile uint32_t *>(full) != round) break;
    uint32_t need = 0;
#pragma unroll
    for (int q = 0; q < QT; q++)
      if (cnt[q] >= cap) need |= 1u << q;
    pq_reduce<QT>(buf, thr, cnt, cap, k, need, t);
#pragma unroll
    for (int q = 0; q < QT; q++) {
      limit[q] = thr[q];
      if (!(key[q] < limit[q])) todo &= ~(1u << q);
    }
  }
}

}  // namespace kmx
