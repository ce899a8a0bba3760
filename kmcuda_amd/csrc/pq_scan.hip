// pq_scan.hip -- top-k search over product-quantiser codes by asymmetric distance computation (kmamd_pq_search,
// pq_job.cpp).  L2, fp32 tables, uint8 codes, 1 <= M <= 64 sub-spaces, k <= 256.
//
//   pq_tables  grid = (sub-space, group of 64 queries).  A block stages the codeword panel of its sub-space in LDS (row
//              stride dsub | 1: no bank conflict at any dsub), thread c owns codeword c and builds, query by query,
//              T[q][m][c] = sum_j fl(fl(x_j - y_j)^2), j ascending from the j = 0 term, +inf for c >= ksub.  Plain
//              VALU arithmetic: the definition is term by term and the phase is Q * 256 * M * dsub operations, nothing
//              beside the scan.  The tables are written as the scan reads them: [query tile][m][code][q in tile].
//   pq_scan    grid = (row chunk, query tile), the row chunk running fastest.  Table-stationary: a block copies the QT
//              tables of its query tile into LDS once (QT * M KB) and streams the code rows of its chunk, one row per
//              lane and step (16-byte loads where M and the base allow, else 4-byte, else bytes), the row's bytes in
//              VGPRs (the next step's already in flight).  For every byte ONE LDS
//              read fetches the QT adjacent entries T[m][code][0..QT) -- ds_read_b128 per four queries -- and feeds QT
//              independent add chains, m ascending from the m = 0 term.
//              Selection: per query an LDS buffer of `cap` >= 2k keys (bits(d) << 32 | row, NaN canonical), a count and
//              a threshold key that every lane holds in registers.  A lane appends a key only below the threshold (one
//              LDS integer atomic per wave and query, by ballot); a buffer that fills is sorted by the block (bitonic),
//              cut to its k smallest keys and lowers the threshold; lanes that found no room try again against the new
//              threshold.  The compare is on the whole 64-bit key, so what is kept is the k smallest keys of the chunk
//              whatever order the lanes arrived in.  The block writes k sorted keys per (query, chunk).
//   pq_merge   one block per query: the chunks' keys, 256 at a time, through a 512-key bitonic sort whose lower half
//              carries the best so far; writes the k indices and distances.
#include <float.h>
#include <math.h>

#include "kernels.hpp"

namespace kmx {

namespace {

constexpr int kPqThreads = 256;                  // pq_scan: one row per thread and step, a 256-row tile
constexpr uint64_t kPqNoKey = ~0ull;             // above every key: bits(d) is at most the canonical NaN's
constexpr uint32_t kPqNanBits = 0x7FC00000u;
constexpr uint32_t kPqTableQueries = 64;         // pq_tables: queries per block, a multiple of every query tile
constexpr uint32_t kPqLdsPerCu = 160u << 10;     // gfx950

__global__ __launch_bounds__(kPqThreads) void pq_tables_kernel(const float *__restrict__ queries, uint32_t Qc,
                                                               const float *__restrict__ codebooks, uint32_t M,
                                                               uint32_t dsub, uint32_t ksub, uint32_t QT,
                                                               float *__restrict__ tables) {
  extern __shared__ float pq_panel[];   // ksub x (dsub | 1)
  const uint32_t m = blockIdx.x, c = threadIdx.x, ld = dsub | 1u;
  const float *book = codebooks + (size_t)m * ksub * dsub;
  for (uint32_t i = c; i < ksub * dsub; i += kPqThreads) pq_panel[(i / dsub) * ld + i % dsub] = book[i];
  __syncthreads();
  const float *y = pq_panel + c * ld;
  const uint32_t q0 = blockIdx.y * kPqTableQueries, q_pad = (Qc + QT - 1) / QT * QT;
  for (uint32_t q = q0; q < q0 + kPqTableQueries && q < q_pad; q++) {
    float d = INFINITY;   // a code byte that names no codeword, and the queries that pad the last tile
    if (q < Qc && c < ksub) {
      const float *x = queries + (size_t)q * M * dsub + (size_t)m * dsub;
      const float t0 = x[0] - y[0];
      d = t0 * t0;
      for (uint32_t j = 1; j < dsub; j++) {
        const float t = x[j] - y[j];
        d = d + t * t;
      }
    }
    tables[(((size_t)(q / QT) * M + m) * 256 + c) * QT + q % QT] = d;
  }
}

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

template <int QT, bool VEC>
__global__ __launch_bounds__(kPqThreads) void pq_scan_kernel(PqGeom g, const float *__restrict__ tables,
                                                             uint32_t queries, uint64_t *__restrict__ part) {
  extern __shared__ float4 pq_lds4[];
  const uint32_t M = g.M, k = g.k, cap = g.cap, t = threadIdx.x, lane = t & 63u;
  const uint32_t chunk = blockIdx.x % g.G, tile = blockIdx.x / g.G;
  float *T = reinterpret_cast<float *>(pq_lds4);                          // M x 256 x QT
  uint64_t *buf = reinterpret_cast<uint64_t *>(T + (size_t)QT * M * 256);   // QT x cap
  uint64_t *thr = buf + (size_t)QT * cap;                                 // QT
  uint32_t *cnt = reinterpret_cast<uint32_t *>(thr + QT);                 // QT
  uint32_t *full = cnt + QT;                                              // the round in which a buffer last filled
  {
    const float4 *src = reinterpret_cast<const float4 *>(tables + (size_t)tile * QT * M * 256);
    for (uint32_t i = t; i < (uint32_t)QT * M * 64; i += kPqThreads) pq_lds4[i] = src[i];
    if (t < (uint32_t)QT) { thr[t] = kPqNoKey; cnt[t] = 0; }
    if (t == 0) *full = 0;
  }
  __syncthreads();

  const bool dwords = (M & 3u) == 0 && (reinterpret_cast<uintptr_t>(g.codes) & 3u) == 0;
  const uint64_t r0 = (uint64_t)chunk * g.R, r1 = r0 + g.R < g.N ? r0 + g.R : g.N;
  uint64_t limit[QT];   // every lane's copy of thr[]
#pragma unroll
  for (int q = 0; q < QT; q++) limit[q] = kPqNoKey;
  uint32_t round = 0, w[16], wn[16];
  pq_load_codes<VEC>(g.codes, r0 + t, r0 + t < r1, M, dwords, wn);
  for (uint64_t base = r0; base < r1; base += kPqThreads) {
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = wn[i];
    const uint64_t row = base + t, next = row + kPqThreads;
    pq_load_codes<VEC>(g.codes, next, next < r1, M, dwords, wn);

    float acc[QT];
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

    uint64_t key[QT];
    uint32_t todo = 0;
#pragma unroll
    for (int q = 0; q < QT; q++) {
      const uint32_t bits = acc[q] != acc[q] ? kPqNanBits : __float_as_uint(acc[q]);
      key[q] = (uint64_t)bits << 32 | (uint32_t)row;
      if (row < r1 && key[q] < limit[q]) todo |= 1u << q;
    }
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
  pq_reduce<QT>(buf, thr, cnt, cap, k, (1u << QT) - 1u, t);
#pragma unroll
  for (int q = 0; q < QT; q++) {
    const uint32_t query = tile * QT + q;
    if (query < queries && t < k)
      part[((size_t)query * g.G + chunk) * k + t] = t < cnt[q] ? buf[q * cap + t] : kPqNoKey;
  }
}

__global__ __launch_bounds__(kPqThreads) void pq_merge_kernel(const uint64_t *__restrict__ part, uint32_t G, uint32_t k,
                                                              uint32_t *__restrict__ indices,
                                                              float *__restrict__ distances) {
  __shared__ uint64_t s[2 * kPqThreads];   // [0, 256): the best so far; [256, 512): the next 256 keys
  const uint32_t q = blockIdx.x, t = threadIdx.x;
  const uint64_t total = (uint64_t)G * k;
  const uint64_t *mine = part + (size_t)q * total;
  s[t] = kPqNoKey;
  for (uint64_t at = 0; at < total; at += kPqThreads) {
    s[kPqThreads + t] = at + t < total ? mine[at + t] : kPqNoKey;
    __syncthreads();
    for (uint32_t size = 2; size <= 2 * kPqThreads; size <<= 1)
      for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
        const uint32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const uint64_t a = s[lo], b = s[hi];
        if ((a > b) == ((lo & size) == 0)) {
          s[lo] = b;
          s[hi] = a;
        }
        __syncthreads();
      }
  }
  if (t < k) {
    indices[(size_t)q * k + t] = (uint32_t)s[t];
    distances[(size_t)q * k + t] = __uint_as_float((uint32_t)(s[t] >> 32));
  }
}

template <int QT>
hipError_t pq_scan_launch(const PqGeom &g, bool vec, const float *tables, uint32_t queries, uint64_t *part,
                          hipStream_t st) {
  const size_t lds = pq_scan_lds_bytes(g.M, g.k, QT);
  const uint32_t tiles = (queries + QT - 1) / QT;
  // M a multiple of 16 has a tile of at most 4: the larger tiles have no 16-byte variant
  return with_flag(vec && QT <= 4, [&](auto V16) {
    using V = std::integral_constant<bool, decltype(V16)::value && QT <= 4>;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&pq_scan_kernel<QT, V::value>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((pq_scan_kernel<QT, V::value>), dim3(g.G * tiles), dim3(kPqThreads), lds, st, g, tables, queries,
                       part);
    return hipGetLastError();
  });
}

}  // namespace

uint32_t pq_candidate_cap(uint32_t k) {
  uint32_t cap = 64;
  while (cap < 2 * k) cap <<= 1;
  return cap;
}

size_t pq_scan_lds_bytes(uint32_t M, uint32_t k, uint32_t QT) {
  return (size_t)QT * ((size_t)M * 1024 + (size_t)pq_candidate_cap(k) * 8 + 16) + 16;
}

uint32_t pq_query_tile(uint32_t M, uint32_t k) {
  if (M == 0 || M > 64 || k == 0 || k > 256) return 0;
  for (uint32_t qt : {16u, 8u, 4u})   // two blocks per CU
    if (pq_scan_lds_bytes(M, k, qt) <= kPqLdsPerCu / 2) return qt;
  for (uint32_t qt : {4u, 2u})        // one
    if (pq_scan_lds_bytes(M, k, qt) <= kPqLdsPerCu) return qt;
  return 0;
}

hipError_t launch_pq_tables(const float *queries, uint32_t Qc, const float *codebooks, uint32_t M, uint32_t dsub,
                            uint32_t ksub, uint32_t QT, float *tables, hipStream_t st) {
  const size_t lds = (size_t)ksub * (dsub | 1u) * sizeof(float);
  const uint32_t q_pad = (Qc + QT - 1) / QT * QT;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&pq_tables_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pq_tables_kernel, dim3(M, (q_pad + kPqTableQueries - 1) / kPqTableQueries), dim3(kPqThreads), lds,
                     st, queries, Qc, codebooks, M, dsub, ksub, QT, tables);
  return hipGetLastError();
}

hipError_t launch_pq_scan(const PqGeom &g, const float *tables, uint32_t queries, uint64_t *part, hipStream_t st) {
  const bool vec = (g.M & 15u) == 0 && (((uintptr_t)g.codes) & 15u) == 0;
  switch (g.QT) {
    case 2: return pq_scan_launch<2>(g, vec, tables, queries, part, st);
    case 4: return pq_scan_launch<4>(g, vec, tables, queries, part, st);
    case 8: return pq_scan_launch<8>(g, vec, tables, queries, part, st);
    case 16: return pq_scan_launch<16>(g, vec, tables, queries, part, st);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_pq_merge(const uint64_t *part, uint32_t queries, uint32_t G, uint32_t k, uint32_t *indices,
                           float *distances, hipStream_t st) {
  hipLaunchKernelGGL(pq_merge_kernel, dim3(queries), dim3(kPqThreads), 0, st, part, G, k, indices, distances);
  return hipGetLastError();
}

}  // namespace kmx
