// pq16_scan.hip -- the two byte-code scans over fp16 lookup tables (kmamd_pq_search_f16, pq_job.cpp;
// kmamd_ivfpq_search_f16, ivfpq_job.cpp).  The tables are built in fp32 exactly as pq_scan.hip and
// ivfpq_scan.hip build them, every entry is rounded ONCE to IEEE binary16 (round to nearest even, subnormals kept,
// beyond 65504 +inf, NaN stays NaN) and a row's distance is sum_m float(T16[m][code_m]), m ascending from the m = 0
// term, as separate fp32 round-to-nearest additions.  Codes, keys, selection (pq_select.hpp), merge (launch_pq_merge)
// and pair sort (launch_ivfpq_group) are the fp32 scans'.
//
// An entry T[m][code][0..QT) is QT halves: 512 bytes per (sub-space, query) where the fp32 tables take 1 KB, so a
// tile's tables are half the LDS and one ds_read_b64 (QT = 4), one ds_read_b128 (8) or two (16) serve a code byte.  No
// swizzle: the entry of a byte is one naturally aligned read of 2, 4 or 2 x 4 banks whose position among the 64 banks
// is the code's low bits -- for codes that are anything like uniform the lanes of a wave already spread over every
// bank group, and lanes with equal codes read one address.
//
// The add: acc = fl(float(h) + acc) is written as the mixed-precision FMA v_fma_mix_f32 acc, h, 1.0, acc -- the
// product float(h) * 1.0 is exact, the FMA rounds once, so the bits are those of the conversion followed by the
// addition, and a table entry costs one VALU instruction where convert-and-add costs two.  op_sel picks the half of
// the 32-bit pair; the halves never leave their pairs.
//
//   pq16_tables  grid = (sub-space, group of 64 queries), pq_tables' panel (row stride dsub | 1).  Thread c owns
//              codeword c and builds FOUR queries at a time (every tile is a multiple of 4), four chains in ascending
//              j; the four halves go out as one 8-byte store, adjacent for adjacent codewords at QT = 4.
//              [query tile][m][code][q in tile] in halves.
//   pq16_scan  grid = (row chunk, query tile), table-stationary as pq_scan: the tile's tables into LDS by 16-byte
//              copies (QT * M * 512 bytes), then the stream -- pq_load_codes, 16-byte code loads also at QT = 8 (a block
//              has 256 VGPRs a lane at two waves per SIMD; the fp32 scan kept them to QT <= 4) --, pq_append, pq_reduce.
//   ivfpq16_scan  grid = (pair tile, row split) as ivfpq_scan: the block's QT tables are built in its own LDS, thread c
//              against the QT staged residual sub-vectors, QT fp32 chains, the QT adjacent entries rounded and stored
//              as halves with one wide LDS write.  The residuals are staged in the candidate buffers (QT x 256 of their
//              QT x cap x 8 >= QT x 512 bytes), which nothing uses before the stream starts: one LDS size and one tile
//              rule for both scans.
//   ivfpq16_scan_nonres  the same block over non-residual lists (kmamd_ivfpq_search_nonresidual_f16):
//              the tables are pq_fill_tables' copy (pq_select.hpp) of the pairs' query-level lines of halves
//              (ivfpq_query_tables, 512 bytes per sub-space), QT halves packed into one wide LDS write; no arithmetic.
#include <float.h>
#include <math.h>

#include <hip/hip_fp16.h>

#include "kernels.hpp"
#include "pq_select.hpp"

namespace kmx {

namespace {

constexpr uint32_t kPq16TableQueries = 64;   // pq16_tables: queries per block, a multiple of every query tile
constexpr uint32_t kPq16Stage = 64;          // floats of one staged residual sub-vector: the largest dsub
// waves per SIMD the scans are compiled for: two blocks of four waves per CU, as the tile rule lays out the LDS
constexpr int kPq16Waves = 2;

// two floats rounded to nearest even into a pair of halves, `lo` in bits 0..15
__device__ __forceinline__ uint32_t pq16_pack(float lo, float hi) {
  return (uint32_t)__half_as_ushort(__float2half_rn(lo)) | (uint32_t)__half_as_ushort(__float2half_rn(hi)) << 16;
}

// float(half `hi` of `pair`)
template <int HI>
__device__ __forceinline__ float pq16_float(uint32_t pair) {
  return __half2float(__ushort_as_half((unsigned short)(HI ? pair >> 16 : pair & 0xFFFFu)));
}

// fl(float(half HI of `pair`) + acc): float(h) * 1.0 is exact and the FMA rounds once
template <int HI>
__device__ __forceinline__ float pq16_add(uint32_t pair, float acc) {
  float r;
  if (HI)
    asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(pair), "v"(acc));
  else
    asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(pair), "v"(acc));
  return r;
}

// the QT halves of one entry as QT / 2 pairs: one ds_read_b64, one ds_read_b128 or two
template <int QT>
__device__ __forceinline__ void pq16_lookup(const uint32_t *__restrict__ e, uint32_t (&p)[QT / 2]) {
  if (QT == 4) {
    const uint2 a = *reinterpret_cast<const uint2 *>(e);
    p[0] = a.x; p[1] = a.y;
  } else {
#pragma unroll
    for (int j = 0; j < QT / 8; j++) {
      const uint4 a = reinterpret_cast<const uint4 *>(e)[j];
      p[j * 4] = a.x; p[j * 4 + 1] = a.y; p[j * 4 + 2] = a.z; p[j * 4 + 3] = a.w;
    }
  }
}

// QT floats rounded to an entry of QT halves, stored with one wide write (two at QT = 16)
template <int QT>
__device__ __forceinline__ void pq16_store(uint32_t *e, const float (&v)[QT]) {
  if (QT == 4) {
    *reinterpret_cast<uint2 *>(e) = make_uint2(pq16_pack(v[0], v[1]), pq16_pack(v[2], v[3]));
  } else {
#pragma unroll
    for (int j = 0; j < QT / 8; j++)
      reinterpret_cast<uint4 *>(e)[j] = make_uint4(pq16_pack(v[j * 8], v[j * 8 + 1]), pq16_pack(v[j * 8 + 2], v[j * 8 + 3]),
                                                   pq16_pack(v[j * 8 + 4], v[j * 8 + 5]), pq16_pack(v[j * 8 + 6], v[j * 8 + 7]));
  }
}

// acc[q] = sum_m float(T[m][byte m of w][q]), m ascending from the m = 0 term; T is M x 256 entries of QT / 2 pairs
template <int QT, bool VEC>
__device__ __forceinline__ void pq16_score(const uint32_t *__restrict__ T, const uint32_t (&w)[16], uint32_t M,
                                           float (&acc)[QT]) {
#pragma unroll
  for (int grp = 0; grp < 4; grp++)
    if ((uint32_t)grp * 16 < M) {
#pragma unroll
      for (int b = 0; b < 16; b++) {
        const int m = grp * 16 + b;
        if (VEC || (uint32_t)m < M) {
          const uint32_t code = (w[m / 4] >> (8 * (m % 4))) & 0xFFu;
          uint32_t p[QT / 2];
          pq16_lookup<QT>(T + ((size_t)m * 256 + code) * (QT / 2), p);
#pragma unroll
          for (int i = 0; i < QT / 2; i++) {
            acc[2 * i] = m == 0 ? pq16_float<0>(p[i]) : pq16_add<0>(p[i], acc[2 * i]);
            acc[2 * i + 1] = m == 0 ? pq16_float<1>(p[i]) : pq16_add<1>(p[i], acc[2 * i + 1]);
          }
        }
      }
    }
}

// one term of a table entry: acc = fl(fl(x - y)^2) for the j = 0 term, else fl(acc + fl(fl(x - y)^2))
__device__ __forceinline__ void pq16_term(float &acc, float x, float y, bool first) {
  const float d = x - y;
  acc = first ? d * d : acc + d * d;
}

__global__ __launch_bounds__(kPqThreads) void pq16_tables_kernel(const float *__restrict__ queries, uint32_t Qc,
                                                                 const float *__restrict__ codebooks, uint32_t M,
                                                                 uint32_t dsub, uint32_t ksub, uint32_t QT,
                                                                 uint32_t *__restrict__ tables) {
  extern __shared__ float pq16_panel[];   // ksub x (dsub | 1)
  const uint32_t m = blockIdx.x, c = threadIdx.x, ld = dsub | 1u, D = M * dsub;
  const float *book = codebooks + (size_t)m * ksub * dsub;
  for (uint32_t i = c; i < ksub * dsub; i += kPqThreads) pq16_panel[(i / dsub) * ld + i % dsub] = book[i];
  __syncthreads();
  const float *y = pq16_panel + (c < ksub ? c : 0u) * ld;
  const uint32_t q0 = blockIdx.y * kPq16TableQueries, q_pad = (Qc + QT - 1) / QT * QT;
  // q0, q_pad and QT are multiples of 4: a group of four queries lies in one tile and inside the padded chunk
  for (uint32_t q = q0; q < q0 + kPq16TableQueries && q < q_pad; q += 4) {
    float d[4];
    // a code byte that names no codeword, and the queries that pad the last tile
#pragma unroll
    for (int i = 0; i < 4; i++) d[i] = INFINITY;
    if (c < ksub) {
      const float *x = queries + (size_t)q * D + (size_t)m * dsub;
      for (uint32_t j = 0; j < dsub; j++) {
        const float yy = y[j];
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (q + i < Qc) pq16_term(d[i], x[(size_t)i * D + j], yy, j == 0);
      }
    }
    // pair index: (((tile * M + m) * 256 + c) * QT + q % QT) / 2
    uint32_t *e = tables + ((((size_t)(q / QT) * M + m) * 256 + c) * QT + q % QT) / 2;
    *reinterpret_cast<uint2 *>(e) = make_uint2(pq16_pack(d[0], d[1]), pq16_pack(d[2], d[3]));
  }
}

template <int QT, bool VEC>
__global__ __launch_bounds__(kPqThreads, kPq16Waves) void pq16_scan_kernel(PqGeom g, const uint32_t *__restrict__ tables,
                                                                           uint32_t queries,
                                                                           uint64_t *__restrict__ part) {
  extern __shared__ uint4 pq16_lds4[];
  const uint32_t M = g.M, k = g.k, cap = g.cap, t = threadIdx.x;
  const uint32_t chunk = blockIdx.x % g.G, tile = blockIdx.x / g.G;
  uint32_t *T = reinterpret_cast<uint32_t *>(pq16_lds4);                          // M x 256 x QT / 2 pairs of halves
  uint64_t *buf = reinterpret_cast<uint64_t *>(T + (size_t)(QT / 2) * M * 256);   // QT x cap
  uint64_t *thr = buf + (size_t)QT * cap;                                         // QT
  uint32_t *cnt = reinterpret_cast<uint32_t *>(thr + QT);                         // QT
  uint32_t *full = cnt + QT;                                                      // the round in which a buffer last filled
  {
    const uint4 *src = reinterpret_cast<const uint4 *>(tables + (size_t)tile * (QT / 2) * M * 256);
    for (uint32_t i = t; i < (uint32_t)QT * M * 32; i += kPqThreads) pq16_lds4[i] = src[i];
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
    pq16_score<QT, VEC>(T, w, M, acc);

    uint64_t key[QT];
    uint32_t todo = 0;
#pragma unroll
    for (int q = 0; q < QT; q++) {
      const uint32_t bits = acc[q] != acc[q] ? kPqNanBits : __float_as_uint(acc[q]);
      key[q] = (uint64_t)bits << 32 | (uint32_t)row;
      if (row < r1 && key[q] < limit[q]) todo |= 1u << q;
    }
    pq_append<QT>(buf, thr, cnt, full, cap, k, t, key, todo, limit, round);
  }
  pq_reduce<QT>(buf, thr, cnt, cap, k, (1u << QT) - 1u, t);
#pragma unroll
  for (int q = 0; q < QT; q++) {
    const uint32_t query = tile * QT + q;
    if (query < queries && t < k)
      part[((size_t)query * g.G + chunk) * k + t] = t < cnt[q] ? buf[q * cap + t] : kPqNoKey;
  }
}

// The tables of the block's pairs into T, rounded to halves.  pid[q]: the pair of slot q, ~0 for a slot without one
// (its entries are +inf; it never appends).  `stage` is QT x 64 floats.  Two barriers per sub-space; the last one
// orders the tables before the scan and the staged residuals before whatever the caller keeps in their place.
template <int QT>
__device__ __forceinline__ void ivfpq16_build_tables(const IvfPqGeom &g, const float *__restrict__ queries,
                                                     const float *__restrict__ centroid, const uint32_t *pid,
                                                     float *stage, uint32_t *T, uint32_t t) {
  const uint32_t M = g.M, dsub = g.dsub, ksub = g.ksub, D = M * dsub;
  const bool wide = (dsub & 3u) == 0 && (reinterpret_cast<uintptr_t>(g.codebooks) & 15u) == 0;
  for (uint32_t m = 0; m < M; m++) {
    for (uint32_t i = t; i < (uint32_t)QT * dsub; i += kPqThreads) {
      const uint32_t q = i / dsub, j = i - q * dsub, pair = pid[q];
      float r = 0.0f;
      if (pair != ~0u) r = queries[(size_t)(pair / g.nprobe) * D + m * dsub + j] - centroid[m * dsub + j];
      stage[q * kPq16Stage + j] = r;
    }
    __syncthreads();
    float acc[QT];
#pragma unroll
    for (int q = 0; q < QT; q++) acc[q] = INFINITY;
    if (t < ksub) {
      const float *y = g.codebooks + ((size_t)m * ksub + t) * dsub;
      if (wide) {
        for (uint32_t j = 0; j < dsub; j += 4) {
          const float4 yy = *reinterpret_cast<const float4 *>(y + j);
#pragma unroll
          for (int q = 0; q < QT; q++) {
            const float4 x = *reinterpret_cast<const float4 *>(stage + q * kPq16Stage + j);
            pq16_term(acc[q], x.x, yy.x, j == 0);
            pq16_term(acc[q], x.y, yy.y, false);
            pq16_term(acc[q], x.z, yy.z, false);
            pq16_term(acc[q], x.w, yy.w, false);
          }
        }
      } else {
        for (uint32_t j = 0; j < dsub; j++) {
          const float yy = y[j];
#pragma unroll
          for (int q = 0; q < QT; q++) pq16_term(acc[q], stage[q * kPq16Stage + j], yy, j == 0);
        }
      }
#pragma unroll
      for (int q = 0; q < QT; q++)
        if (pid[q] == ~0u) acc[q] = INFINITY;
    }
    pq16_store<QT>(T + ((size_t)m * 256 + t) * (QT / 2), acc);
    __syncthreads();
  }
}

// QT halves, as they lie in a query's table line, into an entry: one wide write (two at QT = 16)
template <int QT>
__device__ __forceinline__ void pq16_store_halves(uint32_t *e, const uint16_t (&h)[QT]) {
  uint32_t p[QT / 2];
#pragma unroll
  for (int i = 0; i < QT / 2; i++) p[i] = (uint32_t)h[2 * i] | (uint32_t)h[2 * i + 1] << 16;
  if (QT == 4) {
    *reinterpret_cast<uint2 *>(e) = make_uint2(p[0], p[1]);
  } else {
#pragma unroll
    for (int j = 0; j < QT / 8; j++)
      reinterpret_cast<uint4 *>(e)[j] = make_uint4(p[j * 4], p[j * 4 + 1], p[j * 4 + 2], p[j * 4 + 3]);
  }
}

// One IVF scan block.  LINES: non-residual lists -- the tables are copied from `qtables`, the query-level lines of
// halves (`queries` unused); else they are built from `queries` and the centroid.
template <int QT, bool VEC, bool LINES>
__device__ __forceinline__ void ivfpq16_scan_block(const IvfPqGeom &g, const float *__restrict__ queries,
                                                   const uint16_t *__restrict__ qtables,
                                                   const uint32_t *__restrict__ pair_start,
                                                   const uint32_t *__restrict__ tile_start,
                                                   const uint32_t *__restrict__ pairs, uint64_t *__restrict__ part) {
  extern __shared__ uint4 ivfpq16_lds4[];
  const uint32_t M = g.M, k = g.k, cap = g.cap, K = g.K, t = threadIdx.x;
  const uint32_t split = blockIdx.x % g.S, tile = blockIdx.x / g.S;
  if (tile >= tile_start[K]) return;   // the grid is the upper bound ceil(P / QT) + K of the tile count
  uint32_t c = 0, above = K;           // tile_start[c] <= tile < tile_start[above]
  while (above - c > 1) {
    const uint32_t mid = c + (above - c) / 2;
    if (tile_start[mid] <= tile) c = mid; else above = mid;
  }
  // the list of cluster c, whatever `offsets` holds: both ends into [0, L], the end not before the start
  const uint64_t lo = g.offsets[c] < g.L ? g.offsets[c] : g.L;
  uint64_t hi = g.offsets[c + 1] < g.L ? g.offsets[c + 1] : g.L;
  if (hi < lo) hi = lo;
  // every list is cut into S splits of whole 256-row steps by its own length
  const uint64_t steps = (hi - lo + kPqThreads - 1) / kPqThreads, rows = (steps + g.S - 1) / g.S * kPqThreads;
  const uint64_t r0 = lo + split * rows, r1 = r0 + rows < hi ? r0 + rows : hi;
  if (r0 >= hi) return;   // nothing of the list in this split: part keeps its "no key" fill
  const uint32_t p0 = pair_start[c] + (tile - tile_start[c]) * QT, left = pair_start[c + 1] - p0;
  const uint32_t live = left < (uint32_t)QT ? left : (uint32_t)QT;

  uint32_t *T = reinterpret_cast<uint32_t *>(ivfpq16_lds4);                       // M x 256 x QT / 2 pairs of halves
  uint64_t *buf = reinterpret_cast<uint64_t *>(T + (size_t)(QT / 2) * M * 256);   // QT x cap; first the staged residuals
  uint64_t *thr = buf + (size_t)QT * cap;                                         // QT
  uint32_t *cnt = reinterpret_cast<uint32_t *>(thr + QT);                         // QT
  uint32_t *pid = cnt + QT;                                                       // QT
  uint32_t *full = pid + QT;                                                      // the round in which a buffer last filled
  if (t < (uint32_t)QT) {
    thr[t] = kPqNoKey;
    cnt[t] = 0;
    pid[t] = t < live ? pairs[p0 + t] : ~0u;
  }
  if (t == 0) *full = 0;
  __syncthreads();
  if constexpr (LINES)
    pq_fill_tables<QT>(qtables, pid, live, g.nprobe, M, (uint16_t)0x7C00u, t, [&](uint32_t m, const uint16_t (&h)[QT]) {
      pq16_store_halves<QT>(T + ((size_t)m * 256 + t) * (QT / 2), h);
    });
  else   // cap >= 64 keys: QT x 512 bytes, twice the staged sub-vectors
    ivfpq16_build_tables<QT>(g, queries, g.centroids + (size_t)c * M * g.dsub, pid, reinterpret_cast<float *>(buf), T,
                             t);

  const bool dwords = (M & 3u) == 0 && (reinterpret_cast<uintptr_t>(g.codes) & 3u) == 0;
  uint64_t limit[QT];   // every lane's copy of thr[]
#pragma unroll
  for (int q = 0; q < QT; q++) limit[q] = kPqNoKey;
  uint32_t round = 0, w[16], wn[16], id, idn = 0;
  pq_load_codes<VEC>(g.codes, r0 + t, r0 + t < r1, M, dwords, wn);
  if (r0 + t < r1) idn = g.ids[r0 + t];
  for (uint64_t base = r0; base < r1; base += kPqThreads) {
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = wn[i];
    id = idn;
    const uint64_t row = base + t, next = row + kPqThreads;
    pq_load_codes<VEC>(g.codes, next, next < r1, M, dwords, wn);
    if (next < r1) idn = g.ids[next];

    float acc[QT];
    pq16_score<QT, VEC>(T, w, M, acc);

    uint64_t key[QT];
    uint32_t todo = 0;
#pragma unroll
    for (int q = 0; q < QT; q++) {
      const uint32_t bits = acc[q] != acc[q] ? kPqNanBits : __float_as_uint(acc[q]);
      key[q] = (uint64_t)bits << 32 | id;
      if (row < r1 && (uint32_t)q < live && key[q] < limit[q]) todo |= 1u << q;
    }
    pq_append<QT>(buf, thr, cnt, full, cap, k, t, key, todo, limit, round);
  }
  pq_reduce<QT>(buf, thr, cnt, cap, k, (1u << QT) - 1u, t);
#pragma unroll
  for (int q = 0; q < QT; q++)
    if ((uint32_t)q < live && t < k)
      part[((size_t)pid[q] * g.S + split) * k + t] = t < cnt[q] ? buf[q * cap + t] : kPqNoKey;
}

template <int QT, bool VEC>
__global__ __launch_bounds__(kPqThreads, kPq16Waves) void ivfpq16_scan_kernel(
    IvfPqGeom g, const float *__restrict__ queries, const uint32_t *__restrict__ pair_start,
    const uint32_t *__restrict__ tile_start, const uint32_t *__restrict__ pairs, uint64_t *__restrict__ part) {
  ivfpq16_scan_block<QT, VEC, false>(g, queries, nullptr, pair_start, tile_start, pairs, part);
}

template <int QT, bool VEC>
__global__ __launch_bounds__(kPqThreads, kPq16Waves) void ivfpq16_scan_nonres_kernel(
    IvfPqGeom g, const uint16_t *__restrict__ qtables, const uint32_t *__restrict__ pair_start,
    const uint32_t *__restrict__ tile_start, const uint32_t *__restrict__ pairs, uint64_t *__restrict__ part) {
  ivfpq16_scan_block<QT, VEC, true>(g, nullptr, qtables, pair_start, tile_start, pairs, part);
}

// a code row is read 16 bytes at a time where M is a multiple of 16 and the matrix is 16-byte aligned; a tile of 16
// never meets such a row (M <= 8 there)
bool pq16_vec(const uint8_t *codes, uint32_t M) {
  return (M & 15u) == 0 && (reinterpret_cast<uintptr_t>(codes) & 15u) == 0;
}

template <int QT>
hipError_t pq16_scan_launch(const PqGeom &g, const uint32_t *tables, uint32_t queries, uint64_t *part,
                            hipStream_t st) {
  const size_t lds = pq16_scan_lds_bytes(g.M, g.k, QT);
  const uint32_t tiles = (queries + QT - 1) / QT;
  return with_flag(QT <= 8 && pq16_vec(g.codes, g.M), [&](auto V16) {
    constexpr bool V = decltype(V16)::value && QT <= 8;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&pq16_scan_kernel<QT, V>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((pq16_scan_kernel<QT, V>), dim3(g.G * tiles), dim3(kPqThreads), lds, st, g, tables, queries,
                       part);
    return hipGetLastError();
  });
}

template <int QT>
hipError_t ivfpq16_scan_launch(const IvfPqGeom &g, const float *queries, uint32_t tiles, const uint32_t *pair_start,
                               const uint32_t *tile_start, const uint32_t *pairs, uint64_t *part, hipStream_t st) {
  const size_t lds = pq16_scan_lds_bytes(g.M, g.k, QT);
  return with_flag(QT <= 8 && pq16_vec(g.codes, g.M), [&](auto V16) {
    constexpr bool V = decltype(V16)::value && QT <= 8;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ivfpq16_scan_kernel<QT, V>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((ivfpq16_scan_kernel<QT, V>), dim3(tiles * g.S), dim3(kPqThreads), lds, st, g, queries,
                       pair_start, tile_start, pairs, part);
    return hipGetLastError();
  });
}

template <int QT>
hipError_t ivfpq16_scan_nonres_launch(const IvfPqGeom &g, const uint16_t *qtables, uint32_t tiles,
                                      const uint32_t *pair_start, const uint32_t *tile_start, const uint32_t *pairs,
                                      uint64_t *part, hipStream_t st) {
  const size_t lds = pq16_scan_lds_bytes(g.M, g.k, QT);
  return with_flag(QT <= 8 && pq16_vec(g.codes, g.M), [&](auto V16) {
    constexpr bool V = decltype(V16)::value && QT <= 8;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ivfpq16_scan_nonres_kernel<QT, V>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((ivfpq16_scan_nonres_kernel<QT, V>), dim3(tiles * g.S), dim3(kPqThreads), lds, st, g, qtables,
                       pair_start, tile_start, pairs, part);
    return hipGetLastError();
  });
}

}  // namespace

size_t pq16_scan_lds_bytes(uint32_t M, uint32_t k, uint32_t QT) {
  return (size_t)QT * ((size_t)M * 512 + (size_t)pq_candidate_cap(k) * 8 + 16) + 16;
}

uint32_t pq16_query_tile(uint32_t M, uint32_t k) {
  if (M == 0 || M > 64 || k == 0 || k > 256) return 0;
  for (uint32_t qt : {16u, 8u, 4u})   // two blocks per CU
    if (pq16_scan_lds_bytes(M, k, qt) <= kPqLdsPerCu / 2) return qt;
  return 4;                           // one: at most 147 536 bytes (M = 64, k > 128)
}

hipError_t launch_pq16_tables(const float *queries, uint32_t Qc, const float *codebooks, uint32_t M, uint32_t dsub,
                              uint32_t ksub, uint32_t QT, uint16_t *tables, hipStream_t st) {
  const size_t lds = (size_t)ksub * (dsub | 1u) * sizeof(float);
  const uint32_t q_pad = (Qc + QT - 1) / QT * QT;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&pq16_tables_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pq16_tables_kernel, dim3(M, (q_pad + kPq16TableQueries - 1) / kPq16TableQueries),
                     dim3(kPqThreads), lds, st, queries, Qc, codebooks, M, dsub, ksub, QT,
                     reinterpret_cast<uint32_t *>(tables));
  return hipGetLastError();
}

hipError_t launch_pq16_scan(const PqGeom &g, const uint16_t *tables, uint32_t queries, uint64_t *part,
                            hipStream_t st) {
  const uint32_t *t32 = reinterpret_cast<const uint32_t *>(tables);
  switch (g.QT) {
    case 4: return pq16_scan_launch<4>(g, t32, queries, part, st);
    case 8: return pq16_scan_launch<8>(g, t32, queries, part, st);
    case 16: return pq16_scan_launch<16>(g, t32, queries, part, st);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_ivfpq16_scan(const IvfPqGeom &g, const float *queries, uint32_t tiles, const uint32_t *pair_start,
                               const uint32_t *tile_start, const uint32_t *pairs, uint64_t *part, hipStream_t st) {
  switch (g.QT) {
    case 4: return ivfpq16_scan_launch<4>(g, queries, tiles, pair_start, tile_start, pairs, part, st);
    case 8: return ivfpq16_scan_launch<8>(g, queries, tiles, pair_start, tile_start, pairs, part, st);
    case 16: return ivfpq16_scan_launch<16>(g, queries, tiles, pair_start, tile_start, pairs, part, st);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_ivfpq16_scan_nonres(const IvfPqGeom &g, const uint16_t *qtables, uint32_t tiles,
                                      const uint32_t *pair_start, const uint32_t *tile_start, const uint32_t *pairs,
                                      uint64_t *part, hipStream_t st) {
  switch (g.QT) {
    case 4: return ivfpq16_scan_nonres_launch<4>(g, qtables, tiles, pair_start, tile_start, pairs, part, st);
    case 8: return ivfpq16_scan_nonres_launch<8>(g, qtables, tiles, pair_start, tile_start, pairs, part, st);
    case 16: return ivfpq16_scan_nonres_launch<16>(g, qtables, tiles, pair_start, tile_start, pairs, part, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace kmx
