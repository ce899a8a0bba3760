// pq4_scan.hip -- the two scans over 4-bit product-quantiser codes (kmamd_pq4_search, pq_job.cpp; kmamd_ivfpq4_search,
// ivfpq_job.cpp).  L2, fp32 tables, 1 <= M <= 128 sub-spaces of at most 16 codewords, k <= 256.  A code
// row is ceil(M / 2) bytes: byte j holds sub-space 2j in bits 0..3 and sub-space 2j + 1 in bits 4..7; with odd M the
// last high nibble is never looked at.  The definition is pq_scan.hip's and ivfpq_scan.hip's, term by term; the
// selection (pq_select.hpp), the merge (launch_pq_merge) and the pair sort (launch_ivfpq_group) are theirs as well.
//
// A table is M x 16 entries of QT floats (QT the query tile): 64 bytes per sub-space and query where the byte codes
// take 1 KB.  Entry (m, c) starts at float (m * 16 + c) * QT; inside it the four-query group ("quad") j sits at quad
// slot j ^ h(c), h(c) = c * (QT / 4) / 16.  At QT = 16 an entry is 16 of the 64 LDS banks wide, so without the swizzle
// the 16-byte reads of codes c and c + 4 for the same quad fall on the same four banks -- up to four ways among the
// lanes served together; with it the 16 codes of a sub-space take 16 different bank quads for every j (same at QT = 8
// with c and c + 8; at QT = 4 an entry is one quad and nothing collides).  Lanes with equal codes read one address.
// The price is the address: (c * QT + h * 4) ^ (j * 4), three XORs per nibble at QT = 16 beside the bit-field extract.
//
//   pq4_tables  grid = (group of 16 sub-spaces, group of 64 queries).  A block stages the codeword panels of its 16
//              sub-spaces (16 * ksub rows, stride dsub | 1: 64 lanes, 64 different banks); thread t owns entry
//              (sub-space t / 16, codeword t % 16) and builds it query by query, j ascending from the j = 0 term, +inf
//              for c >= ksub; written as the scan reads it: [query tile][m][16][swizzled q in tile].
//   pq4_scan    grid = (row chunk, query tile), the row chunk running fastest.  Table-stationary: the block copies its
//              tile's tables into LDS (QT * M * 64 bytes) and streams its chunk, one row per lane and step, the row's
//              nibbles in up to 16 VGPRs and the next step's in flight (16- / 4- / 1-byte loads by the row's width).  A
//              sub-space's code is one bit-field extract, (w[m / 8] >> 4 (m % 8)) & 15; one LDS read per nibble and
//              four queries (ds_read_b128) feeds QT independent add chains, m ascending from the m = 0 term.
//   ivfpq4_scan grid = (pair tile, row split) as ivfpq_scan.  The block builds its pairs' tables in its own LDS, 16
//              sub-spaces a round: thread t owns entry (t / 16, t % 16) of the round and reads its codeword straight
//              from global memory, 8 features a pass (no other thread wants it: a staged panel would be a round trip
//              through LDS for nothing); the pass's residuals fl(x_j - centroid_j) of the QT pairs, QT x 16 x 8 floats,
//              are staged in the candidate buffers, which nothing uses before the stream starts -- so the block's LDS
//              is the flat scan's and so is its tile.  Two barriers a pass, M / 16 rounds of ceil(dsub / 8) passes,
//              where the byte scan has two barriers for every sub-space.  Then the stream, ids[pos] in the key.
#include <float.h>
#include <math.h>

#include "kernels.hpp"
#include "pq_select.hpp"

namespace kmx {

namespace {

constexpr uint32_t kPq4TableQueries = 64;   // pq4_tables: queries per block, a multiple of every query tile
constexpr uint32_t kPq4Round = 16;          // sub-spaces a block serves at once, 16 threads each
constexpr uint32_t kPq4Pass = 8;            // features of a sub-space staged at once: QT x 16 x 8 floats = QT x 512 B
// waves per SIMD the scans are compiled for: two blocks of four waves per CU, as the tile rule lays out the LDS.  Left
// to itself the compiler takes 272 registers at a tile of 16 with 16-byte loads: one block per CU
constexpr int kPq4Waves = 2;

// float offset of quad 0 of codeword c's entry within its sub-space; quad j is at pq4_entry(c) ^ (j * 4)
__device__ __forceinline__ uint32_t pq4_entry(uint32_t c, uint32_t QT) { return c * QT + (((c * (QT / 4)) >> 4) << 2); }

// acc[q] = sum_m T[m][nibble m of w][q], m ascending from the m = 0 term; T is M x 16 x QT in LDS.  VEC: the row is
// whole 16-byte groups, so only a last odd nibble can be beyond M
template <int QT, bool VEC>
__device__ __forceinline__ void pq4_score(const float *__restrict__ T, const uint32_t (&w)[16], uint32_t M,
                                          float (&acc)[QT]) {
#pragma unroll
  for (int grp = 0; grp < 8; grp++)
    if ((uint32_t)grp * 16 < M) {
#pragma unroll
      for (int b = 0; b < 16; b++) {
        const int m = grp * 16 + b;
        if ((VEC && (m & 1) == 0) || (uint32_t)m < M) {
          const uint32_t code = (w[m / 8] >> (4 * (m % 8))) & 15u;
          const float *sub = T + m * 16 * QT;
          const uint32_t e = pq4_entry(code, QT);
#pragma unroll
          for (int j = 0; j < QT / 4; j++) {
            const float4 a = *reinterpret_cast<const float4 *>(sub + (e ^ (uint32_t)(j * 4)));
            const float v[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int i = 0; i < 4; i++) acc[j * 4 + i] = m == 0 ? v[i] : acc[j * 4 + i] + v[i];
          }
        }
      }
    }
}

__global__ __launch_bounds__(kPqThreads) void pq4_tables_kernel(const float *__restrict__ queries, uint32_t Qc,
                                                                const float *__restrict__ codebooks, uint32_t M,
                                                                uint32_t dsub, uint32_t ksub, uint32_t QT,
                                                                float *__restrict__ tables) {
  extern __shared__ float pq4_panel[];   // up to 16 x ksub codewords, row stride dsub | 1
  const uint32_t t = threadIdx.x, ms = t >> 4, c = t & 15u, m0 = blockIdx.x * kPq4Round, m = m0 + ms, ld = dsub | 1u;
  const uint32_t mn = M - m0 < kPq4Round ? M - m0 : kPq4Round;
  const float *book = codebooks + (size_t)m0 * ksub * dsub;
  for (uint32_t i = t; i < mn * ksub * dsub; i += kPqThreads) pq4_panel[(i / dsub) * ld + i % dsub] = book[i];
  __syncthreads();
  if (m >= M) return;
  const float *y = pq4_panel + (ms * ksub + (c < ksub ? c : 0u)) * ld;
  const uint32_t at = pq4_entry(c, QT) - c * QT;   // the swizzle of this codeword: XORed into q's quad bits
  const uint32_t q0 = blockIdx.y * kPq4TableQueries, q_pad = (Qc + QT - 1) / QT * QT;
  for (uint32_t q = q0; q < q0 + kPq4TableQueries && q < q_pad; q++) {
    float d = INFINITY;   // a nibble that names no codeword, and the queries that pad the last tile
    if (q < Qc && c < ksub) {
      const float *x = queries + (size_t)q * M * dsub + (size_t)m * dsub;
      const float t0 = x[0] - y[0];
      d = t0 * t0;
      for (uint32_t j = 1; j < dsub; j++) {
        const float tj = x[j] - y[j];
        d = d + tj * tj;
      }
    }
    tables[(((size_t)(q / QT) * M + m) * 16 + c) * QT + ((q % QT) ^ at)] = d;
  }
}

template <int QT, bool VEC>
__global__ __launch_bounds__(kPqThreads, kPq4Waves) void pq4_scan_kernel(PqGeom g, const float *__restrict__ tables,
                                                                         uint32_t queries,
                                                                         uint64_t *__restrict__ part) {
  extern __shared__ float4 pq4_lds4[];
  const uint32_t M = g.M, W = (M + 1) / 2, k = g.k, cap = g.cap, t = threadIdx.x;
  const uint32_t chunk = blockIdx.x % g.G, tile = blockIdx.x / g.G;
  float *T = reinterpret_cast<float *>(pq4_lds4);                          // M x 16 x QT
  uint64_t *buf = reinterpret_cast<uint64_t *>(T + (size_t)QT * M * 16);   // QT x cap
  uint64_t *thr = buf + (size_t)QT * cap;                                  // QT
  uint32_t *cnt = reinterpret_cast<uint32_t *>(thr + QT);                  // QT
  uint32_t *full = cnt + QT;                                               // the round in which a buffer last filled
  {
    const float4 *src = reinterpret_cast<const float4 *>(tables + (size_t)tile * QT * M * 16);
    for (uint32_t i = t; i < (uint32_t)QT * M * 4; i += kPqThreads) pq4_lds4[i] = src[i];
    if (t < (uint32_t)QT) { thr[t] = kPqNoKey; cnt[t] = 0; }
    if (t == 0) *full = 0;
  }
  __syncthreads();

  const bool dwords = (W & 3u) == 0 && (reinterpret_cast<uintptr_t>(g.codes) & 3u) == 0;
  const uint64_t r0 = (uint64_t)chunk * g.R, r1 = r0 + g.R < g.N ? r0 + g.R : g.N;
  uint64_t limit[QT];   // every lane's copy of thr[]
#pragma unroll
  for (int q = 0; q < QT; q++) limit[q] = kPqNoKey;
  uint32_t round = 0, w[16], wn[16];
  pq_load_codes<VEC>(g.codes, r0 + t, r0 + t < r1, W, dwords, wn);
  for (uint64_t base = r0; base < r1; base += kPqThreads) {
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = wn[i];
    const uint64_t row = base + t, next = row + kPqThreads;
    pq_load_codes<VEC>(g.codes, next, next < r1, W, dwords, wn);

    float acc[QT];
    pq4_score<QT, VEC>(T, w, M, acc);

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

// one term of a table entry: acc = fl(fl(x - y)^2) for the j = 0 term, else fl(acc + fl(fl(x - y)^2))
__device__ __forceinline__ void pq4_term(float &acc, float x, float y, bool first) {
  const float d = x - y;
  acc = first ? d * d : acc + d * d;
}

// The tables of the block's pairs into T.  pid[q]: the pair of slot q, ~0 for a slot without one (its entries are +inf;
// it never appends).  `stage` is QT x 16 x 8 floats.  The last barrier orders the tables before the scan and the
// staged residuals before whatever the caller keeps in their place.
template <int QT>
__device__ __forceinline__ void ivfpq4_build_tables(const IvfPqGeom &g, const float *__restrict__ queries,
                                                    const float *__restrict__ centroid, const uint32_t *pid,
                                                    float *stage, float *T, uint32_t t) {
  const uint32_t M = g.M, dsub = g.dsub, ksub = g.ksub, D = M * dsub, ms = t >> 4, c = t & 15u;
  const bool wide = (dsub & 3u) == 0 && (reinterpret_cast<uintptr_t>(g.codebooks) & 15u) == 0;
  for (uint32_t m0 = 0; m0 < M; m0 += kPq4Round) {
    const uint32_t m = m0 + ms;
    const bool mine = m < M && c < ksub;
    const float *y = g.codebooks + ((size_t)(mine ? m : 0u) * ksub + (mine ? c : 0u)) * dsub;
    float acc[QT];
#pragma unroll
    for (int q = 0; q < QT; q++) acc[q] = INFINITY;
    for (uint32_t j0 = 0; j0 < dsub; j0 += kPq4Pass) {
      const uint32_t jn = dsub - j0 < kPq4Pass ? dsub - j0 : kPq4Pass;
      float yy[kPq4Pass];   // this pass of the thread's codeword, in flight over the staging
#pragma unroll
      for (int j = 0; j < (int)kPq4Pass; j++) yy[j] = 0.0f;
      if (wide) {
        const float4 a = *reinterpret_cast<const float4 *>(y + j0);
        yy[0] = a.x; yy[1] = a.y; yy[2] = a.z; yy[3] = a.w;
        if (jn > 4) {
          const float4 b = *reinterpret_cast<const float4 *>(y + j0 + 4);
          yy[4] = b.x; yy[5] = b.y; yy[6] = b.z; yy[7] = b.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < (int)kPq4Pass; j++)
          if ((uint32_t)j < jn) yy[j] = y[j0 + j];
      }
      for (uint32_t i = t; i < (uint32_t)QT * kPq4Round * kPq4Pass; i += kPqThreads) {
        const uint32_t q = i >> 7, s = (i >> 3) & 15u, j = i & 7u, pair = pid[q];
        float r = 0.0f;
        if (pair != ~0u && m0 + s < M && j < jn) {
          const uint32_t col = (m0 + s) * dsub + j0 + j;
          r = queries[(size_t)(pair / g.nprobe) * D + col] - centroid[col];
        }
        stage[i] = r;
      }
      __syncthreads();
      if (mine) {
#pragma unroll
        for (int q = 0; q < QT; q++) {
          const float4 *sv = reinterpret_cast<const float4 *>(stage + (q * kPq4Round + ms) * kPq4Pass);
          const float4 a = sv[0], b = sv[1];
          const float x[kPq4Pass] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
          for (int j = 0; j < (int)kPq4Pass; j++)
            if ((uint32_t)j < jn) pq4_term(acc[q], x[j], yy[j], j0 == 0 && j == 0);
        }
      }
      __syncthreads();   // the pass is read before the next one is staged
    }
    if (m < M) {
#pragma unroll
      for (int q = 0; q < QT; q++)
        if (pid[q] == ~0u) acc[q] = INFINITY;
      float *sub = T + (size_t)m * 16 * QT;
      const uint32_t e = pq4_entry(c, QT);
#pragma unroll
      for (int j = 0; j < QT / 4; j++)
        *reinterpret_cast<float4 *>(sub + (e ^ (uint32_t)(j * 4))) =
            make_float4(acc[j * 4], acc[j * 4 + 1], acc[j * 4 + 2], acc[j * 4 + 3]);
    }
  }
  __syncthreads();
}

template <int QT, bool VEC>
__global__ __launch_bounds__(kPqThreads, kPq4Waves) void ivfpq4_scan_kernel(
    IvfPqGeom g, const float *__restrict__ queries, const uint32_t *__restrict__ pair_start,
    const uint32_t *__restrict__ tile_start, const uint32_t *__restrict__ pairs, uint64_t *__restrict__ part) {
  extern __shared__ float4 ivfpq4_lds4[];
  const uint32_t M = g.M, W = (M + 1) / 2, k = g.k, cap = g.cap, K = g.K, t = threadIdx.x;
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

  float *T = reinterpret_cast<float *>(ivfpq4_lds4);                       // M x 16 x QT
  uint64_t *buf = reinterpret_cast<uint64_t *>(T + (size_t)QT * M * 16);   // QT x cap; first the staged residuals
  uint64_t *thr = buf + (size_t)QT * cap;                                  // QT
  uint32_t *cnt = reinterpret_cast<uint32_t *>(thr + QT);                  // QT
  uint32_t *pid = cnt + QT;                                                // QT
  uint32_t *full = pid + QT;                                               // the round in which a buffer last filled
  if (t < (uint32_t)QT) {
    thr[t] = kPqNoKey;
    cnt[t] = 0;
    pid[t] = t < live ? pairs[p0 + t] : ~0u;
  }
  if (t == 0) *full = 0;
  __syncthreads();
  // cap >= 64 keys: QT x 512 bytes, the staged pass exactly
  ivfpq4_build_tables<QT>(g, queries, g.centroids + (size_t)c * M * g.dsub, pid, reinterpret_cast<float *>(buf), T, t);

  const bool dwords = (W & 3u) == 0 && (reinterpret_cast<uintptr_t>(g.codes) & 3u) == 0;
  uint64_t limit[QT];   // every lane's copy of thr[]
#pragma unroll
  for (int q = 0; q < QT; q++) limit[q] = kPqNoKey;
  uint32_t round = 0, w[16], wn[16], id, idn = 0;
  pq_load_codes<VEC>(g.codes, r0 + t, r0 + t < r1, W, dwords, wn);
  if (r0 + t < r1) idn = g.ids[r0 + t];
  for (uint64_t base = r0; base < r1; base += kPqThreads) {
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = wn[i];
    id = idn;
    const uint64_t row = base + t, next = row + kPqThreads;
    pq_load_codes<VEC>(g.codes, next, next < r1, W, dwords, wn);
    if (next < r1) idn = g.ids[next];

    float acc[QT];
    pq4_score<QT, VEC>(T, w, M, acc);

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

// a packed row is read 16 bytes at a time where it is whole 16-byte groups and the matrix is 16-byte aligned
bool pq4_vec(const uint8_t *codes, uint32_t M) {
  return (((M + 1) / 2) & 15u) == 0 && (reinterpret_cast<uintptr_t>(codes) & 15u) == 0;
}

template <int QT>
hipError_t pq4_scan_launch(const PqGeom &g, const float *tables, uint32_t queries, uint64_t *part, hipStream_t st) {
  const size_t lds = pq4_scan_lds_bytes(g.M, g.k, QT);
  const uint32_t tiles = (queries + QT - 1) / QT;
  return with_flag(pq4_vec(g.codes, g.M), [&](auto V16) {
    constexpr bool V = decltype(V16)::value;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&pq4_scan_kernel<QT, V>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((pq4_scan_kernel<QT, V>), dim3(g.G * tiles), dim3(kPqThreads), lds, st, g, tables, queries, part);
    return hipGetLastError();
  });
}

template <int QT>
hipError_t ivfpq4_scan_launch(const IvfPqGeom &g, const float *queries, uint32_t tiles, const uint32_t *pair_start,
                              const uint32_t *tile_start, const uint32_t *pairs, uint64_t *part, hipStream_t st) {
  const size_t lds = pq4_scan_lds_bytes(g.M, g.k, QT);
  return with_flag(pq4_vec(g.codes, g.M), [&](auto V16) {
    constexpr bool V = decltype(V16)::value;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ivfpq4_scan_kernel<QT, V>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((ivfpq4_scan_kernel<QT, V>), dim3(tiles * g.S), dim3(kPqThreads), lds, st, g, queries,
                       pair_start, tile_start, pairs, part);
    return hipGetLastError();
  });
}

}  // namespace

size_t pq4_scan_lds_bytes(uint32_t M, uint32_t k, uint32_t QT) {
  return (size_t)QT * ((size_t)M * 64 + (size_t)pq_candidate_cap(k) * 8 + 16) + 16;
}

uint32_t pq4_query_tile(uint32_t M, uint32_t k) {
  if (M == 0 || M > 128 || k == 0 || k > 256) return 0;
  for (uint32_t qt : {16u, 8u, 4u})   // two blocks per CU; 4 fits at every M and k
    if (pq4_scan_lds_bytes(M, k, qt) <= kPqLdsPerCu / 2) return qt;
  return 0;
}

hipError_t launch_pq4_tables(const float *queries, uint32_t Qc, const float *codebooks, uint32_t M, uint32_t dsub,
                             uint32_t ksub, uint32_t QT, float *tables, hipStream_t st) {
  const size_t lds = (size_t)kPq4Round * ksub * (dsub | 1u) * sizeof(float);
  const uint32_t q_pad = (Qc + QT - 1) / QT * QT;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&pq4_tables_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pq4_tables_kernel, dim3((M + kPq4Round - 1) / kPq4Round,
                                             (q_pad + kPq4TableQueries - 1) / kPq4TableQueries),
                     dim3(kPqThreads), lds, st, queries, Qc, codebooks, M, dsub, ksub, QT, tables);
  return hipGetLastError();
}

hipError_t launch_pq4_scan(const PqGeom &g, const float *tables, uint32_t queries, uint64_t *part, hipStream_t st) {
  switch (g.QT) {
    case 4: return pq4_scan_launch<4>(g, tables, queries, part, st);
    case 8: return pq4_scan_launch<8>(g, tables, queries, part, st);
    case 16: return pq4_scan_launch<16>(g, tables, queries, part, st);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_ivfpq4_scan(const IvfPqGeom &g, const float *queries, uint32_t tiles, const uint32_t *pair_start,
                              const uint32_t *tile_start, const uint32_t *pairs, uint64_t *part, hipStream_t st) {
  switch (g.QT) {
    case 4: return ivfpq4_scan_launch<4>(g, queries, tiles, pair_start, tile_start, pairs, part, st);
    case 8: return ivfpq4_scan_launch<8>(g, queries, tiles, pair_start, tile_start, pairs, part, st);
    case 16: return ivfpq4_scan_launch<16>(g, queries, tiles, pair_start, tile_start, pairs, part, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace kmx
