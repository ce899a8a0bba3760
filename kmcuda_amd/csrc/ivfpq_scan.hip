// ivfpq_scan.hip -- IVF-PQ search: product-quantiser codes of residuals (row minus its coarse centroid) in cluster
// lists, probed by asymmetric distance computation (kmamd_ivfpq_search, ivfpq_job.cpp).  L2, fp32
// tables, uint8 codes, 1 <= M <= 64 sub-spaces, k <= 256, nprobe <= 64.  The table of the scan depends on the (query,
// probed cluster) pair, so the unit of work is the pair and the pairs that can share streamed code bytes are those of
// one cluster.
//
//   ivfpq_count / ivfpq_prefix / ivfpq_scatter   a counting sort of the live pairs of a query chunk by cluster, on the
//              device.  Pair i = query * nprobe + rank is live when its probe is < K and no earlier rank of the query
//              names the same cluster.  count: one thread per pair, an integer atomic per live pair into hist[K].
//              prefix: one block walks K, 256 clusters a round, and writes the exclusive prefixes of n_c (where
//              cluster c's pairs start) and of ceil(n_c / QT) (where its tiles start), K + 1 entries each.  scatter:
//              pairs[cursor[c]++] = i.  The order of a cluster's pairs is the arrival order; it decides which pairs
//              share a block and nothing else.
//   ivfpq_scan grid = (pair tile, row split), the split running fastest; launched with the upper bound of the tile
//              count -- a block finds its cluster by binary search in the tile prefix or leaves.  A block owns up to QT
//              pairs of ONE cluster and a split of that cluster's list, clamped into [0, L].  It builds the QT tables
//              in its own LDS, T[m][code][q] as pq_scan reads them: per sub-space the QT residual sub-vectors
//              fl(x_j - centroid_j) are staged in LDS (QT x 64 floats), thread c walks codeword c once -- 16 bytes of
//              it at a time where dsub allows -- against all QT staged vectors (LDS broadcast reads), QT add chains in
//              ascending j, and stores the QT adjacent entries with one wide LDS write; +inf for c >= ksub.  No table
//              goes through global memory.  Then pq_scan's stream over the split's rows: one row per lane and step,
//              16- / 4- / 1-byte code loads, the next step's bytes and id in flight, one ds_read_b128 per byte and
//              four pairs, the thresholded candidate buffers of pq_select.hpp with ids[pos] in the key.  k sorted keys
//              go to part[((query * nprobe + rank) * S + split) * k ..); the host pre-fills part with "no key", which
//              is what dead pairs and splits past a list's end leave behind.  launch_pq_merge reduces them per query.
//   ivfpq_residuals   out[i][j] = fl(x[i][j] - centroids[a[i]][j]), NaN where a[i] >= K: what the codebooks are trained
//              on and the corpus is encoded from.
//
// The precomputed-term variant (kmamd_ivfpq_search_precomputed) splits a pair's table entry
// |x - g - y|^2 over a sub-space into |x - g|^2 + (|y|^2 + 2 g.y) - 2 x.y, with arithmetic -- and bits -- of its own:
//   ivfpq_terms        once per index: A[cluster][m][c] = fl(n + 2 s), n = sum_j fl(y_j y_j), s = sum_j fl(g_j y_j).
//              grid = (sub-space, group of 64 clusters); the codeword panel in LDS at stride dsub | 1, the group's
//              centroid sub-vectors beside it (broadcast reads); thread c owns codeword c, one entry per cluster.
//   ivfpq_query_terms  once per query chunk: B[query][m][256], B = sum_j fl(x_j y_j): pq_tables' grid and panel with
//              a product in place of a squared difference; a pair's sub-space is one 1 KB line.  Columns >= ksub are
//              not written and never read.
//   ivfpq_pair_norms   one thread per pair: t1 = sum_{j < D} fl(fl(x_j - g_j)^2) of the live pairs.
//   ivfpq_scan_pre     ivfpq_scan with another prologue: no staging tile and no barrier per sub-space.  Thread c
//              loads A[cluster][m][c] and the QT values B[query of slot q][m][c] of 16 / QT sub-spaces at a time, the
//              next group's loads issued before this group's entries T = fl(A - 2 B) go to LDS with the same wide
//              store; one barrier, then the same stream.  Behind pq_score a lane adds its slot's t1 (in registers) and
//              turns a result that is negative or -0 into +0 before the key is formed.
//
// Non-residual lists (kmamd_ivfpq_search_nonresidual): the codes are those of the rows themselves, so
// the table is pq_search's and depends on the query only.
//   ivfpq_query_tables   once per query chunk: pq_tables' entries, bit for bit, in ivfpq_query_terms' grid and layout
//              [query][m][256] (1 KB lines), as floats or rounded once to halves (512-byte lines, for pq16_scan.hip's
//              scan); all 256 columns are written.
//   ivfpq_scan_nonres      ivfpq_scan with a third prologue, pq_fill_tables (pq_select.hpp): thread c copies column c of
//              its pairs' lines into T[m][c][q], a group of sub-spaces at a time with the next group in flight; no
//              arithmetic, no staging tile, one barrier.  Then the same stream.
#include <float.h>
#include <math.h>

#include <hip/hip_fp16.h>

#include "kernels.hpp"
#include "pq_select.hpp"

namespace kmx {

namespace {

constexpr uint32_t kIvfPqStage = 64;   // floats of one staged residual sub-vector: the largest dsub

// the cluster pair i probes, K where the pair is dead: a filler, or a cluster an earlier rank of the query names
__device__ __forceinline__ uint32_t ivfpq_pair_cluster(const uint32_t *__restrict__ probes, uint32_t i, uint32_t nprobe,
                                                       uint32_t K) {
  const uint32_t rank = i % nprobe;
  const uint32_t *row = probes + (size_t)(i - rank);
  const uint32_t p = row[rank];
  if (p >= K) return K;
  for (uint32_t r = 0; r < rank; r++)
    if (row[r] == p) return K;
  return p;
}

__global__ __launch_bounds__(kPqThreads) void ivfpq_count_kernel(const uint32_t *__restrict__ probes, uint32_t P,
                                                                 uint32_t nprobe, uint32_t K,
                                                                 uint32_t *__restrict__ hist) {
  const uint64_t i = (uint64_t)blockIdx.x * kPqThreads + threadIdx.x;
  if (i >= P) return;
  const uint32_t c = ivfpq_pair_cluster(probes, (uint32_t)i, nprobe, K);
  if (c < K) atomicAdd(hist + c, 1u);
}

__global__ __launch_bounds__(kPqThreads) void ivfpq_prefix_kernel(const uint32_t *__restrict__ hist, uint32_t K,
                                                                  uint32_t QT, uint32_t *__restrict__ pair_start,
                                                                  uint32_t *__restrict__ tile_start,
                                                                  uint32_t *__restrict__ cursor) {
  __shared__ uint32_t sp[kPqThreads], st[kPqThreads];
  const uint32_t t = threadIdx.x;
  uint32_t pairs = 0, tiles = 0;   // of the clusters before this round, the same in every thread
  for (uint32_t base = 0; base < K; base += kPqThreads) {
    const uint32_t c = base + t, n = c < K ? hist[c] : 0u, nt = (n + QT - 1) / QT;
    sp[t] = n;
    st[t] = nt;
    __syncthreads();
    for (uint32_t d = 1; d < kPqThreads; d <<= 1) {
      const uint32_t a = t >= d ? sp[t - d] : 0u, b = t >= d ? st[t - d] : 0u;
      __syncthreads();
      sp[t] += a;
      st[t] += b;
      __syncthreads();
    }
    if (c < K) {
      pair_start[c] = cursor[c] = pairs + sp[t] - n;
      tile_start[c] = tiles + st[t] - nt;
    }
    pairs += sp[kPqThreads - 1];
    tiles += st[kPqThreads - 1];
    __syncthreads();
  }
  if (t == 0) {
    pair_start[K] = pairs;
    tile_start[K] = tiles;
  }
}

__global__ __launch_bounds__(kPqThreads) void ivfpq_scatter_kernel(const uint32_t *__restrict__ probes, uint32_t P,
                                                                   uint32_t nprobe, uint32_t K,
                                                                   uint32_t *__restrict__ cursor,
                                                                   uint32_t *__restrict__ pairs) {
  const uint64_t i = (uint64_t)blockIdx.x * kPqThreads + threadIdx.x;
  if (i >= P) return;
  const uint32_t c = ivfpq_pair_cluster(probes, (uint32_t)i, nprobe, K);
  if (c < K) pairs[atomicAdd(cursor + c, 1u)] = (uint32_t)i;
}

// one term of a table entry: acc = fl(fl(x - y)^2) for the j = 0 term, else fl(acc + fl(fl(x - y)^2))
__device__ __forceinline__ void ivfpq_term(float &acc, float x, float y, bool first) {
  const float d = x - y;
  acc = first ? d * d : acc + d * d;
}

// The tables of the block's pairs into T[m][code][q].  pid[q]: the pair of slot q, ~0 for a slot without one (its
// entries are +inf; it never appends).  Two barriers per sub-space; the last one orders the tables before the scan.
template <int QT>
__device__ __forceinline__ void ivfpq_build_tables(const IvfPqGeom &g, const float *__restrict__ queries,
                                                   const float *__restrict__ centroid, const uint32_t *pid,
                                                   float *stage, float *T, uint32_t t) {
  const uint32_t M = g.M, dsub = g.dsub, ksub = g.ksub, D = M * dsub;
  const bool wide = (dsub & 3u) == 0 && (reinterpret_cast<uintptr_t>(g.codebooks) & 15u) == 0;
  for (uint32_t m = 0; m < M; m++) {
    for (uint32_t i = t; i < (uint32_t)QT * dsub; i += kPqThreads) {
      const uint32_t q = i / dsub, j = i - q * dsub, pair = pid[q];
      float r = 0.0f;
      if (pair != ~0u) r = queries[(size_t)(pair / g.nprobe) * D + m * dsub + j] - centroid[m * dsub + j];
      stage[q * kIvfPqStage + j] = r;
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
            const float4 x = *reinterpret_cast<const float4 *>(stage + q * kIvfPqStage + j);
            ivfpq_term(acc[q], x.x, yy.x, j == 0);
            ivfpq_term(acc[q], x.y, yy.y, false);
            ivfpq_term(acc[q], x.z, yy.z, false);
            ivfpq_term(acc[q], x.w, yy.w, false);
          }
        }
      } else {
        for (uint32_t j = 0; j < dsub; j++) {
          const float yy = y[j];
#pragma unroll
          for (int q = 0; q < QT; q++) ivfpq_term(acc[q], stage[q * kIvfPqStage + j], yy, j == 0);
        }
      }
#pragma unroll
      for (int q = 0; q < QT; q++)
        if (pid[q] == ~0u) acc[q] = INFINITY;
    }
    float *e = T + ((size_t)m * 256 + t) * QT;
    if (QT == 2) {
      *reinterpret_cast<float2 *>(e) = make_float2(acc[0], acc[1]);
    } else {
#pragma unroll
      for (int j = 0; j < QT / 4; j++)
        reinterpret_cast<float4 *>(e)[j] = make_float4(acc[j * 4], acc[j * 4 + 1], acc[j * 4 + 2], acc[j * 4 + 3]);
    }
    __syncthreads();
  }
}

constexpr int kIvfPqPreLoads = 16;   // B values a thread keeps in flight per group of the precomputed prologue

// The tables of the block's pairs from precomputed terms: T[m][code][q] = fl(A[m][code] - 2 B[query of q][m][code]),
// +inf for code >= ksub and for a slot without a pair.  a_row: the cluster's M x ksub terms; t1[q]: the slot's norm.
// B is indexed in 32 bits: the host keeps a chunk's B within 2^27 floats.  One barrier, at the end.
template <int QT>
__device__ __forceinline__ void ivfpq_fill_tables(const IvfPqGeom &g, const float *__restrict__ a_row,
                                                  const float *__restrict__ qterms, const float *__restrict__ norms,
                                                  const uint32_t *pid, uint32_t live, float *T, uint32_t t,
                                                  float (&t1)[QT]) {
  constexpr int G = kIvfPqPreLoads / QT;
  const uint32_t M = g.M, ksub = g.ksub;
  const bool col = t < ksub;
  uint32_t at[QT];   // B's index of (query of slot q, m = 0, column t)
#pragma unroll
  for (int q = 0; q < QT; q++) {
    const bool have = (uint32_t)q < live;
    const uint32_t pair = have ? pid[q] : 0u;
    at[q] = have ? (pair / g.nprobe * M) * 256u + t : 0u;
    t1[q] = have ? norms[pair] : 0.0f;
  }
  float a[G], b[G][QT], an[G], bn[G][QT];
  auto load = [&](uint32_t m0, float (&av)[G], float (&bv)[G][QT]) {
#pragma unroll
    for (int i = 0; i < G; i++) {
      const uint32_t m = m0 + i;
      av[i] = 0.0f;
#pragma unroll
      for (int q = 0; q < QT; q++) bv[i][q] = 0.0f;
      if (col && m < M) {
        av[i] = a_row[m * ksub + t];
#pragma unroll
        for (int q = 0; q < QT; q++)
          if ((uint32_t)q < live) bv[i][q] = qterms[at[q] + m * 256u];
      }
    }
  };
  load(0, an, bn);
  for (uint32_t m0 = 0; m0 < M; m0 += G) {
#pragma unroll
    for (int i = 0; i < G; i++) {
      a[i] = an[i];
#pragma unroll
      for (int q = 0; q < QT; q++) b[i][q] = bn[i][q];
    }
    load(m0 + G, an, bn);   // in flight over this group's stores
#pragma unroll
    for (int i = 0; i < G; i++) {
      const uint32_t m = m0 + i;
      if (m < M) {
        float e[QT];
#pragma unroll
        for (int q = 0; q < QT; q++) e[q] = col && (uint32_t)q < live ? a[i] - 2.0f * b[i][q] : INFINITY;
        float *dst = T + ((size_t)m * 256 + t) * QT;
        if (QT == 2) {
          *reinterpret_cast<float2 *>(dst) = make_float2(e[0], e[1]);
        } else {
#pragma unroll
          for (int j = 0; j < QT / 4; j++)
            reinterpret_cast<float4 *>(dst)[j] = make_float4(e[j * 4], e[j * 4 + 1], e[j * 4 + 2], e[j * 4 + 3]);
        }
      }
    }
  }
  __syncthreads();
}

// where a scan block's tables come from
enum IvfPqSource {
  kIvfPqResiduals,     // built from `queries` and the centroid through a staging tile
  kIvfPqTerms,         // precomputed terms (terms, qterms, norms): no staging tile, a lane adds its slot's norm to the score
  kIvfPqQueryTables,   // non-residual lists: copied from the query-level tables, which take `qterms`' place and layout
};

// One scan block; `queries` is read by kIvfPqResiduals only, `terms` and `norms` by kIvfPqTerms only.
template <int QT, bool VEC, IvfPqSource SRC>
__device__ __forceinline__ void ivfpq_scan_block(const IvfPqGeom &g, const float *__restrict__ queries,
                                                 const float *__restrict__ terms, const float *__restrict__ qterms,
                                                 const float *__restrict__ norms,
                                                 const uint32_t *__restrict__ pair_start,
                                                 const uint32_t *__restrict__ tile_start,
                                                 const uint32_t *__restrict__ pairs, uint64_t *__restrict__ part) {
  extern __shared__ float4 ivfpq_lds4[];
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

  float *T = reinterpret_cast<float *>(ivfpq_lds4);                          // M x 256 x QT
  float *stage = T + (size_t)QT * M * 256;                                   // QT x 64, kIvfPqResiduals only
  uint64_t *buf = reinterpret_cast<uint64_t *>(stage + (SRC == kIvfPqResiduals ? QT * kIvfPqStage : 0));   // QT x cap
  uint64_t *thr = buf + (size_t)QT * cap;                                    // QT
  uint32_t *cnt = reinterpret_cast<uint32_t *>(thr + QT);                    // QT
  uint32_t *pid = cnt + QT;                                                  // QT
  uint32_t *full = pid + QT;                                                 // the round in which a buffer last filled
  if (t < (uint32_t)QT) {
    thr[t] = kPqNoKey;
    cnt[t] = 0;
    pid[t] = t < live ? pairs[p0 + t] : ~0u;
  }
  if (t == 0) *full = 0;
  __syncthreads();
  float t1[SRC == kIvfPqTerms ? QT : 1];   // the norms of the block's pairs
  if constexpr (SRC == kIvfPqTerms)
    ivfpq_fill_tables<QT>(g, terms + (size_t)c * M * g.ksub, qterms, norms, pid, live, T, t, t1);
  else if constexpr (SRC == kIvfPqQueryTables)
    pq_fill_tables<QT>(qterms, pid, live, g.nprobe, M, INFINITY, t, [&](uint32_t m, const float (&e)[QT]) {
      float *dst = T + ((size_t)m * 256 + t) * QT;
      if (QT == 2) {
        *reinterpret_cast<float2 *>(dst) = make_float2(e[0], e[1]);
      } else {
#pragma unroll
        for (int j = 0; j < QT / 4; j++)
          reinterpret_cast<float4 *>(dst)[j] = make_float4(e[j * 4], e[j * 4 + 1], e[j * 4 + 2], e[j * 4 + 3]);
      }
    });
  else
    ivfpq_build_tables<QT>(g, queries, g.centroids + (size_t)c * M * g.dsub, pid, stage, T, t);

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
    pq_score<QT, VEC>(T, w, M, acc);

    uint64_t key[QT];
    uint32_t todo = 0;
#pragma unroll
    for (int q = 0; q < QT; q++) {
      if constexpr (SRC == kIvfPqTerms) {
        const float d = t1[q] + acc[q];
        acc[q] = d <= 0.0f ? 0.0f : d;   // cancellation can leave a negative sum: the keys compare bits unsigned
      }
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
__global__ __launch_bounds__(kPqThreads) void ivfpq_scan_kernel(IvfPqGeom g, const float *__restrict__ queries,
                                                                const uint32_t *__restrict__ pair_start,
                                                                const uint32_t *__restrict__ tile_start,
                                                                const uint32_t *__restrict__ pairs,
                                                                uint64_t *__restrict__ part) {
  ivfpq_scan_block<QT, VEC, kIvfPqResiduals>(g, queries, nullptr, nullptr, nullptr, pair_start, tile_start, pairs,
                                             part);
}

template <int QT, bool VEC>
__global__ __launch_bounds__(kPqThreads) void ivfpq_scan_pre_kernel(IvfPqGeom g, const float *__restrict__ terms,
                                                                    const float *__restrict__ qterms,
                                                                    const float *__restrict__ norms,
                                                                    const uint32_t *__restrict__ pair_start,
                                                                    const uint32_t *__restrict__ tile_start,
                                                                    const uint32_t *__restrict__ pairs,
                                                                    uint64_t *__restrict__ part) {
  ivfpq_scan_block<QT, VEC, kIvfPqTerms>(g, nullptr, terms, qterms, norms, pair_start, tile_start, pairs, part);
}

template <int QT, bool VEC>
__global__ __launch_bounds__(kPqThreads) void ivfpq_scan_nonres_kernel(IvfPqGeom g, const float *__restrict__ qtables,
                                                                     const uint32_t *__restrict__ pair_start,
                                                                     const uint32_t *__restrict__ tile_start,
                                                                     const uint32_t *__restrict__ pairs,
                                                                     uint64_t *__restrict__ part) {
  ivfpq_scan_block<QT, VEC, kIvfPqQueryTables>(g, nullptr, nullptr, qtables, nullptr, pair_start, tile_start, pairs,
                                               part);
}

__global__ __launch_bounds__(kPqThreads) void ivfpq_residuals_kernel(const float *__restrict__ x,
                                                                     const float *__restrict__ centroids,
                                                                     const uint32_t *__restrict__ a, uint64_t N,
                                                                     uint32_t D, uint32_t K, float *__restrict__ out) {
  const uint64_t total = N * D;
  const uint64_t stride = (uint64_t)gridDim.x * kPqThreads;
  for (uint64_t at = (uint64_t)blockIdx.x * kPqThreads + threadIdx.x; at < total; at += stride) {
    const uint64_t i = at / D;
    const uint32_t j = (uint32_t)(at - i * D), c = a[i];
    out[at] = c < K ? x[at] - centroids[(size_t)c * D + j] : NAN;
  }
}

constexpr uint32_t kIvfPqTermGroup = 64;   // clusters (ivfpq_terms) or queries (ivfpq_query_terms) of one block round

// the codeword panel of sub-space m into LDS, row stride dsub | 1: no bank conflict at any dsub
__device__ __forceinline__ void ivfpq_stage_panel(const float *__restrict__ codebooks, uint32_t m, uint32_t dsub,
                                                  uint32_t ksub, float *panel) {
  const float *book = codebooks + (size_t)m * ksub * dsub;
  const uint32_t ld = dsub | 1u;
  for (uint32_t i = threadIdx.x; i < ksub * dsub; i += kPqThreads) panel[(i / dsub) * ld + i % dsub] = book[i];
}

// sum_j fl(x_j y_j), j ascending from the j = 0 term
__device__ __forceinline__ float ivfpq_dot(const float *x, const float *y, uint32_t dsub) {
  float s = x[0] * y[0];
  for (uint32_t j = 1; j < dsub; j++) s = s + x[j] * y[j];
  return s;
}

__global__ __launch_bounds__(kPqThreads) void ivfpq_terms_kernel(const float *__restrict__ centroids,
                                                                 const float *__restrict__ codebooks, uint32_t K,
                                                                 uint32_t M, uint32_t dsub, uint32_t ksub,
                                                                 float *__restrict__ terms) {
  extern __shared__ float ivfpq_panel[];   // ksub x (dsub | 1), then kIvfPqTermGroup x dsub centroid sub-vectors
  const uint32_t m = blockIdx.x, c = threadIdx.x, ld = dsub | 1u;
  float *cen = ivfpq_panel + ksub * ld;
  ivfpq_stage_panel(codebooks, m, dsub, ksub, ivfpq_panel);
  __syncthreads();
  const float *y = ivfpq_panel + (c < ksub ? c : 0u) * ld;
  const float n = ivfpq_dot(y, y, dsub);
  for (uint64_t p0 = (uint64_t)blockIdx.y * kIvfPqTermGroup; p0 < K; p0 += (uint64_t)gridDim.y * kIvfPqTermGroup) {
    const uint32_t pn = K - p0 < kIvfPqTermGroup ? (uint32_t)(K - p0) : kIvfPqTermGroup;
    for (uint32_t i = c; i < pn * dsub; i += kPqThreads)
      cen[i] = centroids[(size_t)(p0 + i / dsub) * M * dsub + m * dsub + i % dsub];
    __syncthreads();
    if (c < ksub)
      for (uint32_t p = 0; p < pn; p++)
        terms[((size_t)(p0 + p) * M + m) * ksub + c] = n + 2.0f * ivfpq_dot(cen + p * dsub, y, dsub);
    __syncthreads();
  }
}

__global__ __launch_bounds__(kPqThreads) void ivfpq_query_terms_kernel(const float *__restrict__ queries, uint32_t Qc,
                                                                       const float *__restrict__ codebooks, uint32_t M,
                                                                       uint32_t dsub, uint32_t ksub,
                                                                       float *__restrict__ qterms) {
  extern __shared__ float ivfpq_panel[];   // ksub x (dsub | 1)
  const uint32_t m = blockIdx.x, c = threadIdx.x;
  ivfpq_stage_panel(codebooks, m, dsub, ksub, ivfpq_panel);
  __syncthreads();
  if (c >= ksub) return;
  const float *y = ivfpq_panel + c * (dsub | 1u);
  const uint32_t q0 = blockIdx.y * kIvfPqTermGroup;
  for (uint32_t q = q0; q < q0 + kIvfPqTermGroup && q < Qc; q++)
    qterms[((size_t)q * M + m) * 256 + c] = ivfpq_dot(queries + ((size_t)q * M + m) * dsub, y, dsub);
}

__device__ __forceinline__ void ivfpq_put_entry(float *p, float d) { *p = d; }
__device__ __forceinline__ void ivfpq_put_entry(uint16_t *p, float d) { *p = __half_as_ushort(__float2half_rn(d)); }

// pq_tables' entries in ivfpq_query_terms' grid, panel and layout: every column to 255 is written, +inf from ksub on
template <typename E>
__global__ __launch_bounds__(kPqThreads) void ivfpq_query_tables_kernel(const float *__restrict__ queries, uint32_t Qc,
                                                                        const float *__restrict__ codebooks,
                                                                        uint32_t M, uint32_t dsub, uint32_t ksub,
                                                                        E *__restrict__ qtables) {
  extern __shared__ float ivfpq_panel[];   // ksub x (dsub | 1)
  const uint32_t m = blockIdx.x, c = threadIdx.x;
  ivfpq_stage_panel(codebooks, m, dsub, ksub, ivfpq_panel);
  __syncthreads();
  const float *y = ivfpq_panel + (c < ksub ? c : 0u) * (dsub | 1u);
  const uint32_t q0 = blockIdx.y * kIvfPqTermGroup;
  for (uint32_t q = q0; q < q0 + kIvfPqTermGroup && q < Qc; q++) {
    const float *x = queries + ((size_t)q * M + m) * dsub;
    float d = INFINITY;
    if (c < ksub)
      for (uint32_t j = 0; j < dsub; j++) ivfpq_term(d, x[j], y[j], j == 0);
    ivfpq_put_entry(qtables + ((size_t)q * M + m) * 256 + c, d);
  }
}

// norms[i] = sum_{j < D} fl(fl(x_j - g_j)^2) of live pair i = query * nprobe + rank, one chain in ascending j
__global__ __launch_bounds__(kPqThreads) void ivfpq_pair_norms_kernel(const float *__restrict__ queries,
                                                                      const float *__restrict__ centroids,
                                                                      const uint32_t *__restrict__ probes, uint32_t P,
                                                                      uint32_t nprobe, uint32_t K, uint32_t D,
                                                                      float *__restrict__ norms) {
  const uint64_t i = (uint64_t)blockIdx.x * kPqThreads + threadIdx.x;
  if (i >= P) return;
  const uint32_t c = ivfpq_pair_cluster(probes, (uint32_t)i, nprobe, K);
  if (c >= K) return;   // a dead pair is in no tile: its norm is never read
  const float *x = queries + (size_t)(i / nprobe) * D, *g = centroids + (size_t)c * D;
  float acc = 0.0f;
  if ((D & 3u) == 0 && ((reinterpret_cast<uintptr_t>(queries) | reinterpret_cast<uintptr_t>(centroids)) & 15u) == 0) {
    for (uint32_t j = 0; j < D; j += 4) {
      const float4 xx = *reinterpret_cast<const float4 *>(x + j), gg = *reinterpret_cast<const float4 *>(g + j);
      ivfpq_term(acc, xx.x, gg.x, j == 0);
      ivfpq_term(acc, xx.y, gg.y, false);
      ivfpq_term(acc, xx.z, gg.z, false);
      ivfpq_term(acc, xx.w, gg.w, false);
    }
  } else {
    for (uint32_t j = 0; j < D; j++) ivfpq_term(acc, x[j], g[j], j == 0);
  }
  norms[i] = acc;
}

template <int QT>
hipError_t ivfpq_scan_pre_launch(const IvfPqGeom &g, bool vec, const float *terms, const float *qterms,
                                 const float *norms, uint32_t tiles, const uint32_t *pair_start,
                                 const uint32_t *tile_start, const uint32_t *pairs, uint64_t *part, hipStream_t st) {
  const size_t lds = pq_scan_lds_bytes(g.M, g.k, QT);
  return with_flag(vec && QT <= 4, [&](auto V16) {
    using V = std::integral_constant<bool, decltype(V16)::value && QT <= 4>;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ivfpq_scan_pre_kernel<QT, V::value>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((ivfpq_scan_pre_kernel<QT, V::value>), dim3(tiles * g.S), dim3(kPqThreads), lds, st, g, terms,
                       qterms, norms, pair_start, tile_start, pairs, part);
    return hipGetLastError();
  });
}

template <int QT>
hipError_t ivfpq_scan_nonres_launch(const IvfPqGeom &g, bool vec, const float *qtables, uint32_t tiles,
                                  const uint32_t *pair_start, const uint32_t *tile_start, const uint32_t *pairs,
                                  uint64_t *part, hipStream_t st) {
  const size_t lds = pq_scan_lds_bytes(g.M, g.k, QT);
  return with_flag(vec && QT <= 4, [&](auto V16) {
    using V = std::integral_constant<bool, decltype(V16)::value && QT <= 4>;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ivfpq_scan_nonres_kernel<QT, V::value>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((ivfpq_scan_nonres_kernel<QT, V::value>), dim3(tiles * g.S), dim3(kPqThreads), lds, st, g, qtables,
                       pair_start, tile_start, pairs, part);
    return hipGetLastError();
  });
}

template <int QT>
hipError_t ivfpq_scan_launch(const IvfPqGeom &g, bool vec, const float *queries, uint32_t tiles,
                             const uint32_t *pair_start, const uint32_t *tile_start, const uint32_t *pairs,
                             uint64_t *part, hipStream_t st) {
  const size_t lds = ivfpq_scan_lds_bytes(g.M, g.k, QT);
  // M a multiple of 16 has a tile of at most 4: the larger tiles have no 16-byte variant
  return with_flag(vec && QT <= 4, [&](auto V16) {
    using V = std::integral_constant<bool, decltype(V16)::value && QT <= 4>;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ivfpq_scan_kernel<QT, V::value>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((ivfpq_scan_kernel<QT, V::value>), dim3(tiles * g.S), dim3(kPqThreads), lds, st, g, queries,
                       pair_start, tile_start, pairs, part);
    return hipGetLastError();
  });
}

}  // namespace

size_t ivfpq_scan_lds_bytes(uint32_t M, uint32_t k, uint32_t QT) {
  return pq_scan_lds_bytes(M, k, QT) + (size_t)QT * kIvfPqStage * sizeof(float);
}

uint32_t ivfpq_query_tile(uint32_t M, uint32_t k) {
  if (M == 0 || M > 64 || k == 0 || k > 256) return 0;
  for (uint32_t qt : {16u, 8u, 4u})   // two blocks per CU
    if (ivfpq_scan_lds_bytes(M, k, qt) <= kPqLdsPerCu / 2) return qt;
  for (uint32_t qt : {4u, 2u})        // one
    if (ivfpq_scan_lds_bytes(M, k, qt) <= kPqLdsPerCu) return qt;
  return 0;
}

uint32_t ivfpq_row_split(uint64_t pairs, uint32_t QT, uint64_t L) {
  if (pairs == 0 || QT == 0 || L == 0) return 0;
  const uint64_t tiles = (pairs + QT - 1) / QT, steps = (L + kPqThreads - 1) / kPqThreads;
  if (tiles >= kIvfPqBlocks) return 1;
  const uint64_t want = (kIvfPqBlocks + tiles - 1) / tiles;
  return (uint32_t)(want < steps ? want : steps);
}

hipError_t launch_ivfpq_group(const uint32_t *probes, uint32_t P, uint32_t nprobe, uint32_t K, uint32_t QT,
                              uint32_t *hist, uint32_t *pair_start, uint32_t *tile_start, uint32_t *cursor,
                              uint32_t *pairs, hipStream_t st) {
  const uint32_t blocks = (uint32_t)(((uint64_t)P + kPqThreads - 1) / kPqThreads);
  hipError_t e = launch_batched_fill(hist, K, 0u, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ivfpq_count_kernel, dim3(blocks), dim3(kPqThreads), 0, st, probes, P, nprobe, K, hist);
  hipLaunchKernelGGL(ivfpq_prefix_kernel, dim3(1), dim3(kPqThreads), 0, st, hist, K, QT, pair_start, tile_start,
                     cursor);
  hipLaunchKernelGGL(ivfpq_scatter_kernel, dim3(blocks), dim3(kPqThreads), 0, st, probes, P, nprobe, K, cursor, pairs);
  return hipGetLastError();
}

hipError_t launch_ivfpq_scan(const IvfPqGeom &g, const float *queries, uint32_t tiles, const uint32_t *pair_start,
                             const uint32_t *tile_start, const uint32_t *pairs, uint64_t *part, hipStream_t st) {
  const bool vec = (g.M & 15u) == 0 && (((uintptr_t)g.codes) & 15u) == 0;
  switch (g.QT) {
    case 2: return ivfpq_scan_launch<2>(g, vec, queries, tiles, pair_start, tile_start, pairs, part, st);
    case 4: return ivfpq_scan_launch<4>(g, vec, queries, tiles, pair_start, tile_start, pairs, part, st);
    case 8: return ivfpq_scan_launch<8>(g, vec, queries, tiles, pair_start, tile_start, pairs, part, st);
    case 16: return ivfpq_scan_launch<16>(g, vec, queries, tiles, pair_start, tile_start, pairs, part, st);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_ivfpq_terms(const float *centroids, const float *codebooks, uint32_t K, uint32_t M, uint32_t dsub,
                              uint32_t ksub, float *terms, hipStream_t st) {
  const size_t lds = ((size_t)ksub * (dsub | 1u) + (size_t)kIvfPqTermGroup * dsub) * sizeof(float);
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ivfpq_terms_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  const uint32_t groups = (uint32_t)(((uint64_t)K + kIvfPqTermGroup - 1) / kIvfPqTermGroup);
  hipLaunchKernelGGL(ivfpq_terms_kernel, dim3(M, groups < 65535 ? groups : 65535), dim3(kPqThreads), lds, st,
                     centroids, codebooks, K, M, dsub, ksub, terms);
  return hipGetLastError();
}

hipError_t launch_ivfpq_query_terms(const float *queries, uint32_t Qc, const float *codebooks, uint32_t M,
                                    uint32_t dsub, uint32_t ksub, float *qterms, hipStream_t st) {
  const size_t lds = (size_t)ksub * (dsub | 1u) * sizeof(float);
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ivfpq_query_terms_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ivfpq_query_terms_kernel, dim3(M, (Qc + kIvfPqTermGroup - 1) / kIvfPqTermGroup),
                     dim3(kPqThreads), lds, st, queries, Qc, codebooks, M, dsub, ksub, qterms);
  return hipGetLastError();
}

hipError_t launch_ivfpq_pair_norms(const float *queries, const float *centroids, const uint32_t *probes, uint32_t P,
                                   uint32_t nprobe, uint32_t K, uint32_t D, float *norms, hipStream_t st) {
  const uint32_t blocks = (uint32_t)(((uint64_t)P + kPqThreads - 1) / kPqThreads);
  hipLaunchKernelGGL(ivfpq_pair_norms_kernel, dim3(blocks), dim3(kPqThreads), 0, st, queries, centroids, probes, P,
                     nprobe, K, D, norms);
  return hipGetLastError();
}

hipError_t launch_ivfpq_scan_pre(const IvfPqGeom &g, const float *terms, const float *qterms, const float *norms,
                                 uint32_t tiles, const uint32_t *pair_start, const uint32_t *tile_start,
                                 const uint32_t *pairs, uint64_t *part, hipStream_t st) {
  const bool vec = (g.M & 15u) == 0 && (((uintptr_t)g.codes) & 15u) == 0;
  auto launch = [&](auto qt) {
    return ivfpq_scan_pre_launch<decltype(qt)::value>(g, vec, terms, qterms, norms, tiles, pair_start, tile_start,
                                                      pairs, part, st);
  };
  switch (g.QT) {
    case 2: return launch(std::integral_constant<int, 2>());
    case 4: return launch(std::integral_constant<int, 4>());
    case 8: return launch(std::integral_constant<int, 8>());
    case 16: return launch(std::integral_constant<int, 16>());
  }
  return hipErrorInvalidValue;
}

template <typename E>
hipError_t ivfpq_query_tables_launch(const float *queries, uint32_t Qc, const float *codebooks, uint32_t M,
                                     uint32_t dsub, uint32_t ksub, E *qtables, hipStream_t st) {
  const size_t lds = (size_t)ksub * (dsub | 1u) * sizeof(float);
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ivfpq_query_tables_kernel<E>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ivfpq_query_tables_kernel<E>, dim3(M, (Qc + kIvfPqTermGroup - 1) / kIvfPqTermGroup),
                     dim3(kPqThreads), lds, st, queries, Qc, codebooks, M, dsub, ksub, qtables);
  return hipGetLastError();
}

hipError_t launch_ivfpq_query_tables(const float *queries, uint32_t Qc, const float *codebooks, uint32_t M,
                                     uint32_t dsub, uint32_t ksub, float *qtables, hipStream_t st) {
  return ivfpq_query_tables_launch(queries, Qc, codebooks, M, dsub, ksub, qtables, st);
}

hipError_t launch_ivfpq_query_tables_f16(const float *queries, uint32_t Qc, const float *codebooks, uint32_t M,
                                         uint32_t dsub, uint32_t ksub, uint16_t *qtables, hipStream_t st) {
  return ivfpq_query_tables_launch(queries, Qc, codebooks, M, dsub, ksub, qtables, st);
}

hipError_t launch_ivfpq_scan_nonres(const IvfPqGeom &g, const float *qtables, uint32_t tiles, const uint32_t *pair_start,
                                  const uint32_t *tile_start, const uint32_t *pairs, uint64_t *part, hipStream_t st) {
  const bool vec = (g.M & 15u) == 0 && (((uintptr_t)g.codes) & 15u) == 0;
  auto launch = [&](auto qt) {
    return ivfpq_scan_nonres_launch<decltype(qt)::value>(g, vec, qtables, tiles, pair_start, tile_start, pairs, part, st);
  };
  switch (g.QT) {
    case 2: return launch(std::integral_constant<int, 2>());
    case 4: return launch(std::integral_constant<int, 4>());
    case 8: return launch(std::integral_constant<int, 8>());
    case 16: return launch(std::integral_constant<int, 16>());
  }
  return hipErrorInvalidValue;
}

hipError_t launch_ivfpq_residuals(const float *x, const float *centroids, const uint32_t *a, uint64_t N, uint32_t D,
                                  uint32_t K, float *out, hipStream_t st) {
  const uint64_t blocks = (N * D + kPqThreads - 1) / kPqThreads;
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(ivfpq_residuals_kernel, dim3((uint32_t)(blocks < 65536 ? blocks : 65536)), dim3(kPqThreads), 0, st,
                     x, centroids, a, N, D, K, out);
  return hipGetLastError();
}

}  // namespace kmx
