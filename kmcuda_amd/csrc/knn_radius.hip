// knn_radius.hip -- radius search of a query batch against the k-NN index's corpus (kmamd_knn_index_radius_count /
// _fill): every corpus row of a cluster whose exact distance to the query is <= r.
//
// The result is the brute-force set over the clustered rows, in ascending (cluster id, corpus row) order -- the order
// of the cluster-sorted copy.  Two kernels, each in a counting (FILL = false) and a filling (FILL = true) form:
//   knn_radius_f16_kernel    the query mode of knn_f16.hip's filter (same block plan, tile ring, swizzle, operand sets
//                            and error term E) under a threshold that never moves: no heaps, amin evaluated once per
//                            query, the cluster prune known before a tile is issued.  Survivors of the matrix-core
//                            filter go through the reference's exact chain (exact_split.hpp) four at a time (two at 256 features) and are
//                            hits iff distance <= r.
//   knn_radius_exact_kernel  one thread per query, every member of every unpruned cluster with the exact arithmetic
//                            (D > 1024, KMCUDA_AMD_KNN_EXACT, KMCUDA_AMD_FP16_STRICT, KMCUDA_AMD_FILTER=f32, a corpus
//                            or chunk that leaves the half range).
// A query is owned by one lane that meets its candidates in ascending sorted position, so its hits are stored in that
// order at a cursor that starts at offsets[query] and never passes offsets[query + 1]: the writes go to their final
// CSR place.  A query whose hit count differs from its range raises KnnRadiusArgs::flag.
//
// Cluster prune (never the reference's bare triangle test, which has no margin for the rounding of its terms):
//   lb[c][q] > r                                       with the table of knn_centroid_bounds_kernel (KnnArgs::lb), else
//   C[c][c_q] - d(q, c_q) - R[c] - margin > r          margin = prune_abs + prune_rel * (C + d + R), from the host;
//   prune_abs = inf: no cluster is pruned (the half2 arithmetic).  A NaN term compares false: the cluster is visited.
//
// MASK (kmamd_knn_index_radius_count_allow / _fill_allow): a candidate whose bit of KnnArgs::allow_bits
// is clear is no hit; KnnArgs::R holds the radii over the allowed rows, and a cluster without one (allow_count, R = NaN:
// no prune test speaks) is walked over like one without rows.  The f16 kernel takes a sub-tile's 32 bits from two words
// (the same for every lane) and ANDs them into the row mask; a sub-tile whose bits are all clear is not scored at all.
// The bits from the cluster's end on (the next cluster's rows, the padding) do not count.  wait_tiles counts a wave's
// DMAs per tile, so every wave issues for every tile exactly the pieces the unmasked kernel issues, in their order,
// whatever it skips: the MASK kernels issue a sub-tile's pieces in front of its k-steps, not between them.
#include <hip/hip_fp16.h>
#include <stdlib.h>

#include "exact.hpp"
#include "exact_split.hpp"
#include "half2_ops.hpp"
#include "kernels.hpp"

namespace kmx {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// hand-issued LDS reads with counted waits, as knn_f16.hip's (copies: that file's code generation stays untouched)
__device__ __forceinline__ f16x8 rad_frag_issue(uint32_t addr) {
  f16x8 f;
  asm volatile("ds_read_b128 %0, %1" : "=v"(f) : "v"(addr) : "memory");
  return f;
}
__device__ __forceinline__ f32x4 rad_lds_read4(uint32_t addr) {
  f32x4 f;
  asm volatile("ds_read_b128 %0, %1" : "=v"(f) : "v"(addr) : "memory");
  return f;
}
template <int N>
__device__ __forceinline__ void rad_frag_wait(f16x8 &f) {
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(f) : "n"(N));
}

// largest c with offsets[c] <= p, c in [0, K]; K means "no cluster" (knn.hip: cluster_of)
__device__ __forceinline__ uint32_t rad_cluster_of(const uint32_t *__restrict__ offsets, uint32_t K, uint32_t p) {
  uint32_t lo = 0, hi = K + 1;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (offsets[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

// the reference's candidate distance (knn.hip: partial_vv + finalize, metric_abstraction.h:103-136)
template <int METRIC>
__device__ __forceinline__ float rad_distance(const float *__restrict__ a, const float *__restrict__ b, uint32_t n) {
  float acc = 0.f, corr = 0.f;
  for (uint32_t f = 0; f < n; f++) {
    if (METRIC == 0) {
      const float d = a[f] - b[f];
      kahan_fold(fma_rd(d, d, corr), acc, corr);
    } else {
      kahan_fold(fma_rd(a[f], b[f], corr), acc, corr);
    }
  }
  return METRIC == 0 ? sqrtf(acc) : angular_from_prod(acc);
}

// v[i] without a runtime-indexed array, which would live in scratch (written as nested selects: the compiler turns a
// select loop back into an indexed load)
template <typename T>
__device__ __forceinline__ T rad_sel(const T (&v)[4], int i) {
  return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3]));
}
template <typename T>
__device__ __forceinline__ T rad_sel(const T (&v)[2], int i) {
  return i == 0 ? v[0] : v[1];
}

// true if every member of cluster `cls` is farther than r from a query of cluster `mine` (see the head of the file)
__device__ __forceinline__ bool rad_triangle_prunes(const KnnRadiusArgs &ra, uint32_t cls, uint32_t mine, float md) {
  const float cd = ra.a.C[(size_t)cls * ra.a.K + mine], rr = ra.a.R[cls];
  const float lim = cd - md - rr - (ra.prune_abs + ra.prune_rel * (cd + md + rr));
  return lim > ra.radius;
}

}  // namespace

template <int DP, int METRIC, bool FASTX, bool FILL, bool MASK = false>
__global__ __launch_bounds__(knn16_waves(DP) * 64, knn16_blocks_per_cu(DP)) void knn_radius_f16_kernel(KnnRadiusArgs ra) {
  const KnnArgs &a = ra.a;
  constexpr int WV = knn16_waves(DP), NSET = knn16_nset(DP);
  constexpr int NKH = DP / 2;   // features per half-wave
  constexpr int KS = NKH / 8;   // k-steps = 16-byte chunks per half row
  constexpr int ROWB = DP * 2;  // bytes of one candidate row (DP halves)
  constexpr int SUB = knn16_sub(DP);        // 32-candidate sub-tiles per staged tile (= per barrier)
  constexpr int TILEB = 32 * SUB * ROWB;
  constexpr int NP = (TILEB + 1023) / 1024;   // 1-KB LDS-DMA pieces per tile
  constexpr int SWM = (KS < 16 ? KS : 16) - 1;
  constexpr int NBUF = knn16_nbuf(DP);        // ring of tile buffers: NBUF - 1 tiles in flight
  // survivors queued per query = exact chains run at once.  Two operand sets of 256 features are 256 registers' worth
  // of operands: two chains there (exact_distance_w's two-chain body), four everywhere else
  constexpr int QD = (NSET == 2 && DP >= 256) ? 2 : 4;
  typedef __attribute__((address_space(3))) unsigned char lds_byte;
  extern __shared__ __attribute__((aligned(1024))) unsigned char lds2[];
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_byte *)lds2;
  constexpr uint32_t TILES = (uint32_t)(NBUF * TILEB);
  const uint32_t bias0 = lds0 + TILES;                       // NBUF x 64 floats
  uint32_t *flags = reinterpret_cast<uint32_t *>(lds2 + TILES + NBUF * 256);  // 2 x WV words

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), col = lane & 31, h = lane >> 5;
  const uint32_t K = a.K, D = a.D;
  const float r = ra.radius;

  const uint32_t cls0 = a.blocks[2 * (size_t)blockIdx.x], p0 = a.blocks[2 * (size_t)blockIdx.x + 1];
  const uint32_t own_end = a.qoffsets[cls0 + 1];
  uint32_t qp[NSET];
  bool live[NSET];
  // B operands: my half of my queries' rows (centred halves)
  f16x8 xhi[NSET][KS];
  float amin[NSET];
  // hits so far.  FILL: hit number i goes to offsets[query] + i while that is below offsets[query + 1]; the two are
  // read when a hit is stored (few candidates are hits; the registers are the operands')
  uint32_t hits[NSET];
  const float nmax2 = __uint_as_float(a.stats[0]);
  const float u = 5.9604645e-8f;
  const float nmx = sqrtf(nmax2) * 1.0001f;
#pragma unroll
  for (int e = 0; e < NSET; e++) {
    qp[e] = p0 + (uint32_t)wave * (32u * NSET) + 32u * e + col;   // my slot of the block plan ...
    live[e] = qp[e] < own_end;
    if (a.qperm && live[e]) qp[e] = a.qperm[qp[e] - a.p_base];     // ... and the query of this cluster it stands for
    const uint32_t qq = live[e] ? qp[e] : p0;
    const _Float16 *src = reinterpret_cast<const _Float16 *>(a.qxs16) + (size_t)qq * DP + h * NKH;
#pragma unroll
    for (int j = 0; j < KS; j++) {
      xhi[e][j] = reinterpret_cast<const f16x8 *>(src)[j];
      if (!live[e]) {
#pragma unroll
        for (int q = 0; q < 8; q++) xhi[e][j][q] = (_Float16)0.f;
      }
    }
    const float qn2 = live[e] ? a.qn2s[qp[e]] : 0.f;      // centred squared norm
    hits[e] = 0;
    // a candidate can only be within r in the reference's arithmetic if acc >= amin: the
    // bound of knn_f16.hip with the kth distance replaced by r, evaluated once
    const float qn = sqrtf(qn2) * 1.0001f;
    const float e_round = 9.78e-4f * qn * nmx;   // operand rounding of the hi.hi-only score
    if (METRIC == 0) {
      const float E = 4.04f * (3.0f * a.eps + 16.0f * u) * (qn2 + nmax2) + 6e-8f * sqrtf((float)DP) * (qn + nmx) + 2.0f * e_round;
      const float T2 = r * r * 1.000001f;   // (inf for a huge radius: every finite score passes)
      amin[e] = 0.5f * (qn2 - T2 - E) - 1e-6f * (qn2 + T2);
    } else {
      const float mun = sqrtf(a.mu2) * 1.0001f;
      const float kq = (live[e] ? a.qmux[qp[e]] : 0.f) + a.mu2;      // x.y = acc + mu.x' + ||mu||^2
      const float E = 2.02f * (3.0f * a.eps + 16.0f * u) * (qn * nmx + mun * nmx) + 3e-8f * sqrtf((float)DP) * (qn + nmx) +
                      a.eps * (mun * qn + a.mu2) + 1e-6f + e_round;
      amin[e] = r >= 3.1415925f ? -INFINITY : cosf(r) - kq - E;
    }
  }

  // The candidate tiles: knn_f16.hip's LDS-DMA ring.  Linear byte P of a tile lands in LDS at P and is fetched from
  // source byte P ^ (((P / ROWB) & SWM) << 4); the biases of the tile are one 4-byte DMA by wave 0.
  const int my_dma = (NP > wave ? (NP - wave + WV - 1) / WV : 0) + (wave == 0 ? 1 : 0);   // DMAs I issue per tile
  constexpr int PPW = (NP + WV - 1) / WV;   // pieces per wave and tile (waves >= NP % WV may have one less)
  auto issue_piece = [&](uint32_t tile_base, int buf, int i) {
    if (i == PPW) {
      if (wave == 0)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(a.kbias + tile_base + lane),
                                         (__attribute__((address_space(3))) void *)(uintptr_t)(bias0 + buf * 256), 4, 0, 0);
      return;
    }
    const int p = wave + WV * i;
    if (p >= NP) return;   // wave-uniform
    const unsigned char *src = reinterpret_cast<const unsigned char *>(a.xs16) + (size_t)tile_base * ROWB;
    uint32_t P0 = (uint32_t)lane * 16u;
    asm volatile("" : "+v"(P0));
    const uint32_t P = (uint32_t)p * 1024u + P0;
    const uint32_t from = P ^ (((P / ROWB) & SWM) << 4);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + from),
                                     (__attribute__((address_space(3))) void *)(uintptr_t)(lds0 + buf * TILEB + p * 1024), 16, 0, 0);
  };
  auto issue_tile = [&](uint32_t tile_base, int buf) {
#pragma unroll
    for (int i = 0; i <= PPW; i++) issue_piece(tile_base, buf, i);
  };
  auto wait_tiles = [&](bool steady) {
#define KMX_VM_CASE(v) case v: asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NBUF - 2) * v) : "memory"); break
    switch (steady && NBUF > 2 ? my_dma : 0) {
      KMX_VM_CASE(1); KMX_VM_CASE(2); KMX_VM_CASE(3); KMX_VM_CASE(4); KMX_VM_CASE(5);
      KMX_VM_CASE(6); KMX_VM_CASE(7); KMX_VM_CASE(8); KMX_VM_CASE(9);
      default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
#undef KMX_VM_CASE
  };
  static_assert(NBUF == 2 || (PPW + 1 <= 9 && (NBUF - 2) * 9 < 64), "wait_tiles: DMAs per wave and tile");
  static_assert(SUB == 1 || SUB == 2, "one 64-lane bias DMA per tile");
  static_assert(NBUF >= 2, "ring");
  const uint32_t fragbase = lds0 + (uint32_t)col * ROWB + (uint32_t)h * (KS * 16);
  const uint32_t fragswz = (uint32_t)(col & SWM) * 16u;

  // queues of survivors (sorted positions, ascending), one per operand set
  uint32_t qc[NSET][QD];
  int qn_[NSET];
#pragma unroll
  for (int e = 0; e < NSET; e++) {
    qn_[e] = 0;
#pragma unroll
    for (int i = 0; i < QD; i++) qc[e][i] = 0;
  }
  uint32_t chains = 0;   // exact chains this lane's queries have paid for (statistics)
  auto flush = [&](int e) {  // wave-uniform call
    const uint32_t qq = live[e] ? qp[e] : p0;
    const float *xrow = a.qxs + (size_t)qq * DP;   // original values (exact chains)
    const float *crow[4];
#pragma unroll
    for (int i = 0; i < 4; i++) crow[i] = a.xs + (size_t)(i < QD && i < qn_[e] ? qc[e][i < QD ? i : 0] : 0) * DP;
    float dist[4];
    int nq = 1;   // the fullest queue of the wave
#pragma unroll
    for (int i = 2; i <= QD; i++) nq = __ballot(qn_[e] >= i) ? i : nq;
    chains += h == 0 ? (uint32_t)qn_[e] : 0u;
    // (always the QD-chain body: a queue is settled when some lane's is full, so nq is QD but for a query's last
    //  flush, and one call site keeps dist[] in registers)
    exact_distance_w<NKH, METRIC, FASTX, false, QD>(xrow, crow, D, h, col, dist, nq, qn_[e]);
    uint32_t hm = 0;   // which of the queued candidates are hits (a NaN distance is none)
#pragma unroll
    for (int i = 0; i < QD; i++) hm |= (h == 0 && i < qn_[e] && dist[i] <= r ? 1u : 0u) << i;
    if (FILL && hm) {
      // in queue order = ascending sorted position; a rolled loop (few candidates are hits: small code, few registers)
      const uint32_t qi = ra.qinv[qq];
      const unsigned long long first = ra.offsets[qi], last = ra.offsets[qi + 1];
#pragma unroll 1
      for (uint32_t m = hm, n = hits[e]; m; m &= m - 1u, n++) {
        const int i = __ffs((int)m) - 1;
        const unsigned long long at = first + n;
        if (at < last) {
          ra.neighbors[at - ra.out_base] = a.inv[rad_sel(qc[e], i)];
          if (ra.distances) ra.distances[at - ra.out_base] = rad_sel(dist, i);
        }
      }
    }
    hits[e] += (uint32_t)__popc(hm);
    qn_[e] = 0;
  };

  unsigned long long calced = 0, useful = 0;   // wave-uniform (scalar registers)
  uint32_t scored = 0, scored_sets = 0;        // in sub-tiles of 32 x 32 scores (at most N / 32 per operand set: 32 bits)
  int ph = 0;
  for (uint32_t cls = 0; cls < K; cls++) {   // ascending cluster id: the order of the output
    const uint32_t beg = a.offsets[cls], end = a.offsets[cls + 1];
    if (beg == end) continue;                     // nothing to visit (block-uniform)
    if constexpr (MASK) {
      if (a.allow_count[cls] == 0u) continue;     // no row of it may be returned (block-uniform)
    }
    bool pruned[NSET];
#pragma unroll
    for (int e = 0; e < NSET; e++) {
      pruned[e] = !live[e];
      if (!pruned[e])
        pruned[e] = a.lb ? a.lb[(size_t)cls * a.lb_stride + (qp[e] - a.p_base)] > r
                         : rad_triangle_prunes(ra, cls, cls0, a.qmydist[qp[e]]);   // (read per cluster: no register held for it)
    }
    unsigned long long visiting = 0;
    uint32_t nvisit = 0, nsets_live = 0;   // queries / operand sets of the wave that visit the cluster
    bool set_live[NSET];
#pragma unroll
    for (int e = 0; e < NSET; e++) {
      const unsigned long long b = __ballot(!pruned[e]);
      visiting |= b;
      nvisit += (uint32_t)__popcll(b & 0xFFFFFFFFull);
      set_live[e] = b != 0ull;
      nsets_live += b ? 1u : 0u;
    }
    calced += (unsigned long long)nvisit * (end - beg);
    const bool wave_need = visiting != 0ull;
    if (lane == 0) flags[ph * WV + wave] = wave_need ? 1u : 0u;
    __syncthreads();
    uint32_t any_need = 0;
#pragma unroll
    for (int w = 0; w < WV; w++) any_need |= flags[ph * WV + w];
    const bool need = any_need != 0u;
    ph ^= 1;
    if (!need) continue;

    const uint32_t ntiles = (end - beg + 32 * SUB - 1) / (32 * SUB);
    // (the barrier above ordered every wave's reads of the previous cluster's tiles before these writes)
#pragma unroll
    for (int i = 0; i < NBUF - 1; i++)
      if ((uint32_t)i < ntiles) issue_tile(beg + 32u * SUB * i, i);
    f32x16 acc[NSET];
    constexpr int DSTR = (SUB * KS) / (PPW + 1) > 0 ? (SUB * KS) / (PPW + 1) : 1;
    // scores of one sub-tile: the biases seed the accumulators, KS k-steps on hand-issued fragment reads, every
    // fragment feeding the operand sets that have a visiting query
    auto mfma_tile = [&](int buf, int sub, bool dma, uint32_t dma_base, int dma_buf) {
      const uint32_t tb = fragbase + (uint32_t)buf * TILEB + (uint32_t)sub * (32 * ROWB);
      const uint32_t bb = bias0 + (uint32_t)buf * 256u + (uint32_t)sub * 128u + 16u * h;
      f32x4 b4[4];
#pragma unroll
      for (int g = 0; g < 4; g++) b4[g] = rad_lds_read4(bb + 32u * g);
      constexpr int PD = KS < KNN16_PD ? KS : KNN16_PD;   // fragments in flight
      f16x8 fr[PD + 1];
#pragma unroll
      for (int j = 0; j < PD; j++) fr[j] = rad_frag_issue(tb + ((16u * j) ^ fragswz));
      asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(b4[0]), "+v"(b4[1]), "+v"(b4[2]), "+v"(b4[3]) : "n"(PD));
#pragma unroll
      for (int e = 0; e < NSET; e++) {
#pragma unroll
        for (int g = 0; g < 4; g++) {
          acc[e][4 * g + 0] = b4[g].x; acc[e][4 * g + 1] = b4[g].y; acc[e][4 * g + 2] = b4[g].z; acc[e][4 * g + 3] = b4[g].w;
        }
      }
#pragma unroll
      for (int j = 0; j < KS; j++) {
        if (j + PD < KS) fr[(j + PD) % (PD + 1)] = rad_frag_issue(tb + ((16u * (j + PD)) ^ fragswz));
        const int behind = (KS - 1 - j) < PD ? (KS - 1 - j) : PD;
        f16x8 &f = fr[j % (PD + 1)];
        if (behind == 4) rad_frag_wait<4>(f);
        else if (behind == 3) rad_frag_wait<3>(f);
        else if (behind == 2) rad_frag_wait<2>(f);
        else if (behind == 1) rad_frag_wait<1>(f);
        else rad_frag_wait<0>(f);
#pragma unroll
        for (int e = 0; e < NSET; e++)
          if (NSET == 1 || set_live[e]) acc[e] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f, xhi[e][j], acc[e], 0, 0, 0);
        {
          const int slot = sub * KS + j;   // compile-time after unrolling
          if (dma && slot % DSTR == 0 && slot / DSTR <= PPW) issue_piece(dma_base, dma_buf, slot / DSTR);
        }
      }
    };
    // which of the sub-tile's 32 candidates can be within r of which query of set e (bit i: row i of the sub-tile).
    // Both sets' masks are taken before either is drained: no accumulator is live across a flush's exact chains.
    auto score_mask = [&](int e) -> uint32_t {
      uint32_t m16 = 0;
      // the tile's best score first: most tiles hold no candidate for any query of the wave (NaN scores never pass)
      bool some = false;
      if (!pruned[e]) {
        const f32x16 &c = acc[e];
        const float m0 = __builtin_fmaxf(__builtin_fmaxf(c[0], c[1]), c[2]);
        const float m1 = __builtin_fmaxf(__builtin_fmaxf(c[3], c[4]), c[5]);
        const float m2 = __builtin_fmaxf(__builtin_fmaxf(c[6], c[7]), c[8]);
        const float m3 = __builtin_fmaxf(__builtin_fmaxf(c[9], c[10]), c[11]);
        const float m4 = __builtin_fmaxf(__builtin_fmaxf(c[12], c[13]), c[14]);
        const float m5 = __builtin_fmaxf(__builtin_fmaxf(m0, m1), c[15]);
        const float m6 = __builtin_fmaxf(__builtin_fmaxf(m2, m3), m4);
        some = __builtin_fmaxf(m5, m6) >= amin[e];
      }
      uint32_t rowmask = 0;
      if (__ballot(some) != 0ull) {
        if (some) {
#pragma unroll
          for (int rr = 0; rr < 16; rr++) m16 |= (acc[e][rr] >= amin[e] ? 1u : 0u) << rr;
        }
        const uint32_t pm = __shfl_xor(m16, 32);
        const uint32_t m0 = h ? pm : m16, m1 = h ? m16 : pm;
#pragma unroll
        for (int g = 0; g < 4; g++)
          rowmask |= (((m0 >> (4 * g)) & 0xFu) << (8 * g)) | (((m1 >> (4 * g)) & 0xFu) << (8 * g + 4));
      }
      return rowmask;
    };
    // queue them in ascending row order, settle full queues
    auto drain = [&](int e, uint32_t rowmask, uint32_t tile_base) {
      while (__ballot(rowmask != 0u) != 0ull) {
        if (__ballot(qn_[e] == QD) != 0ull) flush(e);
        bool active = rowmask != 0u;
        const uint32_t rho = active ? (uint32_t)__ffs((int)rowmask) - 1u : 0u;
        rowmask &= rowmask - 1u;
        const uint32_t cp = tile_base + rho;
        if (cp >= end) active = false;                 // tile padding: other clusters' rows, or the zero rows behind the corpus
        if (active) {
#pragma unroll
          for (int i = 0; i < QD; i++)
            if (i == qn_[e]) qc[e][i] = cp;
          qn_[e]++;
        }
      }
    };
    for (uint32_t t = 0; t < ntiles; t++) {
      const int buf = (int)(t % NBUF);
      const uint32_t tile_base = beg + t * (32 * SUB);
      {
        // tile t has landed (my pieces: counted wait; everybody's: the barrier), and every wave is done with
        // tile t - 1, whose buffer the tile NBUF - 1 ahead goes into
        const uint32_t ahead = ntiles - 1 - t;
        wait_tiles(ahead >= (uint32_t)(NBUF - 2));
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
      const bool dma = t + (NBUF - 1) < ntiles;
      const uint32_t dma_base = tile_base + 32u * SUB * (NBUF - 1);
      const int dma_buf = (int)((t + NBUF - 1) % NBUF);
      if (dma && !wave_need) issue_tile(dma_base, dma_buf);
      if (wave_need) {
#pragma unroll
        for (int sub = 0; sub < SUB; sub++) {
          // (a last tile of one sub-tile only has no tile NBUF - 1 ahead: no piece is lost by the break)
          if (sub > 0 && tile_base + 32u * sub >= end) break;   // block-uniform
          [[maybe_unused]] uint32_t allowed = 0;   // MASK: bit rho: may sorted position tile_base + 32 sub + rho be returned
          if constexpr (MASK) {
            // (the same for every lane, kept in a scalar register; the sub-tile starts below end <= N: the word behind
            //  it exists.  The bits from `end` on are the next cluster's, or the padding's: not this sub-tile's rows)
            const uint32_t sb = tile_base + 32u * sub, w = sb >> 5, sh = sb & 31u, left = end - sb;
            const unsigned long long two = ((unsigned long long)a.allow_bits[w + 1] << 32) | a.allow_bits[w];
            allowed = (uint32_t)(two >> sh) & (left < 32u ? (1u << left) - 1u : 0xFFFFFFFFu);
            allowed = (uint32_t)__builtin_amdgcn_readfirstlane((int)allowed);
            // The DMA pieces mfma_tile's k-steps of this sub-tile carry in the unmasked kernel -- piece slot / DSTR at slot
            // sub * KS + j where slot % DSTR == 0 and slot / DSTR <= PPW -- and, behind the last sub-tile, the remainder
            // up to PPW: consecutive pieces, issued HERE, in front of the decision, by every wave whatever it skips (the
            // buffer is tile t - 1's: free since the barrier above).  One copy of the address arithmetic for both ways
            // on: a second copy in a skip branch beside mfma_tile's cost 8 to 12 VGPRs and a wave per SIMD at DP 16 / 64.
            if (dma) {
              const int first = (sub * KS + DSTR - 1) / DSTR, last_slot = (sub * KS + KS - 1) / DSTR;
              const int last = sub == SUB - 1 || last_slot > PPW ? PPW : last_slot;
#pragma unroll
              for (int i = first; i <= last; i++) issue_piece(dma_base, dma_buf, i);
            }
            if (allowed == 0u) continue;   // block-uniform: no row of it can be a hit -- not scored, not counted as scored
          }
          mfma_tile(buf, sub, dma && !MASK, dma_base, dma_buf);
          {   // statistics (wave-uniform)
            scored += NSET == 1 ? 1u : nsets_live;
            scored_sets += nsets_live;
            const uint32_t left = end - (tile_base + 32u * sub);
            useful += (unsigned long long)nvisit * (left < 32u ? left : 32u);
          }
          if (sub == SUB - 1 && dma && !MASK) {   // pieces the slots did not cover (very short rows)
#pragma unroll
            for (int i = (SUB * KS - 1) / DSTR + 1; i <= PPW; i++) issue_piece(dma_base, dma_buf, i);
          }
          uint32_t rowmask[NSET];
#pragma unroll
          for (int e = 0; e < NSET; e++) rowmask[e] = score_mask(e);
          if constexpr (MASK) {
#pragma unroll
            for (int e = 0; e < NSET; e++) rowmask[e] &= allowed;
          }
#pragma unroll
          for (int e = 0; e < NSET; e++) drain(e, rowmask[e], tile_base + 32u * sub);
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < NSET; e++) {
    if (__ballot(qn_[e] > 0) != 0ull) flush(e);
    if (live[e] && h == 0) {
      const uint32_t qi = ra.qinv[qp[e]];
      if (FILL) {
        // fewer hits than the range, or more (none stored past it)
        if (ra.offsets[qi] + hits[e] != ra.offsets[qi + 1]) atomicOr(ra.flag, 1u);
      } else {
        ra.counts[qi] = hits[e];
      }
    }
  }
  if (lane == 0 && calced) atomicAdd(a.calced, calced);
  if (lane == 0 && scored) {
    atomicAdd(a.calced + 1, 1024ull * scored);
    atomicAdd(a.calced + 2, useful);
    atomicAdd(a.calced + 4, 1024ull * scored_sets);
  }
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) chains += __shfl_xor(chains, off);   // (the upper half-wave holds zeros)
  if (lane == 0 && chains) atomicAdd(a.calced + 3, (unsigned long long)chains);
}

// one thread per sorted query position of [p_base, p_end); a query without a cluster (a NaN or inf feature) has no hits
template <int METRIC, bool H2, bool FILL, bool MASK = false>
__global__ __launch_bounds__(64) void knn_radius_exact_kernel(KnnRadiusArgs ra) {
  const KnnArgs &a = ra.a;
  const uint32_t qp = a.p_base + blockIdx.x * blockDim.x + threadIdx.x;
  if (qp >= a.p_end) return;
  const uint32_t K = a.K, D = a.D, DP = a.DP;
  const float r = ra.radius;
  const uint32_t mycls = rad_cluster_of(a.qoffsets, K, qp);
  const uint32_t qi = ra.qinv[qp];
  unsigned long long cursor = 0, range_end = 0;
  if (FILL) {
    cursor = ra.offsets[qi];
    range_end = ra.offsets[qi + 1];
  }
  unsigned long long calced = 0;
  if (mycls < K) {
    const float *x = a.qxs + (size_t)qp * DP;
    const float md = a.qmydist[qp];
    for (uint32_t cls = 0; cls < K; cls++) {
      const uint32_t beg = a.offsets[cls], end = a.offsets[cls + 1];
      if (beg == end) continue;
      if constexpr (MASK) {
        if (a.allow_count[cls] == 0u) continue;   // no row of it may be returned
      }
      if (a.lb ? a.lb[(size_t)cls * a.lb_stride + (qp - a.p_base)] > r : rad_triangle_prunes(ra, cls, mycls, md)) continue;
      calced += end - beg;
      for (uint32_t cp = beg; cp < end; cp++) {
        if constexpr (MASK) {
          if (((a.allow_bits[cp >> 5] >> (cp & 31u)) & 1u) == 0u) continue;
        }
        const float dist = H2 ? h2_distance<METRIC>(x, a.xs + (size_t)cp * DP, D)   // distance_tt, F = half2
                              : rad_distance<METRIC>(x, a.xs + (size_t)cp * DP, D);
        if (dist <= r) {   // (a NaN distance is no hit)
          if (FILL) {
            if (cursor < range_end) {
              const unsigned long long at = cursor - ra.out_base;
              ra.neighbors[at] = a.inv[cp];
              if (ra.distances) ra.distances[at] = dist;
            }
          }
          cursor++;
        }
      }
    }
  }
  if (FILL) {
    if (cursor != range_end) atomicOr(ra.flag, 1u);
  } else {
    ra.counts[qi] = (uint32_t)cursor;
  }
  if (calced) atomicAdd(a.calced, calced);
}

// The queries the block plan of the f16 kernel does not cover (sorted positions [p_base, p_end): no cluster, no hits):
// count 0, or a range that must be empty
__global__ void knn_radius_rest_kernel(KnnRadiusArgs ra, bool fill) {
  const uint32_t qp = ra.a.p_base + blockIdx.x * blockDim.x + threadIdx.x;
  if (qp >= ra.a.p_end) return;
  const uint32_t qi = ra.qinv[qp];
  if (!fill) ra.counts[qi] = 0;
  else if (ra.offsets[qi] != ra.offsets[qi + 1]) atomicOr(ra.flag, 1u);
}

// flag |= 1 if offsets[0 .. n] decreases somewhere
__global__ void knn_radius_offsets_kernel(const unsigned long long *__restrict__ offsets, uint32_t n,
                                          uint32_t *__restrict__ flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && offsets[i] > offsets[i + 1]) atomicOr(flag, 1u);
}

template <int DP, int METRIC, bool FILL, bool MASK>
static hipError_t launch_knn_radius_f16_t(const KnnRadiusArgs &ra, uint32_t nblocks, hipStream_t st) {
  const size_t lds_bytes = (size_t)knn16_nbuf(DP) * (32 * knn16_sub(DP) * DP * 2) + knn16_nbuf(DP) * 256 + 2 * knn16_waves(DP) * 4;
  return with_flag(ra.a.D == (uint32_t)DP, [&](auto FAST) {
    if (lds_bytes > 65536) {   // (per launch: the attribute belongs to the current device's copy of the kernel)
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&knn_radius_f16_kernel<DP, METRIC, FAST(), FILL, MASK>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((knn_radius_f16_kernel<DP, METRIC, FAST(), FILL, MASK>), dim3(nblocks), dim3(knn16_waves(DP) * 64), lds_bytes, st, ra);
    return hipGetLastError();
  });
}

hipError_t launch_knn_radius_f16(int metric, const KnnRadiusArgs &ra, uint32_t nblocks, bool fill, hipStream_t st,
                                 bool mask) {
  if (mask && (!ra.a.allow_bits || !ra.a.allow_count)) return hipErrorInvalidValue;
  if (nblocks == 0) return hipSuccess;
  return with_width<KnnF16Widths>(ra.a.DP, [&](auto DP) {
    return with_metric(metric, [&](auto M) {
      return with_flag(fill, [&](auto FILL) {
        return with_flag(mask, [&](auto MASK) { return launch_knn_radius_f16_t<DP(), M(), FILL(), MASK()>(ra, nblocks, st); });
      });
    });
  });
}

hipError_t launch_knn_radius_exact(int metric, const KnnRadiusArgs &ra, bool strict_h2, bool fill, hipStream_t st,
                                   bool mask) {
  if (mask && (!ra.a.allow_bits || !ra.a.allow_count)) return hipErrorInvalidValue;
  if (ra.a.p_end <= ra.a.p_base) return hipSuccess;
  const dim3 grid((ra.a.p_end - ra.a.p_base + 63) / 64);
  return with_metric(metric, [&](auto M) {
    return with_flag(strict_h2, [&](auto H) {
      return with_flag(fill, [&](auto FILL) {
        return with_flag(mask, [&](auto MASK) {
          hipLaunchKernelGGL((knn_radius_exact_kernel<M(), H(), FILL(), MASK()>), grid, dim3(64), 0, st, ra);
          return hipGetLastError();
        });
      });
    });
  });
}

hipError_t launch_knn_radius_rest(const KnnRadiusArgs &ra, bool fill, hipStream_t st) {
  if (ra.a.p_end <= ra.a.p_base) return hipSuccess;
  hipLaunchKernelGGL(knn_radius_rest_kernel, dim3((ra.a.p_end - ra.a.p_base + 255) / 256), dim3(256), 0, st, ra, fill);
  return hipGetLastError();
}

hipError_t launch_knn_radius_offsets_check(const uint64_t *offsets, uint32_t n, uint32_t *flag, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(knn_radius_offsets_kernel, dim3((n + 255) / 256), dim3(256), 0, st,
                     reinterpret_cast<const unsigned long long *>(offsets), n, flag);
  return hipGetLastError();
}

}  // namespace kmx
