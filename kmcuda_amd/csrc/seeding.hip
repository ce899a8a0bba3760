// seeding.hip -- exact-arithmetic helper kernels around the hot path:
//   kmpp_step          (reference: kmeans.cu:42-67 kmeans_plus_plus): d[s] = min(d[s], dist(s, newest c))
//   member_distances   (reference: kmeans.cu:674-691 kmeans_calc_average_distance, per-sample part)
// Distances use the reference's exact arithmetic (exact.hpp) so that the host-side chooser sees
// the very same floats as the reference's and picks the same seeds.
#include <hip/hip_fp16.h>
#include <rocrand/rocrand_xorwow.h>

#include "exact.hpp"
#include "kernels.hpp"

namespace kmx {

template <int METRIC>
__global__ void kmpp_step_kernel(const float *__restrict__ samples, uint32_t N, uint32_t D,
                                 const float *__restrict__ centroid, uint32_t cc, float *__restrict__ dists) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= N) return;
  const float *x = samples + (size_t)s * D;
  float dist = 0.f;
  if (x[0] == x[0]) dist = distance_vv<METRIC>(x, centroid, D);  // kmeans.cu:53-56
  if (cc == 1 || dist < dists[s]) dists[s] = dist;                // :57-62
}

hipError_t launch_kmpp_step(int metric, const float *samples, uint32_t N, uint32_t D, const float *centroid,
                            uint32_t cc, float *dists, hipStream_t st) {
  const dim3 grid((N + 127) / 128), block(128);
  return with_metric(metric, [&](auto M) {
    hipLaunchKernelGGL((kmpp_step_kernel<M()>), grid, block, 0, st, samples, N, D, centroid, cc, dists);
    return hipGetLastError();
  });
}

// ---------------------------------------------------------------------------------------
// k-means++ chooser on the device.  The reference picks the next seed on the HOST from
// the N distances (kmcuda.cc:286-326): dist_sum = warp-butterfly float sums of 32 accumulated in
// double, then sequential double prefix sums from a guessed start.  Sums of floats in double are EXACT
// -- hence order free, hence parallel -- as long as every partial sum fits 53 bits:
// (max exponent + 1 + ceil(log2 N)) - (min nonzero exponent - 23) <= 53.  The step kernel reports the
// exponent range; when it fits (distances of one data set rarely span more than a few binades) the
// device reproduces the host's choice bit for bit from exact block sums, otherwise (or with a NaN /
// inf distance) the caller falls back to the host path.
// ---------------------------------------------------------------------------------------
constexpr int kKmppBlock = 256;   // rows per block of the step kernel = granularity of the exact prefix sums

struct KmppBlockStat {   // one per block of kKmppBlock rows
  double sum_d;          // exact sum of the block's BULK distances (biased exponent >= the step's cut, below)
  double sum_g;          // exact sum of its per-32 butterfly float sums (over all its distances, as the reference)
  uint32_t emin, emax;   // biased exponent range of its bulk distances (emin > emax: none)
  uint32_t bad;          // a NaN or inf distance
  uint32_t grange;       // (max << 16) | min biased exponent of its non-zero butterfly sums (min 0xFFFF: none)
};

// Round 5: BULK and OUTLIERS.  The chooser's sums are exact -- order free -- only while every partial sum fits a
// double, i.e. while the distances span few enough binades; the angular metric breaks that from the second or third
// seed on (a seed's own row sits at acos(fl(x.x)) = 3.5e-4, twelve binades under the bulk of the angles) and every
// step went to the host chooser (4 ms per step at 8M rows).  Now the non-zero distances below the step's exponent cut
// -- a handful: the seeds' own rows, duplicates of them -- are kept OUT of the exact sums and listed (index, value, the
// exact sum of the bulk distances in front of them in their block), and the chooser replays the host's SEQUENTIAL
// double sum over that list: between two listed values the running sum moves by an exact bulk sum, at a listed value
// it is rounded as the host's addition rounds it, and when it enters a new binade the residue of the listed values
// loses one bit, to even (kmpp_settle).  The cut is the previous step's largest exponent + log2 N - 27: two binades
// inside the window in which bulk sums are exact, so that every bulk partial sum is a multiple of four grid steps of
// the running sum wherever that stands.
struct KmppOutlier {
  uint32_t idx;   // row (in its shard)
  float val;
  double pre;     // exact sum of the bulk distances of its 256-row block in front of it
};
constexpr uint32_t kKmppOutCap = 2048;   // listed values a step may have (more: the host chooser takes the step)

// list != nullptr: the rows list[0 .. *count) only (kmpp_filter_kernel's survivors), blocks striding over the
// list, no block statistics (kmpp_stats_kernel follows)
template <int METRIC>
__global__ __launch_bounds__(kKmppBlock) void kmpp_step2_kernel(const float *__restrict__ samples, uint32_t N,
                                                                uint32_t D, const float *__restrict__ centroid,
                                                                uint32_t cc, float *__restrict__ dists,
                                                                KmppBlockStat *__restrict__ stats,
                                                                const uint32_t *__restrict__ list,
                                                                const uint32_t *__restrict__ count,
                                                                const uint32_t *__restrict__ fail) {
  // *fail != 0: an earlier step of the enqueued run could not be decided on the device (kmpp_choose_kernel): the
  // distances stay as that step left them until the host has chosen its seed
  if (fail && *fail) return;
  __shared__ __attribute__((aligned(16))) float tile[kKmppBlock * 36];
  if (list) {
    const uint32_t n = *count;
    __shared__ uint32_t rows[kKmppBlock];
    for (uint32_t base = blockIdx.x * kKmppBlock; base < n; base += gridDim.x * kKmppBlock) {
      __syncthreads();   // the previous round's tile and rows[] are done with
      rows[threadIdx.x] = base + threadIdx.x < n ? list[base + threadIdx.x] : 0xFFFFFFFFu;
      __syncthreads();
      const uint32_t s = rows[threadIdx.x];
      float acc = 0.f, corr = 0.f, x0 = 0.f;
      if ((D & 3u) == 0 && ((uintptr_t)samples & 15u) == 0) {
        const uint32_t nchunk = (D + 31) / 32;
        for (uint32_t ch = 0; ch < nchunk; ch++) {
          __syncthreads();
#pragma unroll
          for (int q = 0; q < 8; q++) {
            const uint32_t p = threadIdx.x + kKmppBlock * q, r = p >> 3, c4 = p & 7u;
            const uint32_t row = rows[r], f = ch * 32 + c4 * 4;
            const float4 v4 = (row < N && f < D) ? *reinterpret_cast<const float4 *>(samples + (size_t)row * D + f)
                                                 : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4 *>(&tile[r * 36 + c4 * 4]) = v4;
          }
          __syncthreads();
          const uint32_t fmax = D - ch * 32 < 32u ? D - ch * 32 : 32u;   // multiple of 4
          for (uint32_t c4 = 0; c4 * 4 < fmax; c4++) {
            const float4 xv = *reinterpret_cast<const float4 *>(&tile[threadIdx.x * 36 + c4 * 4]);
            const float4 cv = *reinterpret_cast<const float4 *>(centroid + ch * 32 + c4 * 4);
            const float aa[4] = {xv.x, xv.y, xv.z, xv.w}, bb[4] = {cv.x, cv.y, cv.z, cv.w};
            if (ch == 0 && c4 == 0) x0 = aa[0];
#pragma unroll
            for (int q = 0; q < 4; q++) {
              if (METRIC == 0) {
                const float d = aa[q] - bb[q];
                kahan_fold(fma_rd(d, d, corr), acc, corr);
              } else {
                kahan_fold(fma_rd(aa[q], bb[q], corr), acc, corr);
              }
            }
          }
        }
        if (s < N) {
          float dist = 0.f;
          if (x0 == x0) dist = METRIC == 0 ? sqrtf(acc) : angular_from_prod(acc);   // kmeans.cu:53-56
          if (cc == 1 || dist < dists[s]) dists[s] = dist;                            // :57-62
        }
      } else if (s < N) {
        const float *x = samples + (size_t)s * D;
        float dist = 0.f;
        if (x[0] == x[0]) dist = distance_vv<METRIC>(x, centroid, D);
        if (cc == 1 || dist < dists[s]) dists[s] = dist;
      }
    }
    return;
  }
  const uint32_t s = blockIdx.x * kKmppBlock + threadIdx.x;
  float v = 0.f;   // rows past N count as 0, like the host emulation of the butterfly
  if ((D & 3u) == 0 && ((uintptr_t)samples & 15u) == 0) {
    // One serial chain per row, but the rows come in through LDS: a thread walking its own row makes
    // every 16-byte load of a wave touch 64 different lines (1.1 TB/s measured).  Chunks of 32
    // features: 8 lanes fetch a row's 128-byte line, the tile is stored with a 36-float row stride
    // (conflict-free b128 reads by 16 consecutive rows), the next chunk's loads fly during the chain.
    const uint32_t nchunk = (D + 31) / 32;
    float4 stage[8];
    auto fetch = [&](uint32_t ch) {
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const uint32_t p = threadIdx.x + kKmppBlock * q, r = p >> 3, c4 = p & 7u;
        const uint32_t row = blockIdx.x * kKmppBlock + r, f = ch * 32 + c4 * 4;
        stage[q] = (row < N && f < D) ? *reinterpret_cast<const float4 *>(samples + (size_t)row * D + f)
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    };
    float acc = 0.f, corr = 0.f, x0 = 0.f;
    fetch(0);
    for (uint32_t ch = 0; ch < nchunk; ch++) {
      __syncthreads();   // the previous chunk has been consumed
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const uint32_t p = threadIdx.x + kKmppBlock * q, r = p >> 3, c4 = p & 7u;
        *reinterpret_cast<float4 *>(&tile[r * 36 + c4 * 4]) = stage[q];
      }
      __syncthreads();
      if (ch + 1 < nchunk) fetch(ch + 1);
      const uint32_t fmax = D - ch * 32 < 32u ? D - ch * 32 : 32u;   // multiple of 4
      for (uint32_t c4 = 0; c4 * 4 < fmax; c4++) {
        const float4 xv = *reinterpret_cast<const float4 *>(&tile[threadIdx.x * 36 + c4 * 4]);
        const float4 cv = *reinterpret_cast<const float4 *>(centroid + ch * 32 + c4 * 4);
        const float aa[4] = {xv.x, xv.y, xv.z, xv.w}, bb[4] = {cv.x, cv.y, cv.z, cv.w};
        if (ch == 0 && c4 == 0) x0 = aa[0];
#pragma unroll
        for (int q = 0; q < 4; q++) {
          if (METRIC == 0) {
            const float d = aa[q] - bb[q];
            kahan_fold(fma_rd(d, d, corr), acc, corr);
          } else {
            kahan_fold(fma_rd(aa[q], bb[q], corr), acc, corr);
          }
        }
      }
    }
    if (s < N) {
      float dist = 0.f;
      if (x0 == x0) dist = METRIC == 0 ? sqrtf(acc) : angular_from_prod(acc);   // kmeans.cu:53-56
      if (cc == 1 || dist < dists[s]) dists[s] = dist; else dist = dists[s];     // :57-62
      v = dist;
    }
  } else if (s < N) {
    const float *x = samples + (size_t)s * D;
    float dist = 0.f;
    if (x[0] == x[0]) dist = distance_vv<METRIC>(x, centroid, D);  // kmeans.cu:53-56
    if (cc == 1 || dist < dists[s]) dists[s] = dist; else dist = dists[s];   // :57-62
    v = dist;
  }
  (void)v;
  (void)stats;   // (the block statistics are kmpp_stats_kernel's, which follows every step)
}

// block statistics of the distances as they stand (after a step): ONE WAVE per block of kKmppBlock rows, four trips
// of 64 rows, no LDS, no barrier (four waves meeting in LDS was latency: 70 us for 32 MB).  The butterfly sums are per
// 32 lanes, the double sums exact in any order.  *ecut (0 counts as 1): the step's exponent cut; the non-zero
// distances below it are listed in outl / *outl_count instead of summed (KmppOutlier).
__global__ __launch_bounds__(256) void kmpp_stats_kernel(const float *__restrict__ dists, uint32_t N,
                                                         KmppBlockStat *__restrict__ stats,
                                                         uint32_t *__restrict__ list_count,
                                                         const uint32_t *__restrict__ fail,
                                                         const uint32_t *__restrict__ ecut_ptr,
                                                         KmppOutlier *__restrict__ outl, uint32_t *__restrict__ outl_count) {
  if (*fail) return;
  if (list_count && blockIdx.x == 0 && threadIdx.x == 0) {   // the step's survivor list has been consumed (stream order); [1..2] behind it: the running total
    *reinterpret_cast<unsigned long long *>(list_count + 1) += *list_count;
    *list_count = 0u;
  }
  const uint32_t ecut = max(*ecut_ptr, 1u);
  const uint32_t nb = (N + kKmppBlock - 1) / kKmppBlock;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave_global = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  for (uint32_t b = wave_global; b < nb; b += nwaves) {
    float v[kKmppBlock / 64];
#pragma unroll
    for (int t = 0; t < kKmppBlock / 64; t++) {
      const uint32_t s = b * kKmppBlock + t * 64 + lane;
      v[t] = s < N ? dists[s] : 0.f;
    }
    double sd = 0.0, sg = 0.0;
    uint32_t emin = 0xFFFFu, emax = 0u, bad = 0u, gmin = 0xFFFFu, gmax = 0u;
    bool isbulk[kKmppBlock / 64], isout[kKmppBlock / 64];
    unsigned long long any_out = 0ull;
#pragma unroll
    for (int t = 0; t < kKmppBlock / 64; t++) {
      float g = v[t];   // warpReduceSum over 32 lanes (kmeans.cu:63-66)
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) g = g + __shfl_down(g, off, 32);
      const uint32_t bits = __float_as_uint(v[t]), ex = (bits >> 23) & 0xFFu;
      const bool finite = ex != 0xFFu, nz = (bits & 0x7FFFFFFFu) != 0u;
      const uint32_t ee = ex ? ex : 1u;
      isbulk[t] = finite && nz && ee >= ecut;
      isout[t] = finite && nz && ee < ecut;
      if (isbulk[t]) {
        sd += (double)v[t];
        emin = min(emin, ee);
        emax = max(emax, ee);
      }
      if ((lane & 31) == 0) {
        sg += (double)g;
        const uint32_t gb = __float_as_uint(g), gx = (gb >> 23) & 0xFFu;
        if (gx != 0xFFu && (gb & 0x7FFFFFFFu) != 0u) {
          gmin = min(gmin, gx ? gx : 1u);
          gmax = max(gmax, gx ? gx : 1u);
        }
      }
      bad |= finite ? 0u : 1u;
      any_out |= __ballot(isout[t]);
    }
    if (any_out) {   // (wave-uniform; rare) the listed values with the exact bulk sum in front of each
      double carry = 0.0;
#pragma unroll
      for (int t = 0; t < kKmppBlock / 64; t++) {
        const double bv = isbulk[t] ? (double)v[t] : 0.0;
        double inc = bv;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const double up = __shfl_up(inc, o);
          if ((int)lane >= o) inc += up;
        }
        const unsigned long long m = __ballot(isout[t]);
        if (m) {
          uint32_t base = 0;
          if (lane == 0) base = atomicAdd(outl_count, (uint32_t)__popcll(m));
          base = __shfl(base, 0);
          const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
          if (isout[t] && at < kKmppOutCap) {
            KmppOutlier o;
            o.idx = b * kKmppBlock + t * 64 + lane;
            o.val = v[t];
            o.pre = carry + (inc - bv);
            outl[at] = o;
          }
        }
        carry += __shfl(inc, 63);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sd += __shfl_xor(sd, off);
      sg += __shfl_xor(sg, off);
      emin = min(emin, (uint32_t)__shfl_xor((int)emin, off));
      emax = max(emax, (uint32_t)__shfl_xor((int)emax, off));
      gmin = min(gmin, (uint32_t)__shfl_xor((int)gmin, off));
      gmax = max(gmax, (uint32_t)__shfl_xor((int)gmax, off));
      bad |= (uint32_t)__shfl_xor((int)bad, off);
    }
    if (lane == 0) {
      KmppBlockStat st;
      st.sum_d = sd; st.sum_g = sg; st.emin = emin; st.emax = emax; st.bad = bad; st.grange = (gmax << 16) | gmin;
      stats[b] = st;
    }
  }
}

// ---------------------------------------------------------------------------------------
// Filtered steps.  A step only changes dists[s] where the new seed is CLOSER than the row's nearest seed so
// far -- one row in i at step i on average -- but the plain step streams all N rows (4 D bytes each) to find out.
// Here the rows are kept a second time as centred BYTES, x' = x - mu ~ a q with q in [-127, 127] and a = max |x'| /
// 127 per row, beside (a, an upper bound of ||x' - a q||, ||x'||^2, mu.x') per row (DP + 16 bytes; kmpp_cache_kernel,
// once per call).  A step's first kernel forms a (q . s') per row (8 lanes per row, the seed s' = s - mu in fp32,
// fp32 accumulation) and drops every row whose distance to the new seed provably is not below dists[s]: the cluster-
// pruned k-NN search's candidate test with one query, the seed, and a threshold per candidate (knn_f16.hip, DESIGN.md
// 4.2 / 4.5), with that test's operand-rounding term (halves: 2^-10 ||x'|| ||s'||) replaced by the row's MEASURED
// residual, |x'.s' - a q.s'| <= ||x' - a q|| ||s'||.  Only the survivors' exact chains run (kmpp_step2_kernel over
// the list).  dists[] afterwards is the plain step's bit for bit: a dropped row keeps its value in both.
// (Round 3 first kept the rows as halves: 0.62 % of the (row, step) pairs survived on 8M uniform rows in 256-D, and
// the 4.1-GB stream was 87 % of the seeding.  Bytes halve the stream; the margin a new seed has to beat -- the gap
// between a row's distance to a random point and to the nearest of i seeds -- is two orders of magnitude wider than
// either rounding, so the survivors stay what they were.)
// ---------------------------------------------------------------------------------------
typedef float f32x4_kp __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_kp __attribute__((ext_vector_type(4)));

// column sums of (up to) the first `rows` rows, one partial per block in fixed order: part[b][f]
__global__ __launch_bounds__(256) void kmpp_colsum_kernel(const float *__restrict__ samples, uint32_t rows, uint32_t D,
                                                          double *__restrict__ part) {
  for (uint32_t f = threadIdx.x; f < D; f += 256) {
    double acc = 0.0;
    for (uint32_t r = blockIdx.x; r < rows; r += gridDim.x) {
      const float v = samples[(size_t)r * D + f];
      if ((v - v) == 0.f) acc += (double)v;   // finite values only: mu is just a translation
    }
    part[(size_t)blockIdx.x * D + f] = acc;
  }
}
__global__ __launch_bounds__(256) void kmpp_mean_kernel(const double *__restrict__ part, uint32_t nblocks, uint32_t rows,
                                                        uint32_t D, uint32_t DP, float *__restrict__ mu) {
  const uint32_t f = blockIdx.x * 256 + threadIdx.x;
  if (f >= DP) return;
  double acc = 0.0;
  if (f < D)
    for (uint32_t b = 0; b < nblocks; b++) acc += part[(size_t)b * D + f];
  mu[f] = f < D ? (float)(acc / (double)rows) : 0.f;
}

// one wave per row: q = round(x' / a) as bytes (zero padded to DP), meta = (a, residual bound, ||x'||^2, mu.x')
__global__ __launch_bounds__(256) void kmpp_cache_kernel(const float *__restrict__ samples, uint32_t N, uint32_t D,
                                                         uint32_t DP, const float *__restrict__ mu,
                                                         signed char *__restrict__ xs8, f32x4_kp *__restrict__ meta) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t p = blockIdx.x * 4 + (threadIdx.x >> 6); p < N; p += gridDim.x * 4) {   // (kernels.hpp: wave_row_grid)
    const float *src = samples + (size_t)p * D;
    signed char *dst = xs8 + (size_t)p * DP;
    float n2 = 0.f, mx = 0.f, mb = 0.f;
    for (uint32_t f = lane; f < D; f += 64) {
      const float m = mu[f], v = src[f] - m;
      n2 = fmaf(v, v, n2);
      mb = fmaf(m, v, mb);
      mx = fmaxf(mx, fabsf(v));   // (fmaxf drops a NaN operand: a NaN row shows in n2)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      n2 += __shfl_xor(n2, off);
      mb += __shfl_xor(mb, off);
      mx = fmaxf(mx, __shfl_xor(mx, off));
    }
    const bool fin = (n2 - n2) == 0.f;
    const float a = fin ? mx / 127.0f : 0.f, inv = (fin && a > 0.f) ? 1.0f / a : 0.f;
    float r2 = 0.f;
    for (uint32_t f = lane; f < DP; f += 64) {
      float q = 0.f;
      if (f < D && fin) {
        const float v = src[f] - mu[f];
        q = fminf(fmaxf(rintf(v * inv), -127.f), 127.f);
        const float r = v - a * q;
        r2 = fmaf(r, r, r2);
      }
      dst[f] = (signed char)(int)q;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) r2 += __shfl_xor(r2, off);
    if (lane == 0) {
      // the residual's norm from above: its fp32 evaluation is off by a few ulps of ||x'|| at most
      const float rn = (sqrtf(r2) + 1e-6f * sqrtf(n2)) * 1.001f;
      // a row that is not finite keeps NaN in its record: the filter never drops it
      meta[p] = f32x4_kp{fin ? a : __builtin_nanf(""), rn, n2, mb};
    }
  }
}

// PPL: 16-byte pieces per lane and row (DP = 128 PPL), 0 = any DP (rolled loops).  With PPL known a wave has the
// pieces of 4 x 8 rows in flight before the first product (a 2-GB stream per step: bandwidth is the whole cost).
template <int PPL, int METRIC>
__global__ __launch_bounds__(256) void kmpp_filter_kernel(const signed char *__restrict__ xs8,
                                                          const f32x4_kp *__restrict__ meta,
                                                          const float *__restrict__ mu, const float *__restrict__ seed,
                                                          uint32_t N, uint32_t D, uint32_t DP, float eps,
                                                          const float *__restrict__ dists, uint32_t *__restrict__ list,
                                                          uint32_t *__restrict__ count, const uint32_t *__restrict__ fail) {
  extern __shared__ __attribute__((aligned(16))) float sfl[];   // DP floats: s' = s - mu
  if (*fail) return;
  __shared__ float red[3][4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float part = 0.f, pmus = 0.f, pmu2 = 0.f;
  for (uint32_t f = threadIdx.x; f < DP; f += 256) {
    const float m = f < D ? mu[f] : 0.f;
    const float v = f < D ? seed[f] - m : 0.f;
    sfl[f] = v;
    part = fmaf(v, v, part);
    pmus = fmaf(m, v, pmus);
    pmu2 = fmaf(m, m, pmu2);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    part += __shfl_xor(part, off);
    pmus += __shfl_xor(pmus, off);
    pmu2 += __shfl_xor(pmu2, off);
  }
  if (lane == 0) { red[0][wave] = part; red[1][wave] = pmus; red[2][wave] = pmu2; }
  __syncthreads();
  const float sn2 = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);   // ||s'||^2 (the "query" of knn_f16.hip)
  const float mus = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);   // mu.s'
  const float mu2 = ((red[2][0] + red[2][1]) + (red[2][2] + red[2][3])) * 1.0001f;   // ||mu||^2, as knn_cuda inflates it
  const float u = 5.9604645e-8f;
  const float qn = sqrtf(sn2) * 1.0001f, mun = sqrtf(mu2) * 1.0001f;
  const float kq = mus + mu2;
  const bool usable = (sn2 - sn2) == 0.f && (mu2 - mu2) == 0.f && qn < 1.0e18f;
  const uint32_t l8 = lane & 7u, rsub = lane >> 3;
  constexpr uint32_t kBuf = 128;
  __shared__ uint32_t buf[4][kBuf];
  uint32_t *mine = buf[wave];
  uint32_t buffered = 0;   // wave-uniform
  auto flush = [&]() {
    if (buffered == 0) return;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(count, buffered);
    base = __shfl(base, 0);
    for (uint32_t i = lane; i < buffered; i += 64) list[base + i] = mine[i];
    buffered = 0;
  };
  // knn_f16.hip's bound with one query (the seed) and this row as the candidate: the row can only come closer than
  // T = dists[s] if   (L2)       a q.s' - ||x'||^2 / 2  >=  (||s'||^2 - T^2 - E) / 2 - 1e-6 (||s'||^2 + T^2)
  //                   (angular)  a q.s' + mu.x'         >=  cos T - (mu.s' + ||mu||^2) - E
  // E: the reference's own rounding + the centring in fp32 (the k-NN filter's terms, with this row's norm) + the
  // quantisation, |x'.s' - a q.s'| <= rn ||s'||, + the fp32 accumulation of q.s' (gamma_D ||x'|| ||s'||)
  auto decide = [&](uint32_t s, bool live, float acc) {
    acc += __shfl_xor(acc, 1);
    acc += __shfl_xor(acc, 2);
    acc += __shfl_xor(acc, 4);
    bool need = false;
    if (live && l8 == 0) {
      const f32x4_kp m = meta[s];
      const float a = m.x, rn = m.y, n2 = m.z, T = dists[s];
      const float xn = sqrtf(n2) * 1.0001f;
      const float e_q = rn * qn * 1.001f + eps * xn * qn;
      float score, amin;
      if (METRIC == 0) {
        const float E = 4.04f * (3.0f * eps + 16.0f * u) * (sn2 + n2) + 6e-8f * sqrtf((float)DP) * (qn + xn) + 2.0f * e_q;
        score = a * acc - 0.5f * n2;
        const float T2 = T * T * 1.000001f;
        amin = 0.5f * (sn2 - T2 - E) - 1e-6f * (sn2 + T2);
      } else {
        const float E = 2.02f * (3.0f * eps + 16.0f * u) * (qn * xn + mun * xn) + 3e-8f * sqrtf((float)DP) * (qn + xn) +
                        eps * (mun * qn + mu2) + 1e-6f + e_q;
        score = a * acc + m.w;
        amin = T >= 3.1415925f ? -INFINITY : cosf(T) - kq - E;
      }
      // (a NaN anywhere -- a row that is not finite has NaN for a -- : not dropped; norms near the end of the float
      //  range, where the bound's own products would overflow: neither)
      need = !(usable && xn < 1.0e18f && score < amin);
    }
    // Survivors wait in the wave's LDS buffer: one global atomic per kBuf of them, not one per 8-row group (same-
    // address atomics are served one at a time by L2: 50 K of them per step were half of the kernel's time)
    const unsigned long long m = __ballot(need);
    if (m) {
      const uint32_t n = (uint32_t)__popcll(m);
      if (buffered + n > kBuf) flush();
      if (need) mine[buffered + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = s;
      buffered += n;
    }
  };
  // 16 bytes of q against 16 floats of s'
  auto dot16 = [](const u32x4_kp &xq, const float *sv, float acc) {
#pragma unroll
    for (int w = 0; w < 4; w++) {
      const int x = (int)xq[w];
      acc = fmaf((float)(signed char)(x & 0xFF), sv[4 * w + 0], acc);
      acc = fmaf((float)(signed char)((x >> 8) & 0xFF), sv[4 * w + 1], acc);
      acc = fmaf((float)(signed char)((x >> 16) & 0xFF), sv[4 * w + 2], acc);
      acc = fmaf((float)(x >> 24), sv[4 * w + 3], acc);
    }
    return acc;
  };
  if constexpr (PPL > 0) {
    constexpr int R = 4;   // 8-row groups in flight per wave
    float sv[PPL][16];
#pragma unroll
    for (int i = 0; i < PPL; i++)
#pragma unroll
      for (int q = 0; q < 16; q++) sv[i][q] = sfl[(l8 + 8 * i) * 16 + q];
    for (uint32_t row0 = (blockIdx.x * 4 + wave) * (8 * R); row0 < N; row0 += gridDim.x * (32 * R)) {
      u32x4_kp xv[R][PPL];
#pragma unroll
      for (int r = 0; r < R; r++) {
        const uint32_t s = row0 + 8 * r + rsub;
        const u32x4_kp *xr = reinterpret_cast<const u32x4_kp *>(xs8 + (size_t)(s < N ? s : 0) * DP);
#pragma unroll
        for (int i = 0; i < PPL; i++) xv[r][i] = __builtin_nontemporal_load(&xr[l8 + 8 * i]);
      }
#pragma unroll
      for (int r = 0; r < R; r++) {
        const uint32_t s = row0 + 8 * r + rsub;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < PPL; i++) acc = dot16(xv[r][i], sv[i], acc);
        decide(s, s < N, acc);
      }
    }
  } else {
    const uint32_t npieces = DP / 16;   // 16-byte pieces per row; DP is a multiple of 128
    for (uint32_t row0 = (blockIdx.x * 4 + wave) * 8; row0 < N; row0 += gridDim.x * 32) {
      const uint32_t s = row0 + rsub;
      const bool live = s < N;
      const u32x4_kp *xr = reinterpret_cast<const u32x4_kp *>(xs8 + (size_t)(live ? s : 0) * DP);
      float acc = 0.f;
      for (uint32_t p = l8; p < npieces; p += 8) acc = dot16(xr[p], &sfl[p * 16], acc);
      decide(s, live, acc);
    }
  }
  flush();
}

// out[c][:] = samples[idx[c]][:] for c < K: the K seed rows of init = "random" in one launch (1024 separate
// device-to-device copies were 2 ms of a 20-ms call)
__global__ __launch_bounds__(256) void gather_rows_kernel(const float *__restrict__ samples, const uint32_t *__restrict__ idx,
                                                          uint32_t K, uint32_t D, float *__restrict__ out) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6); c < K; c += gridDim.x * 4) {
    const float *src = samples + (size_t)idx[c] * D;
    for (uint32_t f = lane; f < D; f += 64) out[(size_t)c * D + f] = src[f];
  }
}
hipError_t launch_gather_rows(const float *samples, const uint32_t *idx, uint32_t K, uint32_t D, float *out, hipStream_t st) {
  hipLaunchKernelGGL(gather_rows_kernel, dim3(wave_row_grid(K)), dim3(256), 0, st, samples, idx, K, D, out);
  return hipGetLastError();
}

struct KmppTotals {   // device memory, one per shard (the host allocates kmpp_totals_bytes() and never reads it)
  double sum_g, sum_d;
  uint32_t emin, emax, bad, chosen;
  uint32_t grange, pad;   // exponent range of the non-zero butterfly sums ((max << 16) | min)
};

// Exclusive prefix of the block sums in two launches.  (a) every 1024 block statistics: their local exclusive
// prefix -> bpre[i], their totals -> aux[b]; (b) one block: exclusive prefix of the aux sums -> carry[b],
// carry[nchunks] = the total, the other totals -> out.  prefix of block i = bpre[i] + carry[i / 1024]: every
// partial sum is exact (caller's exponent-range test), so the association does not matter.
struct KmppChunk {
  double sum, sg;
  uint32_t emin, emax, bad, grange;
};
__device__ __forceinline__ uint32_t kmpp_grange_join(uint32_t a, uint32_t b) {
  return (max(a >> 16, b >> 16) << 16) | min(a & 0xFFFFu, b & 0xFFFFu);
}
__global__ __launch_bounds__(1024) void kmpp_reduce_a_kernel(const KmppBlockStat *__restrict__ stats, uint32_t nb,
                                                             double *__restrict__ bpre, KmppChunk *__restrict__ aux,
                                                             const uint32_t *__restrict__ fail) {
  if (fail && *fail) return;
  __shared__ double wsum[16], wsg[16];
  __shared__ uint32_t wmin[16], wmax[16], wbad[16], wgr[16];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x * 1024 + threadIdx.x;
  const bool in = i < nb;
  const double v = in ? stats[i].sum_d : 0.0;
  double sg = in ? stats[i].sum_g : 0.0;
  uint32_t emin = in ? stats[i].emin : 0xFFFFu, emax = in ? stats[i].emax : 0u, bad = in ? stats[i].bad : 0u;
  uint32_t gr = in ? stats[i].grange : 0xFFFFu;
  double inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(inc, o);
    if ((int)lane >= o) inc += t;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sg += __shfl_xor(sg, o);
    emin = min(emin, (uint32_t)__shfl_xor((int)emin, o));
    emax = max(emax, (uint32_t)__shfl_xor((int)emax, o));
    bad |= (uint32_t)__shfl_xor((int)bad, o);
    gr = kmpp_grange_join(gr, (uint32_t)__shfl_xor((int)gr, o));
  }
  if (lane == 63) wsum[wave] = inc;
  if (lane == 0) { wsg[wave] = sg; wmin[wave] = emin; wmax[wave] = emax; wbad[wave] = bad; wgr[wave] = gr; }
  __syncthreads();
  double wbase = 0.0, all = 0.0;
#pragma unroll
  for (uint32_t k = 0; k < 16; k++) {
    const double t = wsum[k];
    if (k < wave) wbase += t;
    all += t;
  }
  if (in) bpre[i] = wbase + inc - v;
  if (threadIdx.x == 0) {
    KmppChunk c;
    c.sum = all;
    double g = 0.0;
    uint32_t mn = 0xFFFFu, mx = 0u, bd = 0u, gg = 0xFFFFu;
    for (uint32_t k = 0; k < 16; k++) { g += wsg[k]; mn = min(mn, wmin[k]); mx = max(mx, wmax[k]); bd |= wbad[k]; gg = kmpp_grange_join(gg, wgr[k]); }
    c.sg = g; c.emin = mn; c.emax = mx; c.bad = bd; c.grange = gg;
    aux[blockIdx.x] = c;
  }
}
// nchunks <= 1024
__global__ __launch_bounds__(1024) void kmpp_reduce_b_kernel(const KmppChunk *__restrict__ aux, uint32_t nchunks,
                                                             double *__restrict__ carry, KmppTotals *__restrict__ out,
                                                             const uint32_t *__restrict__ fail) {
  if (fail && *fail) return;
  __shared__ double wsum[16], wsg[16];
  __shared__ uint32_t wmin[16], wmax[16], wbad[16], wgr[16];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool in = threadIdx.x < nchunks;
  const double v = in ? aux[threadIdx.x].sum : 0.0;
  double sg = in ? aux[threadIdx.x].sg : 0.0;
  uint32_t emin = in ? aux[threadIdx.x].emin : 0xFFFFu, emax = in ? aux[threadIdx.x].emax : 0u,
           bad = in ? aux[threadIdx.x].bad : 0u, gr = in ? aux[threadIdx.x].grange : 0xFFFFu;
  double inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(inc, o);
    if ((int)lane >= o) inc += t;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sg += __shfl_xor(sg, o);
    emin = min(emin, (uint32_t)__shfl_xor((int)emin, o));
    emax = max(emax, (uint32_t)__shfl_xor((int)emax, o));
    bad |= (uint32_t)__shfl_xor((int)bad, o);
    gr = kmpp_grange_join(gr, (uint32_t)__shfl_xor((int)gr, o));
  }
  if (lane == 63) wsum[wave] = inc;
  if (lane == 0) { wsg[wave] = sg; wmin[wave] = emin; wmax[wave] = emax; wbad[wave] = bad; wgr[wave] = gr; }
  __syncthreads();
  double wbase = 0.0, all = 0.0;
#pragma unroll
  for (uint32_t k = 0; k < 16; k++) {
    const double t = wsum[k];
    if (k < wave) wbase += t;
    all += t;
  }
  if (in) carry[threadIdx.x] = wbase + inc - v;
  if (threadIdx.x == 0) {
    carry[nchunks] = all;
    double g = 0.0;
    uint32_t mn = 0xFFFFu, mx = 0u, bd = 0u, gg = 0xFFFFu;
    for (uint32_t k = 0; k < 16; k++) { g += wsg[k]; mn = min(mn, wmin[k]); mx = max(mx, wmax[k]); bd |= wbad[k]; gg = kmpp_grange_join(gg, wgr[k]); }
    out->sum_g = g;
    out->sum_d = all;
    out->emin = mn;
    out->emax = mx;
    out->bad = bd;
    out->grange = gg;
  }
}

// The host chooser (kmcuda.cc:300-326) on exact prefix sums.  prefix(m) = sum of d[0..m).
//   forward search  m0(dca) = min { m in [0, N] : prefix(m) - dca >= cs }  (N when there is none)
//   choice_approx < 100, or prefix(ca) < cs :  j = m0(0)
//   else (backward loop, which subtracts d[ca] first):  j = max(2, min(m0(d[ca]) - 1, ca + 1))
// Called with the step's random number only (choice in [0, 1], kmcuda.cc:300): the totals of the step are read from
// the device, so the host need not wait for them -- it enqueues step after step.  A step the device cannot decide (a
// NaN / inf distance, an exponent range too wide for exact sums, an index out of range) raises *fail = step: every
// later kmpp kernel of the run returns at once, and the host chooses that seed the reference's way before it goes on.
// Otherwise the chosen row is copied into centroid slot `step` here.
//
// ROW SHARDS (round 5; kmeans.cu:774-828 runs the step on every device, kmcuda.cc:286-326 chooses on the host from all
// N distances): every shard runs the step on its own rows and leaves its own block sums, local prefixes and totals
// (launch_kmpp_step2 / _filtered with the shard's length); ONE chooser -- this kernel, on the first shard's device --
// reads them where they lie (peer access; a few KB per step) as the concatenation they are: the exact prefix of global
// block i is  (the exact sum of the earlier shards' totals) + (the owning shard's local prefix).  Exact sums are
// order free, so every number the chooser compares is the one-shard chooser's, bit for bit, and so is the seed; the
// seed's row is copied from its owner into slot `step` of EVERY shard's centroid replica by this kernel.  No
// N-sized transfer, no host in the loop.  Needs every shard but the last to hold whole blocks of kKmppBlock rows
// (row_plan() aligns the shards that way): the reference's butterfly sums are over aligned groups of 32 rows.
struct KmppShardView {
  const float *dists;        // the shard's distances (its rows in order)
  const double *bpre;        // its local block prefixes + carries (launch_kmpp_reduce)
  const KmppTotals *totals;  // its totals
  const float *samples;      // its rows
  float *centroids;          // its centroid replica (slot `step` is written)
  uint32_t *fail;            // its fail flag (raised on every shard together)
  uint32_t *ecut;            // its exponent cut: read (this step's), then written (the next step's)
  const KmppOutlier *outl;   // its listed values ...
  uint32_t *outl_count;      // ... and their number (zeroed here for the next step)
  uint32_t offset, length;   // its rows: [offset, offset + length) of the N; offset % kKmppBlock == 0
};
struct KmppShards {
  KmppShardView s[kKmppMaxShards];
  uint32_t n;
};

__device__ __forceinline__ int kmpp_ilogb(double x) {   // floor(log2 |x|), x finite, normal, non-zero
  return (int)(((unsigned long long)__double_as_longlong(x) >> 52) & 0x7FFull) - 1023;
}
__device__ __forceinline__ int kmpp_lowbit(double r) {  // exponent of r's lowest set bit (r normal, non-zero)
  const unsigned long long m = ((unsigned long long)__double_as_longlong(r) & 0xFFFFFFFFFFFFFull) | 0x10000000000000ull;
  return kmpp_ilogb(r) - 52 + (__ffsll((long long)m) - 1);
}
// The host's running sum, in double, is (exact bulk sum so far) + r, r being what the listed values have left in
// it.  While bulk values are added that stays exact until the sum enters a binade whose grid is coarser than r's
// lowest bit; there the addition rounds, and what it drops is exactly that one bit (r is a multiple of the old grid,
// the bulk part a multiple of four new grid steps: the caller's range test): a tie, to even, decided by r's own next
// bit.  One bit per binade entered, in this order -- not the same as one rounding to the final grid.
__device__ double kmpp_settle(double r, double B) {
  for (int guard = 0; guard < 80 && r != 0.0; guard++) {
    const double x = B + r;   // (only its binade is used)
    if (x == 0.0) break;
    const int lb = kmpp_lowbit(r);
    if (lb >= kmpp_ilogb(x) - 52) break;
    const double C = ldexp(1.5, 52 + lb + 1);   // (r + C) - C: r to a multiple of 2^(lb + 1), ties to even
    const double t = r + C;
    r = t - C;
  }
  return r;
}

__global__ __launch_bounds__(kKmppBlock) void kmpp_choose_kernel(KmppShards sh, uint32_t N, double choice, uint32_t log2n,
                                                                 uint32_t step, uint32_t D, KmppTotals *__restrict__ out) {
  if (*sh.s[0].fail) return;
  const uint32_t tid = threadIdx.x, S = sh.n;
  __shared__ double base[kKmppMaxShards + 1];    // exact sum of the bulk distances of the shards before s; [S] = of all
  __shared__ uint32_t blk0[kKmppMaxShards + 1];  // first global block of shard s; [S] = the number of blocks
  __shared__ uint32_t obase[kKmppMaxShards + 1]; // listed values of the shards before s
  __shared__ double sum_g_s;
  __shared__ uint32_t exact_s, ecut_s;
  // the listed values of all shards, by global row (sorted below): 32 KB
  __shared__ uint32_t o_idx[kKmppOutCap];
  __shared__ float o_val[kKmppOutCap];
  __shared__ double o_bulk[kKmppOutCap];          // exact sum of the bulk distances in front of the row
  auto fail_all = [&]() {
    for (uint32_t i = 0; i < S; i++) {
      *sh.s[i].fail = step;
      *sh.s[i].outl_count = 0u;   // (the host chooser takes the step from dists[]; the next step lists afresh)
    }
  };
  if (tid == 0) {
    double b = 0.0, g = 0.0;
    uint32_t emin = 0xFFFFu, emax = 0u, bad = 0u, gr = 0xFFFFu, no = 0u;
    for (uint32_t i = 0; i < S; i++) {
      const KmppTotals *t = sh.s[i].totals;
      base[i] = b;
      blk0[i] = sh.s[i].offset / kKmppBlock;
      obase[i] = no;
      b += t->sum_d;
      g += t->sum_g;
      emin = min(emin, t->emin);
      emax = max(emax, t->emax);
      bad |= t->bad;
      gr = kmpp_grange_join(gr, t->grange);
      no += *sh.s[i].outl_count;   // (counts every attempt: beyond the capacity = too many)
    }
    base[S] = b;
    blk0[S] = (N + kKmppBlock - 1) / kKmppBlock;
    obase[S] = no;
    sum_g_s = g;
    ecut_s = max(*sh.s[0].ecut, 1u);   // (the same on every shard: written below)
    // every partial sum of the bulk distances is exact in double iff (emax + 1 + log2 N) - (emin - 23) <= 53; with
    // listed values two binades more are asked for (kmpp_settle: the bulk part a multiple of four grid steps); the
    // butterfly sums of 32 likewise (N / 32 of them)
    const bool none = emin > emax;
    const uint32_t window = no ? 27u : 29u;
    const uint32_t gmin = gr & 0xFFFFu, gmax = gr >> 16;
    const bool gnone = gmin > gmax;
    const bool ok = !bad && (none || emax - emin + log2n <= window) &&
                    (gnone || gmax - gmin + (log2n > 5u ? log2n - 5u : 0u) <= 29u) && no <= kKmppOutCap;
    exact_s = ok ? 1u : 0u;
    if (!ok) fail_all();
    // the next step's cut, also behind a step that goes to the host (the first angular step does: nothing is listed
    // yet): distances only shrink from step to step, so this step's largest exponent bounds the next's
    const uint32_t next = (none || bad) ? 1u : (emax + log2n > 27u ? emax + log2n - 27u : 1u);
    for (uint32_t i = 0; i < S; i++) *sh.s[i].ecut = next;
  }
  __syncthreads();
  if (!exact_s) return;
  const uint32_t nb = blk0[S], nout = obase[S], ecut = ecut_s;
  const uint32_t ca = (uint32_t)(choice * (double)N);   // kmcuda.cc:301-302
  const double cs = choice * sum_g_s;
  // exclusive BULK prefix of global block i (i <= nb): the owner's chunk-local part + its chunk's carry (kmpp_reduce_*,
  // stored behind the shard's local values) + the exact sum of the shards before it; bpre[nb] = the total
  auto shard_of_block = [&](uint32_t i) -> uint32_t {
    uint32_t o = 0;
    for (uint32_t q = 1; q < S; q++)
      if (i >= blk0[q]) o = q;
    return o;
  };
  auto bpre = [&](uint32_t i) -> double {
    if (i >= nb) return base[S];
    const uint32_t o = shard_of_block(i), li = i - blk0[o];
    const uint32_t nbl = (sh.s[o].length + kKmppBlock - 1) / kKmppBlock;
    const double *loc = sh.s[o].bpre;
    return base[o] + (loc[li] + loc[nbl + (li >> 10)]);
  };
  auto dist_at = [&](uint32_t row) -> float {   // row < N
    const uint32_t o = shard_of_block(row / kKmppBlock);
    return sh.s[o].dists[row - sh.s[o].offset];
  };
  auto bulk_of = [&](float v) -> double {       // v as the bulk sums count it (a listed value, a zero: nothing)
    const uint32_t bits = __float_as_uint(v), ex = (bits >> 23) & 0xFFu;
    return ((bits & 0x7FFFFFFFu) != 0u && (ex ? ex : 1u) >= ecut) ? (double)v : 0.0;
  };
  // ---- the listed values, by global row ----
  if (nout) {
    uint32_t n2 = 1;
    while (n2 < nout) n2 <<= 1;
    for (uint32_t i = tid; i < n2; i += kKmppBlock) {
      uint32_t gi = 0xFFFFFFFFu;
      float v = 0.f;
      double bk = 0.0;
      if (i < nout) {
        uint32_t o = 0;
        for (uint32_t q = 1; q < S; q++)
          if (i >= obase[q]) o = q;
        const KmppOutlier rec = sh.s[o].outl[i - obase[o]];
        gi = sh.s[o].offset + rec.idx;
        v = rec.val;
        bk = bpre(gi / kKmppBlock) + rec.pre;
      }
      o_idx[i] = gi; o_val[i] = v; o_bulk[i] = bk;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= n2; k <<= 1) {       // bitonic sort by row (rows are distinct)
      for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
        for (uint32_t i = tid; i < n2; i += kKmppBlock) {
          const uint32_t l = i ^ jj;
          if (l > i) {
            const uint32_t x = o_idx[i], y = o_idx[l];
            const bool up = (i & k) == 0;
            if ((x > y) == up) {
              o_idx[i] = y; o_idx[l] = x;
              const float fv = o_val[i]; o_val[i] = o_val[l]; o_val[l] = fv;
              const double dv = o_bulk[i]; o_bulk[i] = o_bulk[l]; o_bulk[l] = dv;
            }
          }
        }
        __syncthreads();
      }
    }
  }
  __shared__ double incl[kKmppBlock];
  __shared__ uint32_t best;
  // inclusive exact BULK prefix of block bi into incl[] (Hillis-Steele; any order is exact)
  auto scan_block = [&](uint32_t bi) {
    const uint32_t s = bi * kKmppBlock + tid;
    incl[tid] = s < N ? bulk_of(dist_at(s)) : 0.0;
    __syncthreads();
    for (int o = 1; o < kKmppBlock; o <<= 1) {
      const double t = tid >= (uint32_t)o ? incl[tid - o] : 0.0;
      __syncthreads();
      incl[tid] += t;
      __syncthreads();
    }
  };
  // m0 = min { m in [0, N] : (Bulk(m) - c1) + c2 >= cs }  (N when there is none); Bulk(m) = the exact sum of the bulk
  // distances of the rows below m.  Block-uniform result.
  auto first_m = [&](double c1, double c2) -> uint32_t {
    if (tid == 0) best = 0xFFFFFFFFu;
    __syncthreads();
    if ((0.0 - c1) + c2 >= cs) return 0u;                          // Bulk(0) = 0
    // smallest block whose END prefix qualifies: the prefixes do not decrease (distances >= 0; a NaN has sent the step
    // to the host), so two rounds of 256 probes find it: every stride-th block, then the blocks in between
    const uint32_t stride = (nb + kKmppBlock - 1) / kKmppBlock;   // >= 1
    {
      const uint32_t probe = (tid + 1) * stride - 1;              // last block of my range
      const uint32_t pb = probe < nb ? probe : nb - 1;
      if (tid * stride < nb && (bpre(pb + 1) - c1) + c2 >= cs) atomicMin(&best, tid);
    }
    __syncthreads();
    const uint32_t range = best;
    __syncthreads();
    if (tid == 0) best = 0xFFFFFFFFu;
    __syncthreads();
    if (range != 0xFFFFFFFFu) {
      for (uint32_t bi = range * stride + tid; bi < nb && bi < (range + 1) * stride; bi += kKmppBlock)
        if ((bpre(bi + 1) - c1) + c2 >= cs) { atomicMin(&best, bi); break; }
    }
    __syncthreads();
    const uint32_t bi = best;
    __syncthreads();
    if (bi == 0xFFFFFFFFu) return N;
    scan_block(bi);
    if (tid == 0) best = 0xFFFFFFFFu;
    __syncthreads();
    const uint32_t m = bi * kKmppBlock + tid + 1;                  // Bulk(m) = bpre(bi) + incl[tid]
    if (m <= N && ((bpre(bi) + incl[tid]) - c1) + c2 >= cs) atomicMin(&best, m);
    __syncthreads();
    const uint32_t r = best;
    __syncthreads();
    return r == 0xFFFFFFFFu ? N : r;
  };
  // ---- the host's walk (kmcuda.cc:300-326) over the listed values: which way, which residue, which stretch ----
  // what thread 0 leaves for everybody: mode 0 = j is known (w_j), 1 = forward search first_m(0, w_r) in a stretch
  // whose residue (as of cs's binade) is w_r, 2 = backward search first_m(w_c1, w_r) -> j = max(2, m0 - 1), 3 = the host's turn
  __shared__ uint32_t w_mode, w_j;
  __shared__ double w_r, w_c1;
  double bulk_ca = 0.0;
  float dca_f = 0.f;
  if (ca >= 100u) {   // Bulk(ca), exact (block-uniform)
    const uint32_t bi = ca / kKmppBlock, rr = ca % kKmppBlock;
    if (bi >= nb) bulk_ca = bpre(nb);
    else {
      scan_block(bi);
      bulk_ca = bpre(bi) + (rr ? incl[rr - 1] : 0.0);
    }
    __syncthreads();
    dca_f = ca < N ? dist_at(ca) : 0.f;
  }
  if (tid == 0) {
    uint32_t mode = 1, jfix = 0;
    double r = 0.0, c1 = 0.0;
    uint32_t i = 0;
    bool forward = true;
    if (ca >= 100u) {
      for (; i < nout && o_idx[i] < ca; i++) {      // the sum over the rows below ca, rounded where the host's is
        r = kmpp_settle(r, o_bulk[i]);
        const double sb = o_bulk[i] + r;
        r = (sb + (double)o_val[i]) - o_bulk[i];
      }
      r = kmpp_settle(r, bulk_ca);
      forward = (bulk_ca + r) < cs;
    }
    if (forward) {
      // for (j = start; j < N && sum < cs; j++) sum += d[j]: j = the first m >= start with S(m) >= cs
      if (ca < 100u && 0.0 >= cs) { mode = 0; jfix = 0; }
      else {
        bool found = false;
        for (; i < nout; i++) {
          const double rs = kmpp_settle(r, o_bulk[i]);
          const double sb = o_bulk[i] + rs;         // S(p): every row below the listed row p added
          if (sb >= cs) {                           // reached inside the bulk stretch in front of p
            mode = 1;
            found = true;
            break;
          }
          const double s2 = sb + (double)o_val[i];
          r = s2 - o_bulk[i];
          if (s2 >= cs) { mode = 0; jfix = o_idx[i] + 1u; found = true; break; }
        }
        if (!found) {
          const double rs = kmpp_settle(r, base[S]);
          if (base[S] + rs >= cs) mode = 1;
          else { mode = 0; jfix = N; }
        }
      }
    } else {
      // for (j = ca; j > 1 && sum >= cs; j--) sum -= d[j]; j++  -- going down the grid only gets finer: the listed
      // values are the only roundings.  T(j) = (Bulk(j + 1) - bulk part of d[ca]) + r before d[j] is subtracted.
      c1 = bulk_of(dca_f);
      mode = 2;
      // the listed rows <= ca, downwards
      uint32_t t = i;
      while (t < nout && o_idx[t] <= ca) t++;
      while (t > 0) {
        t--;
        const uint32_t p = o_idx[t];
        const double tlow = (o_bulk[t] - c1) + r;   // T(p): Bulk(p + 1) = Bulk(p), p being listed
        if (tlow < cs || p <= 1u) break;            // the loop ends in the stretch above p (or at its j > 1 test)
        const double tnew = tlow - (double)o_val[t];   // d[p] subtracted: T(p - 1), rounded as the host's subtraction
        if (tnew < cs) { mode = 0; jfix = p; break; }  // the loop ends at j = p - 1 (>= 1), then j++
        r = tnew - (o_bulk[t] - c1);
      }
    }
    if (mode == 1u) {
      // Inside the stretch the sum may enter new binades (its residue losing a bit each time) before it reaches cs.
      // Every sum >= cs has been through all of them up to cs's own binade, every sum of a lower binade is < cs: the
      // first row at which the sum reaches cs is the first at which Bulk + (the residue as of cs's binade) does --
      // unless cs IS a power of two (a sum rounded up onto it from below would be taken for reaching it): the host's turn.
      const unsigned long long cb = (unsigned long long)__double_as_longlong(cs);
      if ((cb & 0xFFFFFFFFFFFFFull) == 0ull) mode = 3;
      else {
        for (int guard = 0; guard < 80 && r != 0.0; guard++) {
          const int lb = kmpp_lowbit(r);
          if (lb >= kmpp_ilogb(cs) - 52) break;
          const double C = ldexp(1.5, 52 + lb + 1);
          const double t = r + C;
          r = t - C;
        }
      }
    }
    w_mode = mode; w_j = jfix; w_r = r; w_c1 = c1;
  }
  __syncthreads();
  if (w_mode == 3u) {
    if (tid == 0) fail_all();
    return;
  }
  uint32_t j;
  if (w_mode == 0u) j = w_j;
  else if (w_mode == 1u) j = first_m(0.0, w_r);
  else {
    const uint32_t m0 = first_m(w_c1, w_r);
    const uint32_t mp = m0 == 0u ? 0u : min(m0 - 1u, ca + 1u);
    j = max(2u, mp);
  }
  if (tid == 0) {
    out->chosen = j;
    for (uint32_t i = 0; i < S; i++) *sh.s[i].outl_count = 0u;   // consumed: the next step lists afresh
  }
  if (j == 0u || j > N) {   // (the reference reports an internal bug here: so will the host)
    if (tid == 0) fail_all();
    return;
  }
  // the seed's row, from its owner into every shard's replica
  const uint32_t o = shard_of_block((j - 1u) / kKmppBlock);
  const float *src = sh.s[o].samples + (size_t)(j - 1u - sh.s[o].offset) * D;
  for (uint32_t f = tid; f < D; f += kKmppBlock) {
    const float v = src[f];
    for (uint32_t i = 0; i < S; i++) sh.s[i].centroids[(size_t)step * D + f] = v;
  }
}

// Sample weights (kmamd_kmeans_weighted): the chooser draws a row with probability proportional to w * (its distance
// term) -- one fp32 product, rounded to nearest, kept in a buffer of its own (dists[] stays the plain minimum the next
// step compares with).  The statistics, the prefix sums, the chooser and the host's restatement read that buffer where
// they read dists[] without weights; nothing else changes.
__global__ __launch_bounds__(256) void kmpp_weigh_kernel(const float *__restrict__ dists,
                                                         const float *__restrict__ weights, uint32_t N,
                                                         float *__restrict__ terms, const uint32_t *__restrict__ fail) {
  if (fail && *fail) return;   // (as the step: the terms stay as the undecided step left them)
  for (uint32_t s = blockIdx.x * 256u + threadIdx.x; s < N; s += gridDim.x * 256u) terms[s] = __fmul_rn(weights[s], dists[s]);
}
hipError_t launch_kmpp_weigh(const float *dists, const float *weights, uint32_t N, float *terms, const uint32_t *fail,
                             hipStream_t st) {
  const uint32_t nb = (N + 255u) / 256u;
  hipLaunchKernelGGL(kmpp_weigh_kernel, dim3(nb < 4096u ? (nb ? nb : 1u) : 4096u), dim3(256), 0, st, dists, weights, N,
                     terms, fail);
  return hipGetLastError();
}

// bpre: nb local prefixes, then nchunks + 1 carries, then (16-byte aligned) the nchunks chunk records
static hipError_t launch_kmpp_reduce(const void *block_stats, uint32_t nb, double *bpre, void *totals,
                                     const uint32_t *fail, hipStream_t st) {
  const uint32_t nchunks = (nb + 1023u) / 1024u;
  if (nchunks > 1024u) return hipErrorInvalidValue;   // (N > 2^28 rows: kmpp_supported() keeps such jobs on the host chooser)
  double *carry = bpre + nb;
  KmppChunk *aux = reinterpret_cast<KmppChunk *>(bpre + (((size_t)nb + nchunks + 1 + 1) & ~(size_t)1));
  hipLaunchKernelGGL(kmpp_reduce_a_kernel, dim3(nchunks), dim3(1024), 0, st,
                     reinterpret_cast<const KmppBlockStat *>(block_stats), nb, bpre, aux, fail);
  hipLaunchKernelGGL(kmpp_reduce_b_kernel, dim3(1), dim3(1024), 0, st, aux, nchunks, carry,
                     reinterpret_cast<KmppTotals *>(totals), fail);
  return hipGetLastError();
}

// the exact chains of a step: every row (with the block statistics), or the rows of a list
static hipError_t launch_kmpp_chains(int metric, uint32_t grid, const float *samples, uint32_t N, uint32_t D,
                                     const float *centroid, uint32_t cc, float *dists, void *block_stats,
                                     const uint32_t *list, const uint32_t *nlist, const uint32_t *fail, hipStream_t st) {
  return with_metric(metric, [&](auto M) {
    hipLaunchKernelGGL((kmpp_step2_kernel<M()>), dim3(grid), dim3(kKmppBlock), 0, st, samples, N, D, centroid, cc, dists,
                       reinterpret_cast<KmppBlockStat *>(block_stats), list, nlist, fail);
    return hipGetLastError();
  });
}

hipError_t launch_kmpp_step2(int metric, const float *samples, uint32_t N, uint32_t D, const float *centroid,
                             uint32_t cc, float *dists, void *block_stats, double *bpre, void *totals_host,
                             const uint32_t *fail, const KmppOutlierBuf &out, hipStream_t st, const float *weights,
                             float *terms) {
  const uint32_t nb = (N + kKmppBlock - 1) / kKmppBlock;
  const hipError_t e = launch_kmpp_chains(metric, nb, samples, N, D, centroid, cc, dists, block_stats, nullptr, nullptr, fail, st);
  if (e != hipSuccess) return e;
  if (weights && launch_kmpp_weigh(dists, weights, N, terms, fail, st) != hipSuccess) return hipGetLastError();
  hipLaunchKernelGGL(kmpp_stats_kernel, dim3((nb + 3) / 4 < 2048u ? (nb + 3) / 4 : 2048u), dim3(256), 0, st,
                     weights ? terms : dists, N,
                     reinterpret_cast<KmppBlockStat *>(block_stats), (uint32_t *)nullptr, fail, out.ecut,
                     reinterpret_cast<KmppOutlier *>(out.outl), out.outl_count);
  return launch_kmpp_reduce(block_stats, nb, bpre, totals_host, fail, st);
}

// The centred byte copy of the rows for the filtered steps: mu = column means of the first <= 65536 rows (any
// vector is valid; a central one keeps the norms in the error bound small).  part: 64 x D doubles of scratch;
// xs8: N x DP bytes (DP = D rounded up to 128); meta: N x 4 floats; stats: 4 words ([1] the step's survivor count,
// [2..3] the run's).
hipError_t launch_kmpp_cache(const float *samples, uint32_t N, uint32_t D, uint32_t DP, double *part, float *mu,
                             void *xs8, float *meta, uint32_t *stats, hipStream_t st) {
  const uint32_t rows = N < 65536u ? N : 65536u;
  hipError_t e = hipMemsetAsync(stats, 0, 4 * sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kmpp_colsum_kernel, dim3(64), dim3(256), 0, st, samples, rows, D, part);
  hipLaunchKernelGGL(kmpp_mean_kernel, dim3((DP + 255) / 256), dim3(256), 0, st, part, 64u, rows, D, DP, mu);
  hipLaunchKernelGGL(kmpp_cache_kernel, dim3(wave_row_grid(N)), dim3(256), 0, st, samples, N, D, DP, mu,
                     reinterpret_cast<signed char *>(xs8), reinterpret_cast<f32x4_kp *>(meta));
  return hipGetLastError();
}

// One filtered step (cc >= 2; the first step has nothing to compare with: launch_kmpp_step2): survivors of the
// bound -> exact chains -> block statistics -> totals, as launch_kmpp_step2 leaves them.
hipError_t launch_kmpp_step_filtered(int metric, const float *samples, uint32_t N, uint32_t D, uint32_t DP,
                                     const void *xs8, const float *meta, const float *mu, uint32_t *stats,
                                     uint32_t *list, const float *centroid, uint32_t cc, float *dists,
                                     void *block_stats, double *bpre, void *totals_host, const uint32_t *fail,
                                     const KmppOutlierBuf &out, hipStream_t st, const float *weights, float *terms) {
  const uint32_t nb = (N + kKmppBlock - 1) / kKmppBlock;
  const float eps = (float)(1.02 * ((double)D + 12.0) * 5.9604644775390625e-8);   // as the k-NN filter
  const uint32_t fgrid = (N + 127) / 128 < 1024u ? (N + 127) / 128 : 1024u;   // 16 waves per CU; one list atomic per wave
  auto filter = [&](auto P) {   // (PPL = DP / 128 where the kernel has it unrolled, 0 = any DP)
    return with_metric(metric, [&](auto M) {
      hipLaunchKernelGGL((kmpp_filter_kernel<P(), M()>), dim3(fgrid), dim3(256), (size_t)DP * 4, st,
                         reinterpret_cast<const signed char *>(xs8), reinterpret_cast<const f32x4_kp *>(meta), mu, centroid,
                         N, D, DP, eps, dists, list, stats + 1, fail);
      return hipGetLastError();
    });
  };
  using std::integral_constant;
  hipError_t e;
  switch (DP / 128) {
    case 1: e = filter(integral_constant<int, 1>{}); break;
    case 2: e = filter(integral_constant<int, 2>{}); break;
    case 3: e = filter(integral_constant<int, 3>{}); break;
    case 4: e = filter(integral_constant<int, 4>{}); break;
    default: e = filter(integral_constant<int, 0>{}); break;
  }
  if (e != hipSuccess) return e;
  e = launch_kmpp_chains(metric, nb < 1024u ? nb : 1024u, samples, N, D, centroid, cc, dists, nullptr, list, stats + 1, fail, st);
  if (e != hipSuccess) return e;
  if (weights && launch_kmpp_weigh(dists, weights, N, terms, fail, st) != hipSuccess) return hipGetLastError();
  hipLaunchKernelGGL(kmpp_stats_kernel, dim3((nb + 3) / 4 < 2048u ? (nb + 3) / 4 : 2048u), dim3(256), 0, st,
                     weights ? terms : dists, N,
                     reinterpret_cast<KmppBlockStat *>(block_stats), stats + 1, fail, out.ecut,
                     reinterpret_cast<KmppOutlier *>(out.outl), out.outl_count);
  return launch_kmpp_reduce(block_stats, nb, bpre, totals_host, fail, st);
}

hipError_t launch_kmpp_choose(const KmppShardPtrs *shards, uint32_t nshards, uint32_t N, double choice, uint32_t log2n,
                              uint32_t step, uint32_t D, hipStream_t st) {
  if (nshards == 0 || nshards > (uint32_t)kKmppMaxShards) return hipErrorInvalidValue;
  KmppShards sh;
  sh.n = nshards;
  for (uint32_t i = 0; i < nshards; i++) {
    sh.s[i].dists = shards[i].dists;
    sh.s[i].bpre = shards[i].bpre;
    sh.s[i].totals = reinterpret_cast<const KmppTotals *>(shards[i].totals);
    sh.s[i].samples = shards[i].samples;
    sh.s[i].centroids = shards[i].centroids;
    sh.s[i].fail = shards[i].fail;
    sh.s[i].ecut = shards[i].out.ecut;
    sh.s[i].outl = reinterpret_cast<const KmppOutlier *>(shards[i].out.outl);
    sh.s[i].outl_count = shards[i].out.outl_count;
    sh.s[i].offset = shards[i].offset;
    sh.s[i].length = shards[i].length;
    if (i && shards[i].offset % kKmppBlock != 0) return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(kmpp_choose_kernel, dim3(1), dim3(kKmppBlock), 0, st, sh, N, choice, log2n, step, D,
                     reinterpret_cast<KmppTotals *>(shards[0].totals));
  return hipGetLastError();
}

size_t kmpp_outlier_bytes() { return (size_t)kKmppOutCap * sizeof(KmppOutlier); }
size_t kmpp_totals_bytes() { return sizeof(KmppTotals); }
size_t kmpp_block_stat_bytes(uint32_t N) { return (size_t)((N + kKmppBlock - 1) / kKmppBlock) * sizeof(KmppBlockStat); }
size_t kmpp_blocks(uint32_t N) { return (N + kKmppBlock - 1) / kKmppBlock; }
// doubles the caller allocates for bpre (local prefixes + carries + chunk records)
size_t kmpp_prefix_doubles(uint32_t N) {
  const size_t nb = kmpp_blocks(N), nchunks = (nb + 1023) / 1024;
  return nb + nchunks + 3 + nchunks * (sizeof(KmppChunk) / sizeof(double));
}

// ---------------------------------------------------------------------------------------
// AFK-MC2 seeding (reference: kmeans.cu:69-212, host chain kmcuda.cc:337-396).
// The reference draws from cuRAND's XORWOW (curand_init(seed, thread, step), two curand_uniform per
// thread); cuRAND is not in the reference's tree and not on this box.  The generator as published --
// Marsaglia's xorwow + a Weyl sequence, output d + x[4], and the jumps (subsequence = thread: 2^67
// draws; offset = step) -- is rocRAND's xorwow_engine, whose lines and skip matrices are the
// recurrence's own.  What the two libraries do NOT share is the SEED SCRAMBLING: curand_kernel.h
// (_curand_init_scratch, as the builder knows it: not verifiable offline) salts the seed's halves
// with 0xaad26b49 / 0xf7dcefdd and multiplies by 1099087573 / 2591861531, rocrand_xorwow.h uses
// 0x2c7f967f / 0xa03697cb and 1228688033 / 2073658381.  The only anchors the reference holds for
// this init are four iteration counts (test.py:248-289 and :499-509: 4 / 4 / 4 and, fp16, 4): rocRAND's
// seeding meets all four, the quoted cuRAND constants three (the half2 run takes 5) -- with an
// arbitrary stream a run has 4 iterations with probability ~0.6, so neither outcome proves a stream.
// The DEFAULT is the seeding that meets every pin the reference holds (rocRAND's);
// KMCUDA_AMD_AFKMC2_SEEDING=curand selects the other.  cuRAND's documented uint -> (0, 1] mapping
// x * 2^-32 + 2^-33.  Both flavours equal the oracle's restatement draw for draw, and the
// restatement's generator / jumps equal rocRAND's host generator (tests/test_gpu_afkmc2_rng.py);
// nothing stronger is claimed: parity unpinned.
// ---------------------------------------------------------------------------------------
struct SeededXorwow : rocrand_device::xorwow_engine {
  __device__ SeededXorwow(unsigned long long seed, unsigned long long subsequence, unsigned long long offset, bool curand)
      : rocrand_device::xorwow_engine(0ull, 0ull, 0ull) {   // (no jumps; the state is set below)
    const unsigned int s0 = static_cast<unsigned int>(seed) ^ (curand ? 0xaad26b49u : 0x2c7f967fu);
    const unsigned int s1 = static_cast<unsigned int>(seed >> 32) ^ (curand ? 0xf7dcefddu : 0xa03697cbu);
    const unsigned int t0 = (curand ? 1099087573u : 1228688033u) * s0, t1 = (curand ? 2591861531u : 2073658381u) * s1;
    m_state.d = 6615241u + t1 + t0;
    m_state.x[0] = 123456789u + t0;
    m_state.x[1] = 362436069u ^ t0;
    m_state.x[2] = 521288629u + t1;
    m_state.x[3] = 88675123u ^ t1;
    m_state.x[4] = 5783321u + t0;
    discard_subsequence(subsequence);
    discard(offset);
  }
};
bool afk_curand_seeding() {   // (read per call: tests switch it)
  const char *v = getenv("KMCUDA_AMD_AFKMC2_SEEDING");
  return v && (v[0] == 'c' || v[0] == 'C');
}

// the first n draws of the stream (seed, subsequence = thread, offset): the tests' window on the device generator
__global__ void afk_draws_kernel(unsigned long long seed, unsigned long long offset, uint32_t threads, uint32_t n,
                                 uint32_t *__restrict__ out, bool curand) {
  const uint32_t ti = blockIdx.x * blockDim.x + threadIdx.x;
  if (ti >= threads) return;
  SeededXorwow eng(seed, ti, offset, curand);
  for (uint32_t i = 0; i < n; i++) out[(size_t)ti * n + i] = eng.next();
}
hipError_t launch_afk_draws(unsigned long long seed, unsigned long long offset, uint32_t threads, uint32_t n, uint32_t *out,
                            hipStream_t st) {
  if (threads == 0 || n == 0) return hipSuccess;
  hipLaunchKernelGGL(afk_draws_kernel, dim3((threads + 255) / 256), dim3(256), 0, st, seed, offset, threads, n, out,
                     afk_curand_seeding());
  return hipGetLastError();
}

template <int METRIC>
__global__ void afk_qdist_kernel(const float *__restrict__ samples, uint32_t N, uint32_t D,
                                 const float *__restrict__ c1, float *__restrict__ dists) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= N) return;
  const float d = distance_vv<METRIC>(samples + (size_t)s * D, c1, D);   // kmeans.cu:88-90 (no NaN test here)
  dists[s] = d * d;
}

__global__ void afk_q_kernel(float *__restrict__ q, uint32_t N, float dsum) {   // kmeans.cu:98-109
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= N) return;
  q[s] = 1 / (2.f * N) + q[s] / (2 * dsum);
}

__device__ __forceinline__ float afk_uniform(unsigned int x) { return fmaf((float)x, 2.3283064e-10f, 2.3283064e-10f / 2.0f); }

// one thread per candidate: two uniforms, then the first index whose Kahan prefix sum of q reaches the
// first one (kmeans.cu:111-164; a thread whose sum never gets there leaves its choice as it was)
__global__ void afk_random_step_kernel(uint32_t m, unsigned long long seed, unsigned long long seq,
                                       const float *__restrict__ q, uint32_t N, uint32_t *__restrict__ choices,
                                       float *__restrict__ rand_a, bool curand) {
  const uint32_t ti = blockIdx.x * blockDim.x + threadIdx.x;
  if (ti >= m) return;
  SeededXorwow eng(seed, ti, seq, curand);
  const float part = afk_uniform(eng.next());
  rand_a[ti] = afk_uniform(eng.next());
  float accum = 0.f, corr = 0.f;
  uint32_t i = 0;
  for (; i < N && accum < part; i++) {   // Kahan summation with inverted c
    const float y = corr + q[i];
    const float t = accum + y;
    corr = y - (t - accum);
    accum = t;
  }
  if (accum >= part) choices[ti] = i - 1;
}

template <int METRIC>
__global__ void afk_min_dist_kernel(uint32_t m, uint32_t k, const float *__restrict__ samples, uint32_t D,
                                    const uint32_t *__restrict__ choices, const float *__restrict__ centroids,
                                    float *__restrict__ min_dists) {   // kmeans.cu:166-183
  const uint32_t chi = blockIdx.x * blockDim.x + threadIdx.x;
  if (chi >= m) return;
  const float *x = samples + (size_t)choices[chi] * D;
  float min_dist = 3.402823466e+38f;
  for (uint32_t c = 0; c < k; c++) {
    const float dist = distance_vv<METRIC>(x, centroids + (size_t)c * D, D);
    if (dist < min_dist) min_dist = dist;
  }
  min_dists[chi] = min_dist * min_dist;
}

hipError_t launch_afk_qdist(int metric, const float *samples, uint32_t N, uint32_t D, const float *c1, float *dists,
                            hipStream_t st) {
  const dim3 grid((N + 127) / 128), block(128);
  return with_metric(metric, [&](auto M) {
    hipLaunchKernelGGL((afk_qdist_kernel<M()>), grid, block, 0, st, samples, N, D, c1, dists);
    return hipGetLastError();
  });
}
hipError_t launch_afk_q(float *q, uint32_t N, float dsum, hipStream_t st) {
  hipLaunchKernelGGL(afk_q_kernel, dim3((N + 255) / 256), dim3(256), 0, st, q, N, dsum);
  return hipGetLastError();
}
hipError_t launch_afk_random_step(uint32_t m, uint64_t seed, uint64_t seq, const float *q, uint32_t N,
                                  uint32_t *choices, float *rand_a, hipStream_t st) {
  hipLaunchKernelGGL(afk_random_step_kernel, dim3((m + 63) / 64), dim3(64), 0, st, m, (unsigned long long)seed,
                     (unsigned long long)seq, q, N, choices, rand_a, afk_curand_seeding());
  return hipGetLastError();
}
hipError_t launch_afk_min_dist(int metric, uint32_t m, uint32_t k, const float *samples, uint32_t D,
                               const uint32_t *choices, const float *centroids, float *min_dists, hipStream_t st) {
  const dim3 grid((m + 63) / 64), block(64);
  return with_metric(metric, [&](auto M) {
    hipLaunchKernelGGL((afk_min_dist_kernel<M()>), grid, block, 0, st, m, k, samples, D, choices, centroids, min_dists);
    return hipGetLastError();
  });
}

// LIBM_ACOS (kmamd_kmeans_assign's distance pass under KMCUDA_AMD_ASSIGN_DIST=member): the angle by acosf_fdlibm,
// the C library's acosf restated (exact.hpp), instead of the device library's; the chain is the same
template <int METRIC, bool LIBM_ACOS>
__global__ void member_distances_kernel(const float *__restrict__ samples, uint32_t N, uint32_t D,
                                        const float *__restrict__ centroids, const uint32_t *__restrict__ assignments,
                                        uint32_t K, float *__restrict__ dists) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= N) return;
  const uint32_t a = assignments[s];
  if (METRIC == 1 && LIBM_ACOS)
    dists[s] = a < K ? angular_from_prod_libm(chain_vv<1>(samples + (size_t)s * D, centroids + (size_t)a * D, D)) : NAN;
  else
    dists[s] = a < K ? distance_vv<METRIC>(samples + (size_t)s * D, centroids + (size_t)a * D, D) : NAN;
}

hipError_t launch_member_distances(int metric, const float *samples, uint32_t N, uint32_t D,
                                   const float *centroids, const uint32_t *assignments, uint32_t K,
                                   float *dists, hipStream_t st, bool libm_acos) {
  const dim3 grid((N + 127) / 128), block(128);
  if (metric == 0)
    hipLaunchKernelGGL((member_distances_kernel<0, false>), grid, block, 0, st, samples, N, D, centroids, assignments,
                       K, dists);
  else if (libm_acos)
    hipLaunchKernelGGL((member_distances_kernel<1, true>), grid, block, 0, st, samples, N, D, centroids, assignments,
                       K, dists);
  else
    hipLaunchKernelGGL((member_distances_kernel<1, false>), grid, block, 0, st, samples, N, D, centroids, assignments,
                       K, dists);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// fp16x2 boundary (reference: fp_abstraction.h:100-182, kmcuda.h:107-108): the public buffers
// hold IEEE halves (two per 32-bit "feature").  This implementation computes the fp16 path as
// "the fp32 arithmetic applied to the half values" -- halves are widened exactly on the way in,
// centroids are rounded to half (RN) after every update, exactly where the reference stores them
// as half2 -- instead of accumulating in half2 like the reference (tolerance).
// ---------------------------------------------------------------------------------------
__global__ void half_to_float_kernel(const __half *__restrict__ src, size_t n, float *__restrict__ dst) {
  // (strided from a bounded grid: n / 8 threads pass 2^32 for buffers beyond 32 G halves -- kernels.hpp: wave_row_grid)
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 8; i < n; i += (size_t)gridDim.x * blockDim.x * 8) {
    if (i + 8 <= n) {
      const uint4 raw = *reinterpret_cast<const uint4 *>(src + i);
      const __half2 *h2 = reinterpret_cast<const __half2 *>(&raw);
      float4 lo, hi;
      float2 a = __half22float2(h2[0]), b = __half22float2(h2[1]), c = __half22float2(h2[2]), d = __half22float2(h2[3]);
      lo.x = a.x; lo.y = a.y; lo.z = b.x; lo.w = b.y;
      hi.x = c.x; hi.y = c.y; hi.z = d.x; hi.w = d.y;
      *reinterpret_cast<float4 *>(dst + i) = lo;
      *reinterpret_cast<float4 *>(dst + i + 4) = hi;
    } else {
      for (size_t j = i; j < n; j++) dst[j] = __half2float(src[j]);
    }
  }
}

__global__ void float_to_half_kernel(const float *__restrict__ src, size_t n, __half *__restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = __float2half_rn(src[i]);
}

// v = float(half_rn(v)) in place: the value a half2 centroid buffer would hold
__global__ void quantize_half_kernel(float *__restrict__ v, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = __half2float(__float2half_rn(v[i]));
}

hipError_t launch_half_to_float(const void *src, size_t n, float *dst, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const size_t blocks = ((n + 7) / 8 + 255) / 256;
  hipLaunchKernelGGL(half_to_float_kernel, dim3((uint32_t)(blocks < (1u << 22) ? blocks : (1u << 22))), dim3(256), 0, st,
                     reinterpret_cast<const __half *>(src), n, dst);
  return hipGetLastError();
}

hipError_t launch_float_to_half(const float *src, size_t n, void *dst, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(float_to_half_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, src, n,
                     reinterpret_cast<__half *>(dst));
  return hipGetLastError();
}

hipError_t launch_quantize_half(float *v, size_t n, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(quantize_half_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, v, n);
  return hipGetLastError();
}

}  // namespace kmx
