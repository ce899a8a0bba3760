// seed_par.hip -- the sampling kernels of k-means|| seeding (kmamd_kmeans_seed_parallel, seed_par_job.cpp; DESIGN.md
// 6.3).  The distance work of a round runs on the engine's assignment pass and the distance pass of assign_dist.hip;
// what is here streams 4-8 bytes per row:
//   term update   t <- min(t, d) and the fp64 sum of the terms of every 256 rows (a fixed tree)
//   phi           the sum of those block sums (a fixed order)
//   draw          row s is drawn iff U(seed, r, s) * phi < (double)l * (double)t[s]; per-block counts
//   prefix        exclusive prefix of the block counts, two levels of 1024
//   fill          the drawn row ids in ascending row order, and their rows into the candidate matrix
//   weights       counts[j] = the rows assigned to candidate j (integer atomics: any order, the same counts)
// A block is 256 consecutive rows everywhere; grids are bounded and stride over the blocks (N < 2^32 rows is up to 2^24
// blocks; a grid of one thread per row would pass 2^32 threads, DESIGN_LOG 12.1).  No floating-point atomics.
#include <math.h>

#include "kernels.hpp"

namespace kmx {

namespace {

constexpr int kSpBlock = 256;       // rows per block: the granularity of the block sums, counts and prefixes
constexpr uint32_t kSpGrid = 2048;  // blocks per launch at most (256 CUs x 8); the rest by striding
constexpr int kSpScan = 1024;       // block counts per first-level scan block

__host__ __device__ inline uint32_t sp_blocks(uint32_t N) { return (uint32_t)(((uint64_t)N + kSpBlock - 1) / kSpBlock); }

// h(seed, r, s): the splitmix64 finaliser of ((r << 32) | s) + (seed + 1) * 0x9E3779B97F4A7C15
__device__ inline uint64_t sp_hash(uint64_t key, uint32_t s) {
  uint64_t z = key + s;   // key = (r << 32) + (seed + 1) * golden: the low word of (r << 32 | s) is s alone
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

// a term that is NaN or inf counts as 0 (and a term of 0 is never drawn: U * phi < 0 is false)
__device__ inline double sp_term(float t) { return (t - t == 0.f) ? (double)t : 0.0; }

__device__ inline bool sp_drawn(uint64_t key, uint32_t s, double phi, double ell, float t) {
  const double u = (double)(sp_hash(key, s) >> 11) * 0x1p-53;   // exact: 53 bits
  return u * phi < ell * sp_term(t);
}

// the sum of a block's 256 doubles in a fixed tree: xor-butterfly inside each wave, then the four waves in order
__device__ inline double sp_block_sum(double v, double *lds4) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  const double total = ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
  __syncthreads();
  return total;
}

// t[s] <- d[s] where d[s] < t[s] (a NaN d leaves t as it is).  first: t starts at +inf, and a row whose first feature
// is NaN gets the term 0 for good.  bsum[b] = the fp64 sum of the block's terms.
__global__ __launch_bounds__(kSpBlock) void sp_update_kernel(float *__restrict__ t, const float *__restrict__ d,
                                                             uint32_t N, const float *__restrict__ rows, uint32_t D,
                                                             double *__restrict__ bsum) {
  __shared__ double lds4[4];
  const uint32_t nb = sp_blocks(N);
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint64_t s = (uint64_t)b * kSpBlock + threadIdx.x;
    double term = 0.0;
    if (s < N) {
      float cur = rows ? INFINITY : t[s];
      const float dv = d[s];
      if (dv < cur) cur = dv;
      if (rows) {
        const float x0 = rows[s * D];
        if (x0 != x0) cur = 0.f;
      }
      t[s] = cur;
      term = sp_term(cur);
    }
    const double total = sp_block_sum(term, lds4);
    if (threadIdx.x == 0) bsum[b] = total;
  }
}

// *phi = the sum of bsum[0 .. nb): thread i adds bsum[i], bsum[i + 1024], ... in that order, then a fixed tree
__global__ __launch_bounds__(kSpScan) void sp_phi_kernel(const double *__restrict__ bsum, uint32_t nb,
                                                         double *__restrict__ phi) {
  __shared__ double part[kSpScan];
  double v = 0.0;
  for (uint32_t i = threadIdx.x; i < nb; i += kSpScan) v += bsum[i];
  part[threadIdx.x] = v;
  __syncthreads();
  for (int half = kSpScan / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) *phi = part[0];
}

// bcount[b] = the number of drawn rows of block b
__global__ __launch_bounds__(kSpBlock) void sp_draw_kernel(const float *__restrict__ t, uint32_t N, uint64_t key,
                                                           const double *__restrict__ phi, double ell,
                                                           uint32_t *__restrict__ bcount) {
  __shared__ uint32_t wcount[4];
  const uint32_t nb = sp_blocks(N);
  const double p = *phi;
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint64_t s = (uint64_t)b * kSpBlock + threadIdx.x;
    const bool drawn = s < N && sp_drawn(key, (uint32_t)s, p, ell, t[s]);
    const unsigned long long mask = __ballot(drawn);
    if ((threadIdx.x & 63) == 0) wcount[threadIdx.x >> 6] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) bcount[b] = wcount[0] + wcount[1] + wcount[2] + wcount[3];
    __syncthreads();
  }
}

// exclusive prefix of 1024 values held one per thread; *total = their sum
__device__ inline uint32_t sp_scan_1024(uint32_t v, uint32_t *lds, uint32_t *total) {
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int off = 1; off < kSpScan; off <<= 1) {   // Hillis-Steele, inclusive
    const uint32_t add = (int)threadIdx.x >= off ? lds[threadIdx.x - off] : 0u;
    __syncthreads();
    lds[threadIdx.x] += add;
    __syncthreads();
  }
  const uint32_t incl = lds[threadIdx.x];
  *total = lds[kSpScan - 1];
  __syncthreads();
  return incl - v;
}

// level 1: boff[i] = the exclusive prefix of bcount inside i's chunk of 1024 blocks, aux[c] = the chunk's total
__global__ __launch_bounds__(kSpScan) void sp_scan_a_kernel(const uint32_t *__restrict__ bcount, uint32_t nb,
                                                            uint32_t *__restrict__ boff, uint32_t *__restrict__ aux) {
  __shared__ uint32_t lds[kSpScan];
  const uint32_t nchunks = (nb + kSpScan - 1) / kSpScan;
  for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const uint32_t i = c * kSpScan + threadIdx.x;   // < 2^24 + 1024
    uint32_t total;
    const uint32_t ex = sp_scan_1024(i < nb ? bcount[i] : 0u, lds, &total);
    if (i < nb) boff[i] = ex;
    if (threadIdx.x == 0) aux[c] = total;
  }
}

// level 2 (one block): carry[c] = the exclusive prefix of aux, carry[nchunks] = the number of drawn rows.  nchunks <=
// 2^14: every thread owns up to 16 consecutive chunks.
__global__ __launch_bounds__(kSpScan) void sp_scan_b_kernel(const uint32_t *__restrict__ aux, uint32_t nchunks,
                                                            uint32_t *__restrict__ carry) {
  __shared__ uint32_t lds[kSpScan];
  const uint32_t per = (nchunks + kSpScan - 1) / kSpScan;
  const uint32_t lo = threadIdx.x * per, hi = lo + per < nchunks ? lo + per : nchunks;
  uint32_t mine = 0;
  for (uint32_t c = lo; c < hi; c++) mine += aux[c];
  uint32_t total;
  uint32_t run = sp_scan_1024(mine, lds, &total);
  for (uint32_t c = lo; c < hi; c++) {
    carry[c] = run;
    run += aux[c];
  }
  if (threadIdx.x == 0) carry[nchunks] = total;
}

// ids[boff + carry + rank] = s for the drawn rows of every block, in ascending row order, and their rows into the
// candidate matrix.  M bounds every write (it is carry[nchunks]).
__global__ __launch_bounds__(kSpBlock) void sp_fill_kernel(const float *__restrict__ t, uint32_t N, uint64_t key,
                                                           const double *__restrict__ phi, double ell,
                                                           const uint32_t *__restrict__ boff,
                                                           const uint32_t *__restrict__ carry, uint32_t M,
                                                           const float *__restrict__ rows32, uint32_t D,
                                                           uint32_t *__restrict__ ids, float *__restrict__ cand32) {
  __shared__ uint32_t wcount[4];
  __shared__ uint32_t picked[kSpBlock];
  const uint32_t nb = sp_blocks(N);
  const double p = *phi;
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint64_t s = (uint64_t)b * kSpBlock + threadIdx.x;
    const bool drawn = s < N && sp_drawn(key, (uint32_t)s, p, ell, t[s]);
    const unsigned long long mask = __ballot(drawn);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wcount[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; w++) rank += wcount[w];
    const uint32_t cnt = wcount[0] + wcount[1] + wcount[2] + wcount[3];
    const uint32_t base = boff[b] + carry[b / kSpScan];
    if (drawn) picked[rank] = (uint32_t)s;
    __syncthreads();
    for (uint32_t j = 0; j < cnt; j++) {
      const uint64_t pos = (uint64_t)base + j;
      if (pos >= M) break;   // (never: M is the prefix's own total)
      const uint64_t src = (uint64_t)picked[j] * D, dst = pos * D;
      if (threadIdx.x == 0) ids[pos] = picked[j];
      for (uint32_t f = threadIdx.x; f < D; f += kSpBlock) cand32[dst + f] = rows32[src + f];
    }
    __syncthreads();
  }
}

// counts[a] += 1 for every row whose assignment a is below M
__global__ __launch_bounds__(kSpBlock) void sp_weights_kernel(const uint32_t *__restrict__ asg, uint32_t N, uint32_t M,
                                                              uint32_t *__restrict__ counts) {
  const uint32_t nb = sp_blocks(N);
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint64_t s = (uint64_t)b * kSpBlock + threadIdx.x;
    if (s < N) {
      const uint32_t a = asg[s];
      if (a < M) atomicAdd(counts + a, 1u);
    }
  }
}

// out[j] = in[idx[j]], rows of floats and / or of halves: one block per row at a time
__global__ __launch_bounds__(kSpBlock) void sp_gather_kernel(const float *__restrict__ in32,
                                                             const uint16_t *__restrict__ in16,
                                                             const uint32_t *__restrict__ idx, uint32_t M, uint32_t D,
                                                             float *__restrict__ out32, uint16_t *__restrict__ out16) {
  for (uint32_t j = blockIdx.x; j < M; j += gridDim.x) {
    const uint64_t src = (uint64_t)idx[j] * D, dst = (uint64_t)j * D;
    for (uint32_t f = threadIdx.x; f < D; f += kSpBlock) {
      if (out32) out32[dst + f] = in32[src + f];
      if (out16) out16[dst + f] = in16[src + f];
    }
  }
}

// *best = min over the rows whose first feature is not NaN of ((s - start) mod N): the first such row at or
// cyclically after `start` (0xFFFFFFFFFFFFFFFF: there is none)
__global__ __launch_bounds__(kSpBlock) void sp_first_valid_kernel(const float *__restrict__ rows, uint32_t N,
                                                                  uint32_t D, uint32_t start,
                                                                  unsigned long long *__restrict__ best) {
  const uint32_t nb = sp_blocks(N);
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint64_t s = (uint64_t)b * kSpBlock + threadIdx.x;
    if (s < N) {
      const float x0 = rows[s * D];
      if (x0 == x0) atomicMin(best, (unsigned long long)(s >= start ? s - start : s + N - start));
    }
  }
}

inline uint32_t sp_grid(uint32_t blocks) { return blocks < kSpGrid ? (blocks ? blocks : 1u) : kSpGrid; }

}  // namespace

size_t seed_par_block_count(uint32_t N) { return sp_blocks(N); }
size_t seed_par_chunk_count(uint32_t N) { return (sp_blocks(N) + kSpScan - 1) / kSpScan; }

hipError_t launch_seed_par_update(float *t, const float *d, uint32_t N, const float *rows_first, uint32_t D,
                                  double *bsum, double *phi, hipStream_t st) {
  const uint32_t nb = sp_blocks(N);
  hipLaunchKernelGGL(sp_update_kernel, dim3(sp_grid(nb)), dim3(kSpBlock), 0, st, t, d, N, rows_first, D, bsum);
  hipLaunchKernelGGL(sp_phi_kernel, dim3(1), dim3(kSpScan), 0, st, bsum, nb, phi);
  return hipGetLastError();
}

hipError_t launch_seed_par_draw(const float *t, uint32_t N, uint32_t seed, uint32_t round, const double *phi,
                                float oversampling, uint32_t *bcount, uint32_t *boff, uint32_t *aux, uint32_t *carry,
                                hipStream_t st) {
  const uint32_t nb = sp_blocks(N), nchunks = (nb + kSpScan - 1) / kSpScan;
  const uint64_t key = ((uint64_t)round << 32) + ((uint64_t)seed + 1ull) * 0x9E3779B97F4A7C15ull;
  hipLaunchKernelGGL(sp_draw_kernel, dim3(sp_grid(nb)), dim3(kSpBlock), 0, st, t, N, key, phi, (double)oversampling,
                     bcount);
  hipLaunchKernelGGL(sp_scan_a_kernel, dim3(sp_grid(nchunks)), dim3(kSpScan), 0, st, bcount, nb, boff, aux);
  hipLaunchKernelGGL(sp_scan_b_kernel, dim3(1), dim3(kSpScan), 0, st, aux, nchunks, carry);
  return hipGetLastError();
}

hipError_t launch_seed_par_fill(const float *t, uint32_t N, uint32_t seed, uint32_t round, const double *phi,
                                float oversampling, const uint32_t *boff, const uint32_t *carry, uint32_t M,
                                const float *rows32, uint32_t D, uint32_t *ids, float *cand32, hipStream_t st) {
  const uint32_t nb = sp_blocks(N);
  const uint64_t key = ((uint64_t)round << 32) + ((uint64_t)seed + 1ull) * 0x9E3779B97F4A7C15ull;
  hipLaunchKernelGGL(sp_fill_kernel, dim3(sp_grid(nb)), dim3(kSpBlock), 0, st, t, N, key, phi, (double)oversampling,
                     boff, carry, M, rows32, D, ids, cand32);
  return hipGetLastError();
}

hipError_t launch_seed_par_weights(const uint32_t *assignments, uint32_t N, uint32_t M, uint32_t *counts,
                                   hipStream_t st) {
  hipLaunchKernelGGL(sp_weights_kernel, dim3(sp_grid(sp_blocks(N))), dim3(kSpBlock), 0, st, assignments, N, M, counts);
  return hipGetLastError();
}

hipError_t launch_seed_par_gather(const float *in32, const void *in16, const uint32_t *idx, uint32_t M, uint32_t D,
                                  float *out32, void *out16, hipStream_t st) {
  if (M == 0) return hipSuccess;
  hipLaunchKernelGGL(sp_gather_kernel, dim3(sp_grid(M)), dim3(kSpBlock), 0, st, in32,
                     static_cast<const uint16_t *>(in16), idx, M, D, out32, static_cast<uint16_t *>(out16));
  return hipGetLastError();
}

hipError_t launch_seed_par_first_valid(const float *rows, uint32_t N, uint32_t D, uint32_t start,
                                       unsigned long long *best, hipStream_t st) {
  hipLaunchKernelGGL(sp_first_valid_kernel, dim3(sp_grid(sp_blocks(N))), dim3(kSpBlock), 0, st, rows, N, D, start,
                     best);
  return hipGetLastError();
}

}  // namespace kmx
