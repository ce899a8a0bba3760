// assign_dist.hip -- the kernels kmamd_kmeans_assign (assign_job.cpp) adds to the assignment pass:
//   assigned_distance  distance(row, centroid[assignment]) per row, the per-sample term of the reference's
//                      kmeans_calc_average_distance (kmeans.cu:674-691; metric_abstraction.h:59-72 / :179-191)
//   cluster_stats      per cluster: the number of its rows and the fp64 sum of their distances, in a fixed order
// One serial chain per row in chain_vv's order (exact.hpp): under L2 the distances are distance_vv's bit for bit.  Under
// the angular metric the chain's product is distance_vv's too, and the angle is taken with acosf_fdlibm -- the C
// library's acosf restated, so that the distances equal the CPU oracle's bit for bit -- where distance_vv takes the
// device library's, up to one last place away.
#include <math.h>

#include "exact.hpp"
#include "kernels.hpp"

namespace kmx {

constexpr int kAdBlock = 128;    // rows per block: two tiles of 128 x 36 floats = 36 864 bytes of static LDS
constexpr int kAdStride = 36;    // floats per tile row (conflict-free b128 reads by 16 consecutive rows)

// member_distances_kernel (seeding.hip) lets a thread walk its own row and its own centroid: every 16-byte load of a
// wave touches 64 different lines.  Here both operands come in through LDS, by kmpp_step2_kernel's tile scheme:
// chunks of 32 features, 8 lanes fetch one 128-byte line, a 36-float row stride, the next chunk's loads in flight
// during the chain -- once for the rows and once for the centroids the rows are assigned to (centroids + a[r] * D: a
// gather of whole lines).  A row whose assignment is >= K reads no centroid (zeros in the tile) and gets NaN.
// Rows the 16-byte loads cannot serve (D % 4 != 0, a base that is not 16-byte aligned) take chain_vv itself.
// The grid is bounded and strides over the blocks of rows (kernels.hpp: wave_row_grid).
template <int METRIC>
__global__ __launch_bounds__(kAdBlock) void assigned_distance_kernel(const float *__restrict__ samples, uint32_t N,
                                                                     uint32_t D, const float *__restrict__ centroids,
                                                                     const uint32_t *__restrict__ assignments,
                                                                     uint32_t K, float *__restrict__ dists) {
  const bool tiled = (D & 3u) == 0 && ((((uintptr_t)samples) | ((uintptr_t)centroids)) & 15u) == 0;
  if (!tiled) {
    for (uint64_t s = (uint64_t)blockIdx.x * kAdBlock + threadIdx.x; s < N; s += (uint64_t)gridDim.x * kAdBlock) {
      const uint32_t a = assignments[s];
      if (a < K) {
        const float acc = chain_vv<METRIC>(samples + s * D, centroids + (size_t)a * D, D);
        dists[s] = METRIC == 0 ? sqrtf(acc) : angular_from_prod_libm(acc);
      } else {
        dists[s] = NAN;
      }
    }
    return;
  }
  __shared__ __attribute__((aligned(16))) float xtile[kAdBlock * kAdStride];
  __shared__ __attribute__((aligned(16))) float ctile[kAdBlock * kAdStride];
  __shared__ uint32_t asg[kAdBlock];   // the block's assignments; 0xFFFFFFFF: no centroid to read
  const uint32_t nchunk = (D + 31) / 32;
  for (uint64_t base = (uint64_t)blockIdx.x * kAdBlock; base < N; base += (uint64_t)gridDim.x * kAdBlock) {
    __syncthreads();   // the previous round's tiles and asg[] are done with
    const uint64_t s = base + threadIdx.x;
    {
      const uint32_t a = s < N ? assignments[s] : 0xFFFFFFFFu;
      asg[threadIdx.x] = a < K ? a : 0xFFFFFFFFu;
    }
    __syncthreads();
    float4 xstage[8], cstage[8];
    auto fetch = [&](uint32_t ch) {
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const uint32_t p = threadIdx.x + kAdBlock * q, r = p >> 3, c4 = p & 7u;
        const uint64_t row = base + r;
        const uint32_t f = ch * 32 + c4 * 4, a = asg[r];
        const bool live = row < N && f < D;
        xstage[q] = live ? *reinterpret_cast<const float4 *>(samples + row * D + f) : make_float4(0.f, 0.f, 0.f, 0.f);
        cstage[q] = (live && a != 0xFFFFFFFFu) ? *reinterpret_cast<const float4 *>(centroids + (size_t)a * D + f)
                                               : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    };
    float acc = 0.f, corr = 0.f;
    fetch(0);
    for (uint32_t ch = 0; ch < nchunk; ch++) {
      if (ch) __syncthreads();   // the previous chunk has been consumed
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const uint32_t p = threadIdx.x + kAdBlock * q, r = p >> 3, c4 = p & 7u;
        *reinterpret_cast<float4 *>(&xtile[r * kAdStride + c4 * 4]) = xstage[q];
        *reinterpret_cast<float4 *>(&ctile[r * kAdStride + c4 * 4]) = cstage[q];
      }
      __syncthreads();
      if (ch + 1 < nchunk) fetch(ch + 1);
      const uint32_t fmax = D - ch * 32 < 32u ? D - ch * 32 : 32u;   // multiple of 4
      for (uint32_t c4 = 0; c4 * 4 < fmax; c4++) {
        const float4 xv = *reinterpret_cast<const float4 *>(&xtile[threadIdx.x * kAdStride + c4 * 4]);
        const float4 cv = *reinterpret_cast<const float4 *>(&ctile[threadIdx.x * kAdStride + c4 * 4]);
        const float aa[4] = {xv.x, xv.y, xv.z, xv.w}, bb[4] = {cv.x, cv.y, cv.z, cv.w};
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
      const float dist = METRIC == 0 ? sqrtf(acc) : angular_from_prod_libm(acc);
      dists[s] = asg[threadIdx.x] != 0xFFFFFFFFu ? dist : NAN;
    }
  }
}

static uint32_t assigned_distance_grid(uint32_t N) {
  const uint32_t g = (N + kAdBlock - 1) / kAdBlock;
  return g < kWaveRowGridMax ? (g ? g : 1u) : kWaveRowGridMax;
}

hipError_t launch_assigned_distances(int metric, const float *samples, uint32_t N, uint32_t D, const float *centroids,
                                     const uint32_t *assignments, uint32_t K, float *dists, hipStream_t st) {
  if (N == 0) return hipSuccess;
  const dim3 grid(assigned_distance_grid(N)), block(kAdBlock);
  return with_metric(metric, [&](auto M) {
    hipLaunchKernelGGL((assigned_distance_kernel<M()>), grid, block, 0, st, samples, N, D, centroids, assignments, K, dists);
    return hipGetLastError();
  });
}

// One wave per cluster over the chunk's CSR (launch_inverse_assignments: a stable sort, so a cluster's rows stand in
// ascending row order; the rows without a cluster, key K, lie behind offsets[K] and are in neither output).  Lane l
// adds members l, l + 64, ... in that order in fp64, then the 64 partial sums meet in a fixed butterfly: the same
// bits whenever the chunk is the same.  counts[c] and sums[c] ACCUMULATE (the caller zeroes them before the first
// chunk; the stream orders the chunks), no atomics.
__global__ __launch_bounds__(256) void cluster_stats_kernel(const float *__restrict__ dists,
                                                            const uint32_t *__restrict__ inv,
                                                            const uint32_t *__restrict__ offsets, uint32_t K,
                                                            uint32_t *__restrict__ counts, double *__restrict__ sums) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint64_t c = (uint64_t)blockIdx.x * 4 + wave; c < K; c += (uint64_t)gridDim.x * 4) {
    const uint32_t p0 = offsets[c], p1 = offsets[c + 1];
    if (counts && lane == 0) counts[c] += p1 - p0;
    if (!sums) continue;
    double acc = 0.0;
    for (uint64_t p = (uint64_t)p0 + lane; p < p1; p += 64) acc += (double)dists[inv[p]];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if (lane == 0) sums[c] += acc;
  }
}

hipError_t launch_cluster_stats(const float *dists, const uint32_t *inv, const uint32_t *offsets, uint32_t K,
                                uint32_t *counts, double *sums, hipStream_t st) {
  if (K == 0 || (!counts && !sums)) return hipSuccess;
  hipLaunchKernelGGL(cluster_stats_kernel, dim3(wave_row_grid(K)), dim3(256), 0, st, dists, inv, offsets, K, counts,
                     sums);
  return hipGetLastError();
}

}  // namespace kmx
