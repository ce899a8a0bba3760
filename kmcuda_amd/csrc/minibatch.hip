// minibatch.hip -- the kernels of mini-batch K-means (kmamd_minibatch_*, minibatch_job.cpp): the update
// of the resident centroids from ALL rows of a batch, and the batch draw of a device-resident corpus.
//
//   minibatch_update   one block per centroid over the CSR launch_inverse_assignments leaves for the batch (a stable
//                      sort: a centroid's members stand in ascending batch position).  The block adds up its members'
//                      weights (n_c) and rows (S_c) in fp64 -- list_sum.hpp, the association of cluster_sums
//                      (update.hip), in its scalar and 16-byte mappings -- and applies Sculley's step to C and W in
//                      place: W' = W + n_c, C' = (C W + S_c) / W' (L2) or (C W + S_c) / |C W + S_c| (angular), rounded
//                      once to fp32.  Nothing is all-reduced, so there is no K x D buffer of sums and no second launch.
//                      A centroid without members returns before it touches anything: C and W keep their bits.  The
//                      member list is read where the sort left it, so its length is bounded by the batch alone.
//   minibatch_draw_gather   slot j of step t holds corpus row floor(h(seed, t, j) N / 2^64) (hash_draw.hpp): a wave
//                      copies the row, as it is (floats or halves), and its weight.
#include "hash_draw.hpp"
#include "kernels.hpp"
#include "list_sum.hpp"

namespace kmx {

namespace {

constexpr uint32_t kMbThreads = 1024;
constexpr uint32_t kMbStash = 4096;   // angular: C W + S_c waits in LDS for its norm up to this many features

struct MbArgs {
  const float *rows;        // n x D, the batch
  const float *weights;     // n, finite and > 0 (WEIGHTED)
  const uint32_t *inv;      // the batch positions sorted by cluster
  const uint32_t *offsets;  // K + 1 segment starts
  uint32_t D;
  float *centroids;         // K x D, in place
  double *cweights;         // K, in place
};

template <int METRIC, bool VEC4, bool WEIGHTED>
__global__ __launch_bounds__(kMbThreads) void minibatch_update_kernel(MbArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mb_lds[];
  double *part = reinterpret_cast<double *>(mb_lds);   // 4 per thread
  double *stash = part + kMbThreads * 4;               // angular, D <= kMbStash: D doubles
  __shared__ double sh_val;
  const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t D = a.D;
  const uint32_t o0 = a.offsets[c], n = a.offsets[c + 1] - o0;
  if (n == 0) return;   // no member in the batch: C_c and W_c keep their bits
  const uint32_t *rows = a.inv + o0;
  float *cen = a.centroids + (size_t)c * D;
  const double W = a.cweights[c];

  // ---- n_c: the members' weights in an order that depends on the list alone (cluster_sums' wsum) ----
  double nc = (double)n;
  if constexpr (WEIGHTED) {
    double t = 0.0;
    for (uint32_t r = tid; r < n; r += kMbThreads) t += (double)a.weights[rows[r]];
    part[tid] = t;
    __syncthreads();
    if (wave == 0) {
      t = part[lane];
      for (uint32_t k = 1; k < kMbThreads / 64; k++) t += part[k * 64 + lane];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
      if (lane == 0) sh_val = t;
    }
    __syncthreads();
    nc = sh_val;
    __syncthreads();   // `part` and sh_val go to the feature sums and the norm
  }
  const double Wn = W + nc;

  // what the thread that holds S_c[f] does with it
  double acc = 0.0, nrm = 1.0;
  const bool stashed = METRIC == 1 && D <= kMbStash;
  auto settle = [&](uint32_t f, double s, int phase) {
    const double v = (double)cen[f] * W + s;
    if (METRIC == 0) {
      cen[f] = (float)(v / Wn);
    } else if (phase == 0) {
      acc += v * v;
      if (stashed) stash[f] = v;
    } else {
      cen[f] = (float)(v / nrm);
    }
  };

  // ---- S_c: fl lanes across the features, groups of rows; the two mappings of cluster_sums_body, chosen by the
  //      length of the list ----
  auto sweep = [&](int phase) {
    if (VEC4 && n >= 128u) {
      uint32_t fl = 16;   // lanes per row: a power of two covering D / 4, at most 256
      while (fl < 256u && fl * 4u < D) fl <<= 1;
      const uint32_t groups = kMbThreads / fl, g = tid / fl, lf = tid % fl;
      const uint32_t chunk = (n + groups - 1) / groups;
      const uint32_t r0 = min(n, g * chunk), r1 = min(n, r0 + chunk);
      for (uint32_t f0 = 0; f0 < D; f0 += 4u * fl) {
        const uint32_t f = f0 + 4u * lf;
        const bool fv = f < D;
        double mine[4] = {0.0, 0.0, 0.0, 0.0};
        if (fv && r1 > r0) list_sum4<WEIGHTED>(a.rows, a.weights, D, rows, r0, r1, f, mine);
#pragma unroll
        for (int e = 0; e < 4; e++) part[(size_t)tid * 4 + e] = mine[e];
        __syncthreads();
        if (g == 0 && fv) {
#pragma unroll
          for (int e = 0; e < 4; e++) {
            double t = part[(size_t)lf * 4 + e];
            for (uint32_t gg = 1; gg < groups; gg++) t += part[(size_t)(gg * fl + lf) * 4 + e];
            settle(f + e, t, phase);
          }
        }
        __syncthreads();
      }
    } else {
      const uint32_t fl = D > 128 ? 256u : (D > 64 ? 128u : 64u), groups = kMbThreads / fl;
      const uint32_t g = tid / fl, lf = tid % fl;
      const uint32_t chunk = (n + groups - 1) / groups;
      const uint32_t r0 = min(n, g * chunk), r1 = min(n, r0 + chunk);
      for (uint32_t f0 = 0; f0 < D; f0 += fl) {
        const uint32_t f = f0 + lf;
        const bool fv = f < D;
        part[tid] = (fv && r1 > r0) ? list_sum<WEIGHTED>(a.rows, a.weights, D, rows, r0, r1, f) : 0.0;
        __syncthreads();
        if (g == 0 && fv) {
          double t = part[lf];
          for (uint32_t gg = 1; gg < groups; gg++) t += part[gg * fl + lf];
          settle(f, t, phase);
        }
        __syncthreads();
      }
    }
  };

  sweep(0);
  if (METRIC == 1) {
    // |C W + S_c|: every thread's squares in ascending feature order, the threads through a fixed LDS tree
    part[tid] = acc;
    __syncthreads();
    for (uint32_t s = kMbThreads / 2; s > 0; s >>= 1) {
      if (tid < s) part[tid] += part[tid + s];
      __syncthreads();
    }
    nrm = sqrt(part[0]);
    __syncthreads();
    if (stashed) {
      for (uint32_t f = tid; f < D; f += kMbThreads) cen[f] = (float)(stash[f] / nrm);
    } else {
      sweep(1);   // wider rows: the same sums once more (the same bits), divided this time
    }
  }
  if (tid == 0) a.cweights[c] = Wn;
}

template <typename T>
__global__ __launch_bounds__(256) void minibatch_draw_gather_kernel(const T *__restrict__ corpus, uint64_t N,
                                                                    uint32_t units /* of T per row */,
                                                                    const float *__restrict__ cweights_in,
                                                                    uint32_t seed, uint32_t step, uint32_t batch,
                                                                    T *__restrict__ out, float *__restrict__ wout) {
  const uint32_t j = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= batch) return;
  const uint64_t row = draw_row(hash_draw(seed, step, j), N);
  const T *src = corpus + row * units;
  T *dst = out + (size_t)j * units;
  for (uint32_t i = lane; i < units; i += 64) dst[i] = src[i];
  if (cweights_in && lane == 0) wout[j] = cweights_in[row];
}

}  // namespace

hipError_t launch_minibatch_update(int metric, const float *rows, const float *weights, const uint32_t *inv,
                                   const uint32_t *offsets, uint32_t K, uint32_t D, float *centroids,
                                   double *cluster_weights, hipStream_t st) {
  MbArgs a;
  a.rows = rows; a.weights = weights; a.inv = inv; a.offsets = offsets; a.D = D;
  a.centroids = centroids; a.cweights = cluster_weights;
  // (the mapping depends on D and the rows' alignment only, as in launch_move_deltas)
  const bool vec4 = (D & 3u) == 0 && (((uintptr_t)rows) & 15u) == 0;
  const size_t lds = kMbThreads * 4 * sizeof(double) + ((metric == 1 && D <= kMbStash) ? (size_t)D * sizeof(double) : 0);
  return with_metric(metric, [&](auto M) {
    return with_flag(vec4, [&](auto V) {
      return with_flag(weights != nullptr, [&](auto W) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&minibatch_update_kernel<M(), V(), W()>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((minibatch_update_kernel<M(), V(), W()>), dim3(K), dim3(kMbThreads), lds, st, a);
        return hipGetLastError();
      });
    });
  });
}

hipError_t launch_minibatch_draw_gather(const void *corpus, uint64_t N, uint32_t D, bool fp16, const float *weights,
                                        uint32_t seed, uint32_t step, uint32_t batch, void *out, float *weights_out,
                                        hipStream_t st) {
  if (batch == 0) return hipSuccess;
  const size_t row_bytes = (size_t)D * (fp16 ? sizeof(uint16_t) : sizeof(float));
  const uintptr_t both = (uintptr_t)corpus | (uintptr_t)out;
  const dim3 grid((batch + 3) / 4), block(256);
  if ((row_bytes & 15u) == 0 && (both & 15u) == 0)
    hipLaunchKernelGGL(minibatch_draw_gather_kernel<uint4>, grid, block, 0, st, static_cast<const uint4 *>(corpus), N,
                       (uint32_t)(row_bytes / 16), weights, seed, step, batch, static_cast<uint4 *>(out), weights_out);
  else if ((row_bytes & 3u) == 0 && (both & 3u) == 0)
    hipLaunchKernelGGL(minibatch_draw_gather_kernel<uint32_t>, grid, block, 0, st,
                       static_cast<const uint32_t *>(corpus), N, (uint32_t)(row_bytes / 4), weights, seed, step, batch,
                       static_cast<uint32_t *>(out), weights_out);
  else
    hipLaunchKernelGGL(minibatch_draw_gather_kernel<uint16_t>, grid, block, 0, st,
                       static_cast<const uint16_t *>(corpus), N, (uint32_t)(row_bytes / 2), weights, seed, step, batch,
                       static_cast<uint16_t *>(out), weights_out);
  return hipGetLastError();
}

}  // namespace kmx
