// knn_mask.hip -- what a masked query of the k-NN index prepares once per call (kmamd_knn_index_query_allow /
// _probe_allow): the caller's flags, one byte per row id, as one bit per SORTED position -- the form the
// search kernels' MASK instantiations read --, and the radii of the clusters over their allowed rows.
#include "kernels.hpp"

namespace kmx {

// One wave per 64 sorted positions, one 64-bit ballot each.  The bytes are gathered through inv (a 1-byte read per
// row: 8M rows move 8 MB of flags and 32 MB of inv); positions from *assigned on -- rows without a cluster, the f16
// filter's tile padding, the spare word -- get zeros.
__global__ __launch_bounds__(256) void knn_mask_pack_kernel(const uint8_t *__restrict__ allow,
                                                            const uint32_t *__restrict__ inv,
                                                            const uint32_t *__restrict__ assigned_ptr, size_t nwords,
                                                            unsigned long long *__restrict__ bits) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t assigned = *assigned_ptr;
  for (size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < nwords; w += (size_t)gridDim.x * 4) {
    const size_t p = w * 64 + lane;
    const bool on = p < assigned && allow[inv[p]] != 0;
    const unsigned long long b = __ballot(on);
    if (lane == 0) bits[w] = b;
  }
}

// knn_radii_kernel over the allowed rows (one wave per cluster): the maximum is taken exactly as there, so a cluster's
// radius has the bits a fresh index on the allowed rows gives it; NaN where none is allowed
__global__ __launch_bounds__(64) void knn_masked_radii_kernel(const float *__restrict__ rdist,
                                                              const uint32_t *__restrict__ offsets,
                                                              const uint32_t *__restrict__ bits, float *__restrict__ R,
                                                              uint32_t *__restrict__ count) {
  const uint32_t c = blockIdx.x;
  float mx = -1.f;
  uint32_t n = 0;
  for (uint32_t p = offsets[c] + threadIdx.x; p < offsets[c + 1]; p += 64) {
    if (!((bits[p >> 5] >> (p & 31u)) & 1u)) continue;
    n++;
    const float d = rdist[p];
    if (d > mx) mx = d;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(mx, off);
    if (o > mx) mx = o;
    n += __shfl_xor(n, off);
  }
  if (threadIdx.x == 0) {
    R[c] = mx > -1.f ? mx : NAN;
    count[c] = n;
  }
}

hipError_t launch_knn_mask_pack(const uint8_t *allow, const uint32_t *inv, uint32_t N, const uint32_t *assigned,
                                unsigned long long *bits, hipStream_t st) {
  const size_t nwords = knn_mask_words64(N);
  const size_t blocks = (nwords + 3) / 4;
  hipLaunchKernelGGL(knn_mask_pack_kernel, dim3((uint32_t)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, allow, inv,
                     assigned, nwords, bits);
  return hipGetLastError();
}

hipError_t launch_knn_masked_radii(const float *rdist, const uint32_t *offsets, uint32_t K, const uint32_t *bits,
                                   float *R, uint32_t *count, hipStream_t st) {
  hipLaunchKernelGGL(knn_masked_radii_kernel, dim3(K), dim3(64), 0, st, rdist, offsets, bits, R, count);
  return hipGetLastError();
}

}  // namespace kmx
