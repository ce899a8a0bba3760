// list_sum.hpp -- the fp64 column sum of a list of rows in the FIXED association of DESIGN.md 4.3: what cluster_sums
// (update.hip: the moved rows of a Lloyd step) and minibatch_update (minibatch.hip: all rows of a batch) run per thread.
// The result depends on the list (rows ascending) and the range [r0, r1) alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kmx {

// WEIGHTED: every row's term is (double)w * (double)x -- exact in fp64 (24 x 24 bits), so the sum rounds where the
// unweighted one does.  The weight's address depends on rows[] alone, like the row's: the two loads of a list entry
// are issued together and the weight never stands in front of the row (one 4-byte gather beside 4 D bytes).
template <bool WEIGHTED>
__device__ __forceinline__ double list_sum(const float *__restrict__ samples, const float *__restrict__ weights,
                                           uint32_t D, const uint32_t *rows, uint32_t r0, uint32_t r1, uint32_t f) {
  double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t r = r0;
  for (; r + 8 <= r1; r += 8) {
    float x[8], w[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint32_t row = rows[r + j];
      x[j] = samples[(size_t)row * D + f];
      if constexpr (WEIGHTED) w[j] = weights[row];
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if constexpr (WEIGHTED) a[j] += (double)w[j] * (double)x[j];
      else a[j] += (double)x[j];
    }
  }
  for (uint32_t j = 0; r < r1; r++, j++) {
    const uint32_t row = rows[r];
    if constexpr (WEIGHTED) a[j] += (double)weights[row] * (double)samples[(size_t)row * D + f];
    else a[j] += (double)samples[(size_t)row * D + f];
  }
  return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

// the same for four consecutive features per lane (16-byte loads; D % 4 == 0, aligned rows): four accumulator
// sets by row position, folded as (a0 + a1) + (a2 + a3)
template <bool WEIGHTED>
__device__ __forceinline__ void list_sum4(const float *__restrict__ samples, const float *__restrict__ weights,
                                          uint32_t D, const uint32_t *rows, uint32_t r0, uint32_t r1, uint32_t f,
                                          double (&out)[4]) {
  double a[4][4];
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int e = 0; e < 4; e++) a[j][e] = 0.0;
  uint32_t r = r0;
  for (; r + 4 <= r1; r += 4) {
    float4 x[4];
    double w[4] = {1.0, 1.0, 1.0, 1.0};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t row = rows[r + j];
      x[j] = *reinterpret_cast<const float4 *>(samples + (size_t)row * D + f);
      if constexpr (WEIGHTED) w[j] = (double)weights[row];
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if constexpr (WEIGHTED) {
        a[j][0] += w[j] * (double)x[j].x; a[j][1] += w[j] * (double)x[j].y;
        a[j][2] += w[j] * (double)x[j].z; a[j][3] += w[j] * (double)x[j].w;
      } else {
        a[j][0] += (double)x[j].x; a[j][1] += (double)x[j].y; a[j][2] += (double)x[j].z; a[j][3] += (double)x[j].w;
      }
    }
  }
  for (uint32_t j = 0; r < r1; r++, j++) {
    const uint32_t row = rows[r];
    float4 x = *reinterpret_cast<const float4 *>(samples + (size_t)row * D + f);
    double x0 = (double)x.x, x1 = (double)x.y, x2 = (double)x.z, x3 = (double)x.w;
    if constexpr (WEIGHTED) {
      const double w = (double)weights[row];
      x0 *= w; x1 *= w; x2 *= w; x3 *= w;
    }
    // (j < 4: static indexing after unrolling)
    if (j == 0) { a[0][0] += x0; a[0][1] += x1; a[0][2] += x2; a[0][3] += x3; }
    else if (j == 1) { a[1][0] += x0; a[1][1] += x1; a[1][2] += x2; a[1][3] += x3; }
    else { a[2][0] += x0; a[2][1] += x1; a[2][2] += x2; a[2][3] += x3; }
  }
#pragma unroll
  for (int e = 0; e < 4; e++) out[e] = (a[0][e] + a[1][e]) + (a[2][e] + a[3][e]);
}

}  // namespace kmx
