// hash_draw.hpp -- the stateless draw of include/kmcuda_amd.h for host and device code: h(seed, r, s), k-means||'s hash
// (seed_par.hip and seed_par_job.cpp hold their own copies of it), and the mini-batch draw built on it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kmx {

__host__ __device__ inline uint64_t hash_draw(uint32_t seed, uint32_t r, uint32_t s) {
  uint64_t z = (((uint64_t)r << 32) | s) + ((uint64_t)seed + 1ull) * 0x9E3779B97F4A7C15ull;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

// floor(h * N / 2^64): the high 64 bits of the 128-bit product, a row of [0, N)
__host__ __device__ inline uint64_t draw_row(uint64_t h, uint64_t N) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(h, N);
#else
  return (uint64_t)(((unsigned __int128)h * N) >> 64);
#endif
}

}  // namespace kmx
