// knn_copy_tile.hpp -- the wave's tile copy of the k-NN index's streaming kernels, ONE copy for both: the merge of an
// add (knn_merge.hip) and the gather of a remove (knn_remove.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace kmx {

// `rows` rows of `nvec` pieces each, consecutive at dst; row r comes from position src_q (of lane r) of the index's
// buffer (src_old of lane r) or the chunk's.  The pieces of the tile are dealt to the lanes as one flat range, so a row
// narrower than the wave leaves no lane idle, and every lane has four loads under way before its first store (two
// and eight, and non-temporal accesses, measured the same within the run-to-run spread: DESIGN_LOG 29).  Four named
// values, not an array: the compiler kept an array in LDS and scratch.
// (A caller with one source passes it for both pointers.)
template <typename T>
__device__ __forceinline__ void copy_tile(const T *__restrict__ from_old, const T *__restrict__ from_chunk, T *__restrict__ dst,
                                          uint32_t nvec, uint32_t rows, uint32_t src_q, bool src_old, uint32_t lane) {
  const uint32_t total = rows * nvec;
  auto fetch = [&](uint32_t idx) -> T {
    const uint32_t r = idx < total ? idx / nvec : 0;   // (every lane takes part in the shuffles)
    const uint32_t q = __shfl(src_q, r);
    const bool old = __shfl((int)src_old, r) != 0;
    if (idx >= total) return T();
    return (old ? from_old : from_chunk)[(size_t)q * nvec + (idx - r * nvec)];
  };
  for (uint32_t base = lane; base < total + lane; base += 256) {   // (the bound is the same for every lane)
    const T v0 = fetch(base), v1 = fetch(base + 64), v2 = fetch(base + 128), v3 = fetch(base + 192);
    if (base < total) dst[base] = v0;
    if (base + 64 < total) dst[base + 64] = v1;
    if (base + 128 < total) dst[base + 128] = v2;
    if (base + 192 < total) dst[base + 192] = v3;
  }
}

}  // namespace kmx
