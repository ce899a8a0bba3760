// knn_heap.hpp -- the k-NN heap step, ONE copy for every search kernel (knn.hip, knn_f16.hip), and the cluster of a
// sorted position (knn.hip, knn_merge.hip, knn_remove.hip).
#pragma once
#include <stdint.h>

namespace kmx {

__device__ __forceinline__ uint32_t cluster_of(const uint32_t *__restrict__ offsets, uint32_t K, uint32_t p) {
  // largest c with offsets[c] <= p, c in [0, K]; K means "no cluster" (p >= offsets[K])
  uint32_t lo = 0, hi = K + 1;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (offsets[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

// push_sample (knn.cu:133-175): replace-root + sift-down on a max-heap of interleaved (distance, index)
// pairs.  Which child moves up on equal distances decides the order of tied neighbours in the output, so the
// compares are the reference's, one for one.
__device__ __forceinline__ void knn_push_sample(uint32_t k, float dist, uint32_t index, float *heap) {
  uint32_t pos = 0;
  uint32_t *heapi = reinterpret_cast<uint32_t *>(heap);
  while (true) {
    float left = 0.f, right = 0.f;
    bool left_le, right_le;
    if ((2 * pos + 1) < k) { left = heap[4 * pos + 2]; left_le = dist >= left; } else left_le = true;
    if ((2 * pos + 2) < k) { right = heap[4 * pos + 4]; right_le = dist >= right; } else right_le = true;
    if (left_le && right_le) {
      heap[2 * pos] = dist;
      heapi[2 * pos + 1] = index;
      break;
    }
    bool go_right;
    if (!left_le && !right_le) go_right = left <= right;
    else go_right = left_le;
    if (go_right) {
      heap[2 * pos] = right;
      heapi[2 * pos + 1] = heapi[4 * pos + 5];
      pos = 2 * pos + 2;
    } else {
      heap[2 * pos] = left;
      heapi[2 * pos + 1] = heapi[4 * pos + 3];
      pos = 2 * pos + 1;
    }
  }
}

}  // namespace kmx
