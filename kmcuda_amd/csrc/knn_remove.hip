// knn_remove.hip -- rows removed from a k-NN index in place (kmamd_knn_index_remove, knn_index.cpp): a
// removed row keeps its id and moves to the tail of the cluster-sorted copies, where kmamd_knn_index_create keeps the
// rows whose assignment is K ("no cluster").  The index's assignments are read back from its CSR, the listed ids are
// set to K, the stable sort of a fresh index gives the new order, and ONE streaming kernel gathers every row's values
// into their new places.  Nothing is computed here: what depends on the row alone was made by the kernels that make
// it for a fresh index (knn_gather / knn_split) and is copied; what depends on membership (mydist, R) is made again by
// those kernels (knn_member / knn_radii) on the host's side of the call.
#include "kernels.hpp"
#include "knn_copy_tile.hpp"
#include "knn_heap.hpp"

namespace kmx {

namespace {

constexpr uint32_t kRemoveTile = 64;   // destination rows per wave and step: one per lane

// a bounded grid of 256-thread blocks over n items, strided in size_t (n / 256 blocks need no bound at 2^32 items, but
// one rule for every launch here)
inline uint32_t item_grid(size_t n) {
  const size_t g = (n + 255) / 256;
  return (uint32_t)(g < kWaveRowGridMax ? (g ? g : 1) : kWaveRowGridMax);
}

// *flag |= 1 if an id is no row of the index
__global__ __launch_bounds__(256) void knn_remove_ids_check_kernel(const uint32_t *__restrict__ ids, uint32_t n, uint32_t N,
                                                                   uint32_t *__restrict__ flag) {
  bool bad = false;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) bad |= ids[i] >= N;
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// The index's assignments and positions by row id, read back from its CSR: the row at sorted position p is inv[p],
// its cluster the one whose range holds p (K: the tail).  inv is a permutation: every entry is written once.
__global__ __launch_bounds__(256) void knn_remove_scatter(const uint32_t *__restrict__ offsets, uint32_t K,
                                                          const uint32_t *__restrict__ inv, uint32_t N,
                                                          uint32_t *__restrict__ asg, uint32_t *__restrict__ pos) {
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < N; p += (size_t)gridDim.x * 256) {
    const uint32_t row = inv[p];
    asg[row] = cluster_of(offsets, K, (uint32_t)p);
    pos[row] = (uint32_t)p;
  }
}

// Every listed id loses its cluster; *count: the ids that had one.  The exchange hands the old value to exactly one of
// the threads that name the same id, so a repeated id counts once.  Integer atomics only.  (ids < N: checked before.)
__global__ __launch_bounds__(256) void knn_remove_mark(const uint32_t *__restrict__ ids, uint32_t n, uint32_t K,
                                                       uint32_t *__restrict__ asg, uint32_t *__restrict__ count) {
  uint32_t mine = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    if (atomicExch(&asg[ids[i]], K) < K) mine++;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
  if (mine && (threadIdx.x & 63) == 0) atomicAdd(count, mine);
}

// One wave per tile of kRemoveTile consecutive destination positions (a bounded grid strides over the tiles,
// kernels.hpp: wave_row_grid), the shape of knn_merge_rows_kernel.  Lane l resolves position p = tile + l: the new
// order names its row (out.inv, written by the sort), pos the sorted position that row has in the index.  The lane
// copies that row's scalars (consecutive destinations: coalesced), then the wave copies the tile's rows
// (knn_copy_tile.hpp).  A pure streaming gather: no LDS, no atomics, every destination row written exactly once; two
// dependent loads in front of a tile's 64 rows.  mydist is not copied: it depends on membership and is made again.
// T32 / T16: 16-byte pieces where the row width allows it, else single elements (the exact search keeps DP = D).
template <typename T32, typename T16>
__global__ __launch_bounds__(256) void knn_remove_rows_kernel(KnnRemoveArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t DP = a.DP, N = a.N;
  const bool f16 = a.out.xs16 != nullptr;
  const uint32_t nvec32 = DP * 4 / (uint32_t)sizeof(T32), nvec16 = DP * 2 / (uint32_t)sizeof(T16);
  const size_t ntiles = ((size_t)N + kRemoveTile - 1) / kRemoveTile;
  // (all index arithmetic in size_t: 8M x 256 floats pass 2^32 bytes)
  for (size_t tile = blockIdx.x * 4 + (threadIdx.x >> 6); tile < ntiles; tile += (size_t)gridDim.x * 4) {
    const size_t p0 = tile * kRemoveTile, p = p0 + lane;
    const uint32_t rows = N - p0 < kRemoveTile ? (uint32_t)(N - p0) : kRemoveTile;
    uint32_t q = 0;
    if (lane < rows) {
      q = a.pos[a.out.inv[p]];
      a.out.n2s[p] = a.old_rows.n2s[q];
      if (f16) {
        a.out.n2c[p] = a.old_rows.n2c[q];
        a.out.mux[p] = a.old_rows.mux[q];
        a.out.kbias[p] = a.old_rows.kbias[q];
      }
    }
    const T32 *src32 = reinterpret_cast<const T32 *>(a.old_rows.xs);
    copy_tile(src32, src32, reinterpret_cast<T32 *>(a.out.xs) + p0 * nvec32, nvec32, rows, q, true, lane);
    if (f16) {
      const T16 *src16 = reinterpret_cast<const T16 *>(a.old_rows.xs16);
      copy_tile(src16, src16, reinterpret_cast<T16 *>(a.out.xs16) + p0 * nvec16, nvec16, rows, q, true, lane);
    }
  }
}

}  // namespace

hipError_t launch_knn_remove_ids_check(const uint32_t *ids, uint32_t n, uint32_t N, uint32_t *flag, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(knn_remove_ids_check_kernel, dim3(item_grid(n)), dim3(256), 0, st, ids, n, N, flag);
  return hipGetLastError();
}

hipError_t launch_knn_remove_scatter(const uint32_t *offsets, uint32_t K, const uint32_t *inv, uint32_t N, uint32_t *asg,
                                     uint32_t *pos, hipStream_t st) {
  if (N == 0) return hipSuccess;
  hipLaunchKernelGGL(knn_remove_scatter, dim3(item_grid(N)), dim3(256), 0, st, offsets, K, inv, N, asg, pos);
  return hipGetLastError();
}

hipError_t launch_knn_remove_mark(const uint32_t *ids, uint32_t n, uint32_t K, uint32_t *asg, uint32_t *count,
                                  hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(knn_remove_mark, dim3(item_grid(n)), dim3(256), 0, st, ids, n, K, asg, count);
  return hipGetLastError();
}

hipError_t launch_knn_remove_rows(const KnnRemoveArgs &a, hipStream_t st) {
  if (a.N == 0) return hipSuccess;
  const uintptr_t ptrs = (uintptr_t)a.old_rows.xs | (uintptr_t)a.out.xs | (uintptr_t)a.old_rows.xs16 | (uintptr_t)a.out.xs16;
  const uint32_t grid = wave_row_grid((a.N - 1) / kRemoveTile + 1);   // a wave per tile
  const uint32_t mask = a.out.xs16 ? 7u : 3u;   // (a half row of DP halves is DP / 8 pieces)
  if ((a.DP & mask) == 0 && (ptrs & 15u) == 0)
    hipLaunchKernelGGL((knn_remove_rows_kernel<uint4, uint4>), dim3(grid), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((knn_remove_rows_kernel<uint32_t, uint16_t>), dim3(grid), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace kmx
