// knn_merge.hip -- rows added to a k-NN index in place (kmamd_knn_index_add, knn_index.cpp): the
// cluster-sorted copies of the index and those of one prepared chunk of new rows become ONE cluster-sorted set, every
// cluster's old members first and the chunk's behind them (both in ascending row id, and every new id is larger than
// every old one: the order kmamd_knn_index_create gives the concatenation).  Nothing is computed here: every value
// was made per row by the kernels that make it for a fresh index (knn_gather / knn_member / knn_split), so the merged
// index holds the bits the fresh one would.
#include "kernels.hpp"
#include "knn_copy_tile.hpp"
#include "knn_heap.hpp"

namespace kmx {

namespace {

constexpr uint32_t kMergeTile = 64;   // destination rows per wave and step: one per lane
// One wave per tile of kMergeTile consecutive destination positions (a bounded grid strides over the tiles,
// kernels.hpp: wave_row_grid).  Lane l resolves position p = tile + l: it lies in cluster c (K: the rows without a
// cluster) at rank j; ranks below the cluster's old size come from the index, the others from the chunk.  The lane
// copies that row's scalars (consecutive destinations: coalesced), then the wave copies the tile's rows.  A pure
// streaming copy: no LDS, no atomics, every destination row written exactly once.  T32 / T16: 16-byte pieces where
// the row width allows it, else single elements (the exact search keeps DP = D, any width).
// (One wave per row, each lane walking the offsets for itself, reached 2.2 TB/s at 8M x 256: ten dependent loads in
// front of every 1.5 KB; this one 5.5 - 5.8 TB/s.  DESIGN_LOG 29.)
template <typename T32, typename T16>
__global__ __launch_bounds__(256) void knn_merge_rows_kernel(KnnMergeArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t K = a.K, DP = a.DP, N_new = a.N_old + a.n;
  const bool f16 = a.out.xs16 != nullptr;
  const uint32_t nvec32 = DP * 4 / (uint32_t)sizeof(T32), nvec16 = DP * 2 / (uint32_t)sizeof(T16);
  const size_t ntiles = ((size_t)N_new + kMergeTile - 1) / kMergeTile;
  // (all index arithmetic in size_t: 8M x 256 floats pass 2^32 bytes)
  for (size_t tile = blockIdx.x * 4 + (threadIdx.x >> 6); tile < ntiles; tile += (size_t)gridDim.x * 4) {
    const size_t p0 = tile * kMergeTile, p = p0 + lane;
    const uint32_t rows = N_new - p0 < kMergeTile ? (uint32_t)(N_new - p0) : kMergeTile;
    uint32_t q = 0;
    bool old = true;
    if (lane < rows) {
      const uint32_t c = cluster_of(a.off_new, K, (uint32_t)p);
      const uint32_t j = (uint32_t)p - a.off_new[c];
      const uint32_t first_old = a.off_old[c];
      const uint32_t cnt_old = (c < K ? a.off_old[c + 1] : a.N_old) - first_old;
      old = j < cnt_old;
      q = old ? first_old + j : a.boffs[c] + (j - cnt_old);
      // (pointer by pointer: a reference to one of the two structs would put both into scratch)
      a.out.n2s[p] = (old ? a.old_rows.n2s : a.chunk.n2s)[q];
      a.out.mydist[p] = (old ? a.old_rows.mydist : a.chunk.mydist)[q];
      a.out.inv[p] = old ? a.old_rows.inv[q] : a.N_old + a.chunk.inv[q];
      if (f16) {
        a.out.n2c[p] = (old ? a.old_rows.n2c : a.chunk.n2c)[q];
        a.out.mux[p] = (old ? a.old_rows.mux : a.chunk.mux)[q];
        a.out.kbias[p] = (old ? a.old_rows.kbias : a.chunk.kbias)[q];
      }
    }
    copy_tile(reinterpret_cast<const T32 *>(a.old_rows.xs), reinterpret_cast<const T32 *>(a.chunk.xs),
              reinterpret_cast<T32 *>(a.out.xs) + p0 * nvec32, nvec32, rows, q, old, lane);
    if (f16)
      copy_tile(reinterpret_cast<const T16 *>(a.old_rows.xs16), reinterpret_cast<const T16 *>(a.chunk.xs16),
                reinterpret_cast<T16 *>(a.out.xs16) + p0 * nvec16, nvec16, rows, q, old, lane);
  }
}

// One wave per cluster, as knn_radii_kernel: R = max(the old radius, the chunk's largest member distance); NaN (an
// empty cluster, knn.cu:46-57) gives way to the first members' maximum and stays where none arrive.  The first wave also
// folds the chunk's maxima and half-range flag into the new statistics.
__global__ __launch_bounds__(64) void knn_merge_radii_kernel(const float *__restrict__ R_old, const float *__restrict__ rdist,
                                                             const uint32_t *__restrict__ boffs, float *__restrict__ R_new,
                                                             const uint32_t *__restrict__ stats_old,
                                                             const uint32_t *__restrict__ stats_c_old,
                                                             const uint32_t *__restrict__ bstats,
                                                             uint32_t *__restrict__ stats_new, uint32_t *__restrict__ stats_c_new) {
  const uint32_t c = blockIdx.x;
  float mx = -1.f;
  for (uint32_t p = boffs[c] + threadIdx.x; p < boffs[c + 1]; p += 64) {
    const float d = rdist[p];
    if (d > mx) mx = d;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(mx, off);
    if (o > mx) mx = o;
  }
  if (threadIdx.x != 0) return;
  const float r = R_old[c];
  R_new[c] = r >= mx ? r : (mx > -1.f ? mx : NAN);
  if (c == 0) {
    // (maxima of finite, non-negative floats: bits order like values; bstats: [0] plain maximum, [1] flag, [2] centred)
    stats_new[0] = stats_old[0] > bstats[0] ? stats_old[0] : bstats[0];
    stats_new[1] = stats_old[1] | bstats[1];
    if (stats_c_new) stats_c_new[0] = stats_c_old[0] > bstats[2] ? stats_c_old[0] : bstats[2];
  }
}

}  // namespace

hipError_t launch_knn_merge_rows(const KnnMergeArgs &a, hipStream_t st) {
  const uint32_t N_new = a.N_old + a.n;
  if (N_new == 0) return hipSuccess;
  const uintptr_t ptrs = (uintptr_t)a.old_rows.xs | (uintptr_t)a.chunk.xs | (uintptr_t)a.out.xs | (uintptr_t)a.old_rows.xs16 |
                         (uintptr_t)a.chunk.xs16 | (uintptr_t)a.out.xs16;
  const uint32_t grid = wave_row_grid((N_new - 1) / kMergeTile + 1);   // a wave per tile
  const uint32_t mask = a.out.xs16 ? 7u : 3u;   // (a half row of DP halves is DP / 8 pieces)
  if ((a.DP & mask) == 0 && (ptrs & 15u) == 0)
    hipLaunchKernelGGL((knn_merge_rows_kernel<uint4, uint4>), dim3(grid), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((knn_merge_rows_kernel<uint32_t, uint16_t>), dim3(grid), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_knn_merge_radii(const float *R_old, const float *rdist, const uint32_t *boffs, uint32_t K, float *R_new,
                                  const uint32_t *stats_old, const uint32_t *stats_c_old, const uint32_t *bstats,
                                  uint32_t *stats_new, uint32_t *stats_c_new, hipStream_t st) {
  hipLaunchKernelGGL(knn_merge_radii_kernel, dim3(K), dim3(64), 0, st, R_old, rdist, boffs, R_new, stats_old, stats_c_old,
                     bstats, stats_new, stats_c_new);
  return hipGetLastError();
}

}  // namespace kmx
