// knn_merge_host.hpp -- the host arithmetic of kmamd_knn_index_add (knn_index.cpp) and the rows per
// chunk of every chunked index call, free of any device call so that a stand-alone program can drive it
// (scripts/knn_merge_host_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace kmx {

// The largest row count of an index: 0xFFFFFFFF is the "no neighbour" marker of the searches
constexpr uint64_t kKnnMaxRows = 0xFFFFFFFEull;

inline bool knn_add_fits(uint32_t n_old, uint32_t n_add) { return (uint64_t)n_old + n_add <= kKnnMaxRows; }

// The CSR offsets of the index after one merge.  off_old: K + 2 entries (off_old[c]: first sorted position of cluster
// c; [K]: of the rows without a cluster; [K + 1] = N_old); boffs: the chunk's K + 1 offsets as
// launch_inverse_assignments leaves them (boffs[K]: the chunk's rows that have a cluster), n: the chunk's rows.  A
// cluster's new members go behind its old ones, so every cluster starts later by the number of chunk rows in front of
// it -- the exclusive prefix of the chunk's counts, which boffs is.  False (off_new untouched) unless both inputs are
// offsets of what they claim: non-decreasing, starting at 0, ending at N_old / within n, and the sum fits.
inline bool knn_merge_offsets(const std::vector<uint32_t> &off_old, const uint32_t *boffs, uint32_t K, uint32_t n,
                              std::vector<uint32_t> *off_new) {
  if (off_old.size() != (size_t)K + 2 || off_old[0] != 0 || boffs[0] != 0 || boffs[K] > n) return false;
  for (uint32_t c = 0; c <= K; c++)
    if (off_old[c] > off_old[c + 1] || (c < K && boffs[c] > boffs[c + 1])) return false;
  const uint32_t N_old = off_old[(size_t)K + 1];
  if (!knn_add_fits(N_old, n)) return false;
  std::vector<uint32_t> out((size_t)K + 2);
  for (uint32_t c = 0; c <= K; c++) out[c] = off_old[c] + boffs[c];
  out[(size_t)K + 1] = N_old + n;
  off_new->swap(out);
  return true;
}

// Rows per chunk of a chunked index call over n rows: as many as `budget` bytes hold at row_bytes (> 0) each, or
// `forced` where a test hook sets it (KMCUDA_AMD_KNN_QUERY_CHUNK, KMCUDA_AMD_KNN_ADD_CHUNK); at least one row, never
// more than n
inline uint32_t knn_chunk_rows(size_t budget, size_t row_bytes, size_t forced, uint32_t n) {
  size_t rows = forced ? forced : budget / row_bytes;
  if (rows < 1) rows = 1;
  return rows < n ? (uint32_t)rows : n;
}

// The queries of one chunk of a radius fill to a caller on the host, whose hits are staged on the device: of the n (>=
// 1) queries from q0 on, as many as have their CSR range offsets[q0 + n] - offsets[q0] (non-decreasing offsets) within
// max_hits -- n halved, rounding up, until it fits; a single query larger than that stays a chunk of its own
inline uint32_t knn_fill_chunk_rows(const uint64_t *offsets, uint32_t q0, uint32_t n, uint64_t max_hits) {
  while (n > 1 && offsets[(size_t)q0 + n] - offsets[q0] > max_hits) n = (n + 1) / 2;
  return n;
}

// ... of an add: a chunk's staged fp32 rows (D floats), its sorted fp32 copy (DP floats), the centred halves (DP) and
// the per-row scalars and sort scratch (some 48 bytes)
inline uint32_t knn_add_chunk_rows(uint32_t n, uint32_t D, uint32_t DP, size_t budget, size_t forced) {
  return knn_chunk_rows(budget, (size_t)D * 4 + (size_t)DP * 6 + 48, forced, n);
}

}  // namespace kmx
