// knn_merge_host_check.cpp -- drives the host arithmetic of kmamd_knn_index_add (kmcuda_amd/csrc/knn_merge_host.hpp:
// the merged CSR offsets, the row limit, the chunk loop, the rows per chunk of every chunked index call) on the CPU
// against a plain recount, and replays the merge
// kernel's source rule on the host to check that every destination position gets exactly one source row in the order a
// fresh index has.  No device call: meant for a build with the host sanitizers,
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I kmcuda_amd/csrc \
//       scripts/knn_merge_host_check.cpp -o knn_merge_host_check && ./knn_merge_host_check
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <numeric>
#include <random>

#include "knn_merge_host.hpp"

using namespace kmx;

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
      failures++;                                                       \
    }                                                                   \
  } while (0)

// what launch_inverse_assignments leaves for assignments (ids >= K: no cluster): inv (stable by cluster) and K + 1
// offsets; all: K + 2 entries, the last one the row count (an index's host copy)
static void csr(const std::vector<uint32_t> &asg, uint32_t K, std::vector<uint32_t> *inv, std::vector<uint32_t> *offs,
                bool all) {
  std::vector<uint32_t> key(asg.size());
  for (size_t i = 0; i < asg.size(); i++) key[i] = asg[i] < K ? asg[i] : K;
  inv->resize(asg.size());
  std::iota(inv->begin(), inv->end(), 0u);
  std::stable_sort(inv->begin(), inv->end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
  offs->assign((size_t)K + (all ? 2 : 1), 0);
  for (uint32_t c = 0; c <= K; c++)
    (*offs)[c] = (uint32_t)std::count_if(key.begin(), key.end(), [&](uint32_t v) { return v < c; });
  if (all) (*offs)[(size_t)K + 1] = (uint32_t)asg.size();
}

// knn_merge_rows_kernel's rule for destination position p: which row id lands there
static uint32_t merged_row(uint32_t p, uint32_t K, const std::vector<uint32_t> &off_old, const std::vector<uint32_t> &inv_old,
                           const std::vector<uint32_t> &boffs, const std::vector<uint32_t> &binv,
                           const std::vector<uint32_t> &off_new) {
  uint32_t lo = 0, hi = K + 1;   // cluster_of
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (off_new[mid] <= p) lo = mid; else hi = mid;
  }
  const uint32_t c = lo, j = p - off_new[c], N_old = off_old[(size_t)K + 1];
  const uint32_t cnt_old = (c < K ? off_old[c + 1] : N_old) - off_old[c];
  return j < cnt_old ? inv_old.at((size_t)off_old[c] + j) : N_old + binv.at((size_t)boffs[c] + (j - cnt_old));
}

static void one_case(uint32_t K, uint32_t n_old, uint32_t n_add, size_t chunk, unsigned seed, bool skewed) {
  std::mt19937 rng(seed);
  auto draw = [&](uint32_t n, uint32_t lo_c, uint32_t hi_c) {   // ids in [lo_c, hi_c], hi_c may be K and above
    std::vector<uint32_t> a(n);
    for (auto &v : a) v = lo_c + rng() % (hi_c - lo_c + 1);
    return a;
  };
  // skewed: the old rows leave the upper clusters empty, the new rows sit in few clusters, some rows have none
  std::vector<uint32_t> a_old = skewed ? draw(n_old, 0, K / 2) : draw(n_old, 0, K + 1);
  std::vector<uint32_t> a_add = skewed ? draw(n_add, K / 2, K + 2) : draw(n_add, 0, K);
  std::vector<uint32_t> inv, off, binv, boffs, next;
  csr(a_old, K, &inv, &off, true);
  std::vector<uint32_t> all = a_old;
  uint32_t done = 0;
  while (done < n_add) {   // the chunk loop of KnnIndex::add
    const uint32_t n = knn_add_chunk_rows(n_add - done, 64, 64, (size_t)4 << 30, chunk);
    CHECK(n >= 1 && n <= n_add - done);
    std::vector<uint32_t> piece(a_add.begin() + done, a_add.begin() + done + n);
    csr(piece, K, &binv, &boffs, false);
    CHECK(knn_merge_offsets(off, boffs.data(), K, n, &next));
    std::vector<uint32_t> inv_next((size_t)off[(size_t)K + 1] + n);
    for (uint32_t p = 0; p < inv_next.size(); p++) inv_next[p] = merged_row(p, K, off, inv, boffs, binv, next);
    inv.swap(inv_next);
    off.swap(next);
    all.insert(all.end(), piece.begin(), piece.end());
    done += n;
  }
  // the index a fresh build makes of all rows
  std::vector<uint32_t> want_inv, want_off;
  csr(all, K, &want_inv, &want_off, true);
  CHECK(off == want_off);
  CHECK(inv == want_inv);
}

int main() {
  for (uint32_t K : {1u, 2u, 7u, 64u})
    for (uint32_t n_old : {1u, 63u, 200u})
      for (uint32_t n_add : {1u, 5u, 64u, 333u})
        for (size_t chunk : {(size_t)0, (size_t)1, (size_t)5, (size_t)1000})
          for (int skewed = 0; skewed < 2; skewed++)
            one_case(K, n_old, n_add, chunk, 17u * K + n_old + n_add + (unsigned)chunk, skewed != 0);
  // the row limit: 0xFFFFFFFF is the searches' "no neighbour" marker
  CHECK(knn_add_fits(0xFFFFFFFDu, 1));
  CHECK(!knn_add_fits(0xFFFFFFFDu, 2));
  CHECK(!knn_add_fits(0xFFFFFFFEu, 1));
  CHECK(knn_add_fits(0xFFFFFFFEu, 0));
  CHECK(!knn_add_fits(0x80000000u, 0x80000000u));
  // refusals of knn_merge_offsets leave the output alone
  {
    std::vector<uint32_t> off = {0, 2, 5, 5}, out = {9};   // K = 2: [0,2) [2,5), no unclustered rows, 5 rows
    const uint32_t good[3] = {0, 1, 3}, bad_order[3] = {0, 3, 1}, bad_start[3] = {1, 1, 3}, too_many[3] = {0, 1, 9};
    CHECK(knn_merge_offsets(off, good, 2, 4, &out) && out == std::vector<uint32_t>({0, 3, 8, 9}));
    out = {9};
    CHECK(!knn_merge_offsets(off, bad_order, 2, 4, &out) && out == std::vector<uint32_t>({9}));
    CHECK(!knn_merge_offsets(off, bad_start, 2, 4, &out) && out == std::vector<uint32_t>({9}));
    CHECK(!knn_merge_offsets(off, too_many, 2, 4, &out) && out == std::vector<uint32_t>({9}));
    std::vector<uint32_t> short_off = {0, 2, 5};
    CHECK(!knn_merge_offsets(short_off, good, 2, 4, &out) && out == std::vector<uint32_t>({9}));
    std::vector<uint32_t> full = {0, 0, 0, 0xFFFFFFFEu};
    CHECK(!knn_merge_offsets(full, good, 2, 4, &out) && out == std::vector<uint32_t>({9}));
  }
  // the default chunk: within the budget, at least one row, never more than asked
  CHECK(knn_add_chunk_rows(1048576, 256, 256, (size_t)4 << 30, 0) == 1048576);
  CHECK(knn_add_chunk_rows(0xFFFFFFFEu, 256, 256, (size_t)4 << 30, 0) == ((size_t)4 << 30) / (256 * 10 + 48));
  CHECK(knn_add_chunk_rows(10, 1u << 30, 1u << 30, 1024, 0) == 1);
  CHECK(knn_add_chunk_rows(10, 64, 64, (size_t)4 << 30, 3) == 3);
  // the helper under it, which the query, probe and radius calls size their chunks with
  {
    const size_t budget = (size_t)4 << 30;
    CHECK(knn_chunk_rows(1024, 4096, 0, 10) == 1);    // a budget smaller than one row
    CHECK(knn_chunk_rows(budget, 12, 1000, 37) == 37);   // a forced value above the row count
    CHECK(knn_chunk_rows(budget, 12, 5, 37) == 5);
    CHECK(knn_chunk_rows(budget, 12, 0, 0) == 0);     // no rows
    CHECK(knn_chunk_rows(budget, 12, 7, 0) == 0);
    CHECK(knn_chunk_rows(1024, 4096, 0, 0) == 0);
    // bytes per query: K + 2k floats (query: lb and heaps), pw + 2k (probe: lists and heaps; pw <= min(K, 64)), K
    // (radius: lb) -- against the arithmetic the three calls used to spell out
    auto spelled_out = [&](size_t row_bytes, size_t forced, uint32_t Q) {
      size_t chunk = budget / row_bytes;
      if (forced) chunk = forced;
      if (chunk < 1) chunk = 1;
      return (uint32_t)(chunk < Q ? chunk : Q);
    };
    const size_t Ks[2] = {1, (size_t)1 << 20}, ks[2] = {1, 65535}, pws[2] = {1, 64};
    const uint32_t want[2][3] = {{357913941u, 357913941u, 1073741824u}, {910u, 8188u, 1024u}};
    for (int i = 0; i < 2; i++) {
      const size_t terms[3] = {4 * (Ks[i] + 2 * ks[i]), 4 * (pws[i] + 2 * ks[i]), 4 * Ks[i]};
      for (int t = 0; t < 3; t++)
        for (uint32_t Q : {0u, 1u, 909u, 910u, 911u, 8188u, 8189u, 0xFFFFFFFEu})
          for (size_t forced : {(size_t)0, (size_t)37}) {
            CHECK(knn_chunk_rows(budget, terms[t], forced, Q) == spelled_out(terms[t], forced, Q));
            if (!forced && Q == 0xFFFFFFFEu) CHECK(knn_chunk_rows(budget, terms[t], 0, Q) == want[i][t]);
          }
    }
  }
  // the chunk of a radius fill whose hits are staged: halved until its CSR range fits
  {
    const uint64_t offs[8] = {0, 10, 20, 30, 40, 50, 60, 70};
    CHECK(knn_fill_chunk_rows(offs, 0, 7, 70) == 7);   // fits as it is
    CHECK(knn_fill_chunk_rows(offs, 2, 5, 50) == 5);   // (from q0 on: offs[7] - offs[2])
    CHECK(knn_fill_chunk_rows(offs, 0, 7, 69) == 4);   // one halving of an odd n rounds up
    CHECK(knn_fill_chunk_rows(offs, 0, 7, 15) == 1);   // 7 -> 4 -> 2 -> 1
    CHECK(knn_fill_chunk_rows(offs, 0, 7, 20) == 2);
    CHECK(knn_fill_chunk_rows(offs, 3, 4, 25) == 2);
    CHECK(knn_fill_chunk_rows(offs, 0, 1, 0) == 1);    // a single query larger than the budget stays
    CHECK(knn_fill_chunk_rows(offs, 6, 1, 9) == 1);
    CHECK(knn_fill_chunk_rows(offs, 0, 5, 0) == 1);
    const uint64_t empty[4] = {5, 5, 5, 5};
    CHECK(knn_fill_chunk_rows(empty, 0, 3, 0) == 3);   // empty ranges fit any budget
    // offsets near 2^63 and above: the difference is what counts
    const uint64_t top = (uint64_t)1 << 63;
    const uint64_t big[6] = {top - 3, top - 1, top, top + 4, top + 4, top + 9};
    CHECK(knn_fill_chunk_rows(big, 0, 5, 12) == 5);
    CHECK(knn_fill_chunk_rows(big, 0, 5, 11) == 3);    // big[3] - big[0] = 7
    CHECK(knn_fill_chunk_rows(big, 0, 5, 6) == 2);     // 5 -> 3 -> 2: big[2] - big[0] = 3
    CHECK(knn_fill_chunk_rows(big, 1, 4, 5) == 2);     // 4 -> 2: big[3] - big[1] = 5
    // against the loop the radius call used to spell out, at every start, length and budget of a random CSR
    std::mt19937 rng(5);
    std::vector<uint64_t> o(41, top - 100);
    for (size_t i = 1; i < o.size(); i++) o[i] = o[i - 1] + rng() % 9;
    for (uint32_t q0 = 0; q0 < 40; q0++)
      for (uint32_t n0 = 1; q0 + n0 <= 40; n0++)
        for (uint64_t budget : {(uint64_t)0, (uint64_t)1, (uint64_t)7, (uint64_t)40, (uint64_t)1000}) {
          uint32_t n = n0;
          while (n > 1 && (o[q0 + n] - o[q0]) > budget) n = (n + 1) / 2;
          CHECK(knn_fill_chunk_rows(o.data(), q0, n0, budget) == n);
        }
  }
  printf(failures ? "%d checks FAILED\n" : "knn_merge_host_check: all checks passed\n", failures);
  return failures ? 1 : 0;
}
