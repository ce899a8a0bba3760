// knn_job.cpp -- knn_cuda()'s host side (reference: knn_cuda, kmcuda.cc:572-730 + knn_cuda_calc, knn.cu:381-532).
// Every GPU of the mask holds the whole corpus (as in the reference, kmcuda.cc:593-598) in CLUSTER-SORTED order and
// searches a contiguous slice of the sorted positions; there is no data-path collective.  The small replicated pieces
// (radii, K x K centroid distances) are recomputed on every GPU instead of exchanged.  The steps themselves are the
// shared ones of knn_host.cpp; this file plans the shares and brings the lists back in sample order.
#include <stdio.h>
#include <string.h>

#include <memory>

#include "knn_host.hpp"

#define INFO(...) do { if (verbosity > 0) { printf(__VA_ARGS__); } } while (false)
#define DEBUG(...) do { if (verbosity > 1) { printf(__VA_ARGS__); } } while (false)

namespace kmx {
namespace {

class KnnJob {
 public:
  KnnJob(uint32_t k_, const KnnCorpus &corpus, int verbosity_, uint32_t *neighbors_)
      : c(corpus), k(k_), verbosity(verbosity_), neighbors(neighbors_), sw(knn_switches()) {}

  int run(const std::vector<int> &devs, int nvirtual) {
    plan_shares(devs, nvirtual);
    KNN_TRY(prepare());
    plan_blocks();
    KNN_TRY(search());
    return gather_outputs();
  }

 private:
  const KnnCorpus &c;
  const uint32_t k;
  const int verbosity;
  uint32_t *const neighbors;
  const KnnSwitches sw;
  KnnPath path;
  std::vector<std::unique_ptr<KnnShard>> shards;
  size_t plan_shards = 0, plan_first = 0;   // this call runs shares [plan_first, plan_first + shards.size()) of plan_shards
  std::vector<uint32_t> offsets, blocks;    // the CSR of the corpus; (cluster, first position) per block
  uint32_t assigned = 0;                    // positions >= assigned belong to no cluster (NaN samples)

  // one shard per GPU of the mask
  void plan_shares(const std::vector<int> &devs, int nvirtual) {
    std::vector<int> shard_devs = devs;
    if (nvirtual > 1 && devs.size() == 1) shard_devs.assign(nvirtual, devs[0]);  // test hook
    plan_shards = shard_devs.size();
    // measurement hook KMCUDA_AMD_KNN_SHARD="i/n": plan the queries for n GPUs but run ONLY share i, on the
    // first GPU of the mask (what one rank of an n-GPU search does: whole corpus resident, 1/n of the
    // queries); the other rows of `neighbors` are left untouched
    if (sw.shard_n) {
      plan_shards = sw.shard_n;
      plan_first = sw.shard_i;
      shard_devs.assign(1, devs[0]);
    }
    for (int dev : shard_devs) {
      shards.push_back(std::make_unique<KnnShard>());
      shards.back()->dev = dev;
    }
  }

  // per GPU: inverse assignments, sorted copy, radii, centroid distances
  int prepare() {
    path = knn_choose_path(c.D, c.fp16, verbosity, sw);
    // (the reference's progress lines, kept as a caller sees them; the three steps are one enqueue here)
    INFO("initializing the inverse assignments...\n");
    INFO("calculating the cluster radiuses...\n");
    INFO("calculating the centroid distance matrix...\n");
    std::vector<KnnShard *> all;
    for (auto &s : shards) all.push_back(s.get());
    offsets.resize((size_t)c.K + 1);
    bool left_half_range = false;
    KNN_TRY(knn_prepare_corpus(all.data(), all.size(), c, false, &path, &left_half_range, offsets.data()));
    if (left_half_range)
      INFO("k-NN: a centred row leaves the half range, %s\n",
           path.dp_filter ? "the f32 matrix-core filter instead of the f16 one" : "every candidate is evaluated with the exact arithmetic");
    return 0;
  }

  // the block list, and each shard's contiguous run of it
  void plan_blocks() {
    knn_block_plan(offsets.data(), c.K, knn_qpb(path.use_f16, path.DP), &blocks);
    const uint32_t total_blocks = (uint32_t)(blocks.size() / 2);
    assigned = offsets[c.K];
    for (size_t si = 0; si < shards.size(); si++) {
      KnnShard &s = *shards[si];
      const size_t i = plan_first + si;
      s.first_block = (uint32_t)((uint64_t)total_blocks * i / plan_shards);
      const uint32_t next = (uint32_t)((uint64_t)total_blocks * (i + 1) / plan_shards);
      s.nblocks = next - s.first_block;
      s.p_base = s.nblocks ? blocks[2 * (size_t)s.first_block + 1] : assigned;
      s.p_end = next < total_blocks ? blocks[2 * (size_t)next + 1] : assigned;
      if (!s.nblocks) s.p_end = s.p_base;
      if (i + 1 == plan_shards && !path.dp_filter) s.p_end = c.N;  // the exact kernel also fills the unassigned rows
    }
  }

  int search() {
    INFO("searching for the nearest neighbors...\n");
    for (auto &sp : shards) {
      KnnShard &s = *sp;
      (void)hipSetDevice(s.dev);
      const uint32_t len = s.p_end - s.p_base;
      KNN_TRY(s.alloc(&s.heaps, (size_t)len * 2 * k));
      KNN_TRY(s.alloc(&s.out, (size_t)len * k));
      std::vector<uint32_t> plan(blocks.begin() + 2 * (size_t)s.first_block,
                                 blocks.begin() + 2 * (size_t)(s.first_block + s.nblocks));
      if (path.use_f16 && s.nblocks >= 64 && sw.xcd) plan = knn_xcd_plan(plan);
      KNN_TRY(s.alloc(&s.blocks, plan.size() ? plan.size() : 2));
      if (!plan.empty())
        KMX_HIPCP(hipMemcpy(s.blocks, plan.data(), plan.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
      KnnArgs a;
      a.blocks = s.blocks; a.k = k; a.p_base = s.p_base; a.p_end = s.p_end; a.heaps = s.heaps; a.out = s.out;
      s.scratch.rows = len;
      KNN_TRY(knn_search(s, s.scratch, a, path, sw, (uint32_t)(plan.size() / 2), true, verbosity, nullptr));
    }
    return 0;
  }

  // rows back in sample order
  int gather_outputs() {
    const uint32_t N = c.N;
    const int32_t device_ptrs = c.device_ptrs;
    // rows without a cluster (NaN samples) get no neighbours: 0xFFFFFFFF.  The filters' blocks cover the assigned
    // positions only; the rows behind them are written here, by the call that runs the last share of the plan (with
    // KMCUDA_AMD_KNN_SHARD, a call that does not leaves them untouched like every row of the other shares)
    const bool fill_unassigned = path.dp_filter && assigned < N && plan_first + shards.size() == plan_shards;
    unsigned long long dists_calced = 0;
    std::vector<uint32_t> host_inv, host_out;
    if (device_ptrs < 0) {
      host_inv.resize(N);
      KnnShard &f = *shards[0];
      (void)hipSetDevice(f.dev);
      KMX_HIPCP(hipMemcpy(host_inv.data(), f.inv, (size_t)N * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    for (auto &sp : shards) {
      KnnShard &s = *sp;
      (void)hipSetDevice(s.dev);
      if (hipStreamSynchronize(s.stream) != hipSuccess) {
        INFO("k-NN kernel failed: %s\n", hipGetErrorString(hipGetLastError()));
        return kmcudaRuntimeError;
      }
      unsigned long long cs[KNN_STATS] = {0, 0, 0, 0, 0};
      KMX_HIPCP(hipMemcpy(cs, s.calced, sizeof(cs), hipMemcpyDeviceToHost));
      DEBUG("#%d dists_calced: %llu\n", s.dev, cs[0]);
      // what the f16 search actually did (knn_f16.hip; measurement: KMCUDA_AMD_KNN_STATS=1 prints it at any verbosity)
      if (cs[1] && (verbosity > 1 || sw.stats))
        printf("#%d k-NN filter: %llu pairs by the reference's prune rule, %llu scored on the matrix cores "
               "(%llu of them live query x real candidate; %llu if an operand set nobody visits with were skipped), "
               "%llu exact chains\n", s.dev, cs[0], cs[1], cs[2], cs[4], cs[3]);
      dists_calced += cs[0];
      const uint32_t len = s.p_end - s.p_base;
      if (!len) continue;
      if (device_ptrs < 0) {
        host_out.resize((size_t)len * k);
        KMX_HIPCP(hipMemcpy(host_out.data(), s.out, (size_t)len * k * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < len; i++)
          memcpy(neighbors + (size_t)host_inv[s.p_base + i] * k, host_out.data() + (size_t)i * k, k * sizeof(uint32_t));
      } else {
        KNN_TRY(knn_scatter_on(device_ptrs, s.dev, s.out, s.inv, N, s.p_base, s.p_end, k, neighbors));
      }
    }
    if (fill_unassigned && device_ptrs < 0) {  // (the reference reads out of bounds for these rows)
      for (uint32_t p = assigned; p < N; p++)
        for (uint32_t i = 0; i < k; i++) neighbors[(size_t)host_inv[p] * k + i] = UINT32_MAX;
    } else if (fill_unassigned) {
      const KnnShard &l = *shards.back();
      KNN_TRY(knn_scatter_on(device_ptrs, l.dev, nullptr, l.inv, N, assigned, N, k, neighbors));
    }
    INFO("calculated %f of all the distances\n", (dists_calced + .0) / ((double)N * N));  // knn.cu:529-530
    return 0;
  }
};

}  // namespace

int knn_job_run(const std::vector<int> &devs, int nvirtual, uint32_t k, const KnnCorpus &corpus, int verbosity,
                uint32_t *neighbors) {
  return KnnJob(k, corpus, verbosity, neighbors).run(devs, nvirtual);
}

}  // namespace kmx
