#!/usr/bin/env python3
"""knn_rerank and IvfPqIndex.search(refine=) on device-resident operands, on ivfpq_bench.py's index.

    python scripts/knn_rerank_bench.py                 # N=1M x 256, K=1024, M=32 x 8, Q=10000, k=10
    python scripts/knn_rerank_bench.py --rows 100000 --clusters 128 --queries 1000 --repeat 3

Data and index as scripts/ivfpq_bench.py.  Per R: knn_rerank over the shortlist search(k=R, nprobe=--shortlist-nprobe)
returns, against the torch composition on the same tensors (gather, difference, norm, topk) and the gather floor,
pairs * 4 D bytes at --copy-tbs (the measured copy rate of the chip).  Per nprobe: search without refine and with each
--refine factor, and recall@k of both against an exact torch brute force.  Every time is the median [min, max] of
--repeat runs behind a warm-up, by a host clock around calls that end in a device synchronise.  There is no CPU path."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from ivfpq_bench import _median_ms, exact_topk, recall  # noqa: E402


def torch_rerank(queries, rows, candidates, k, chunk=1000):
    import torch
    idx, dist = [], []
    for q0 in range(0, queries.shape[0], chunk):
        c = candidates[q0:q0 + chunk].long()
        d = (rows[c] - queries[q0:q0 + chunk, None, :]).norm(dim=2)
        best = torch.topk(d, k, dim=1, largest=False)
        idx.append(torch.gather(c, 1, best.indices))
        dist.append(best.values)
    return torch.cat(idx), torch.cat(dist)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--subspaces", type=int, default=32)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--candidates", default="40,160,256")
    ap.add_argument("--shortlist-nprobe", type=int, default=4)
    ap.add_argument("--nprobe", default="1,4,16,64")
    ap.add_argument("--refine", default="4,16")
    ap.add_argument("--train-rows", type=int, default=100000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--copy-tbs", type=float, default=6.29)
    args = ap.parse_args()
    import torch
    from kmcuda_amd import IvfPqIndex, ivfpq_train, knn_rerank
    if not torch.cuda.is_available():
        sys.exit("knn_rerank_bench needs a GPU")
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    n, d, kc, m, k, nq = args.rows, args.features, args.clusters, args.subspaces, args.k, args.queries
    gen = torch.Generator(device=dev).manual_seed(1)
    centres = 2 * torch.randn((kc, d), generator=gen, device=dev)

    def draw(count):
        labels = torch.randint(0, kc, (count,), generator=gen, device=dev)
        return centres[labels] + torch.randn((count, d), generator=gen, device=dev)
    rows = draw(n)
    books = ivfpq_train(rows[:args.train_rows].contiguous(), centres, m, max_iter=10, seed=1)
    index = IvfPqIndex(rows, centres, books, keep_rows=True)
    queries = draw(nq)
    truth = exact_topk(queries, rows, k)
    for r in (int(v) for v in args.candidates.split(",")):
        cand = index.search(queries, r, nprobe=args.shortlist_nprobe)[0]
        ours = _median_ms(lambda: knn_rerank(queries, rows, cand, k), args.repeat, sync)
        composed = _median_ms(lambda: torch_rerank(queries, rows, cand, k), args.repeat, sync)
        pairs = int((cand >= 0).sum())
        floor = pairs * 4 * d / (args.copy_tbs * 1e12) * 1e3
        same = float((knn_rerank(queries, rows, cand, k)[0].long() == torch_rerank(queries, rows, cand, k)[0]).float().mean())
        print(json.dumps({"knn_rerank": {"Q": nq, "R": r, "k": k, "valid_pairs": pairs}, "ms": ours,
                          "torch_composition_ms": composed, "torch_over_ours": composed[0] / ours[0],
                          "gather_floor_ms": floor, "fraction_of_floor": floor / ours[0],
                          "pairs_per_s": pairs / ours[0] * 1e3, "indices_equal_to_torch": same,
                          "note": "[median, min, max] of %d runs" % args.repeat}), flush=True)
    for nprobe in (int(v) for v in args.nprobe.split(",")):
        plain = _median_ms(lambda: index.search(queries, k, nprobe=nprobe), args.repeat, sync)
        line = {"search": {"Q": nq, "k": k, "nprobe": nprobe}, "plain_ms": plain,
                "plain_recall": recall(index.search(queries, k, nprobe=nprobe)[0], truth)}
        for f in (int(v) for v in args.refine.split(",")):
            line["refine_%d_ms" % f] = _median_ms(lambda: index.search(queries, k, nprobe=nprobe, refine=f),
                                                  args.repeat, sync)
            line["refine_%d_recall" % f] = recall(index.search(queries, k, nprobe=nprobe, refine=f)[0], truth)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
