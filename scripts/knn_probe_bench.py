#!/usr/bin/env python
"""Multi-probe search of the k-NN index (KnnIndex.query(nprobe=)) at the BASELINE config D shape, on
scripts/knn_query_bench.py's corpus and queries (N x 256 Gaussian mixture of K = 1024 unit Gaussians, clustered by
kmeans_cuda; `--queries` fresh draws; k = 10; everything device-resident).

For every nprobe of `--nprobe` and for the exact query() of the same index, in ONE process:
  * the call time: after one warm-up call of every arm, `--repeat` rounds that alternate the arms, host clock around a
    call that ends in a synchronise; all raw times and their minimum are printed;
  * the KMCUDA_AMD_KNN_STATS counters of one call (the library prints them; echoed as they come);
  * recall@k against the exact query()'s lists on `--check` of the queries;
  * the ranking's share: kmeans_predict_top(queries, centroids, nprobe) timed alone the same way.
Prints one JSON line per arm at the end."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=8000000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--queries", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--check", type=int, default=10000)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    import torch
    from kmcuda_amd import KnnIndex, kmeans_cuda, kmeans_predict_top
    from kmcuda_amd.api import _DEVICE_ALLOCS
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    n, d, K, Q, k = args.samples, args.features, args.clusters, args.queries, args.k
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    centres = torch.rand((K, d), device=dev, generator=gen) * 10.0
    for s in range(0, n, 1 << 20):
        e = min(n, s + (1 << 20))
        lab = torch.randint(0, K, (e - s,), device=dev, generator=gen)
        x[s:e].normal_(0.0, 1.0, generator=gen)
        x[s:e] += centres[lab]
    q = torch.empty((Q, d), dtype=torch.float32, device=dev)
    for s in range(0, Q, 1 << 20):
        e = min(Q, s + (1 << 20))
        lab = torch.randint(0, K, (e - s,), device=dev, generator=gen)
        q[s:e].normal_(0.0, 1.0, generator=gen)
        q[s:e] += centres[lab]
    cptr, aptr = kmeans_cuda((x.data_ptr(), 0, (n, d)), K, init="random", seed=777, tolerance=0.01, yinyang_t=0,
                             device=1, verbosity=0)
    cen, asg = _DEVICE_ALLOCS[cptr], _DEVICE_ALLOCS[aptr]
    torch.cuda.synchronize()
    ix = KnnIndex(x, cen, asg)
    arms = [None] + [p for p in args.nprobe if 1 <= p <= min(K, 64)]

    def call(p):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = ix.query(q, k, return_distances=False) if p is None else ix.query(q, k, nprobe=p, return_distances=False)
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    def rank(p):
        torch.cuda.synchronize()
        t = time.perf_counter()
        kmeans_predict_top(q, cen, p, return_distances=False)
        torch.cuda.synchronize()
        return time.perf_counter() - t

    lists = {}
    for p in arms:   # warm-up; the lists for the recall
        _, lists[p] = call(p)
        if p is not None:
            rank(p)
    times = {p: [] for p in arms}
    ranks = {p: [] for p in arms if p is not None}
    for _ in range(max(1, args.repeat)):
        for p in arms:
            times[p].append(call(p)[0])
            if p is not None:
                ranks[p].append(rank(p))
    # the counters, one call per arm (the library prints its line at the end of the call)
    os.environ["KMCUDA_AMD_KNN_STATS"] = "1"
    for p in arms:
        print("counters, %s:" % ("exact query" if p is None else "nprobe %d" % p), flush=True)
        if p is None:
            print("  (query() prints none: DESIGN.md 4.7 has the exact search's figures)", flush=True)
        else:
            call(p)
        sys.stdout.flush()
    del os.environ["KMCUDA_AMD_KNN_STATS"]
    rows = torch.randperm(Q, device=dev, generator=gen)[:min(args.check, Q)]
    want = (lists[None][rows].to(torch.int64) & 0xFFFFFFFF)
    for p in arms:
        rec = None
        if p is not None:
            got = (lists[p][rows].to(torch.int64) & 0xFFFFFFFF)
            rec = float((got[:, :, None] == want[:, None, :]).any(2).float().mean())
        best = min(times[p])
        print(json.dumps({
            "arm": "query" if p is None else "nprobe=%d" % p, "queries": Q, "k": k,
            "seconds": [round(t, 4) for t in times[p]], "best_seconds": round(best, 4),
            "lists_per_s": Q / best, "recall_at_k": rec,
            "ranking_seconds": None if p is None else [round(t, 4) for t in ranks[p]],
            "ranking_share": None if p is None else round(min(ranks[p]) / best, 3),
        }), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
