#!/usr/bin/env python
"""k-NN of NEW rows against a clustered corpus (kmcuda_amd.KnnIndex) at the BASELINE config D shape: the corpus is
config_d.py's (N x 256 Gaussian mixture of K = 1024 unit Gaussians, centres uniform in [0,10)^D, same seed, clustered
by kmeans_cuda with the same settings), the queries are `--queries` FRESH draws from the same mixture, k = 10.
Reports the index build and the query time separately, then checks `--check` queries against a float64 torch brute
force (a list may differ from it only where two candidates tie within fp32 rounding).

--max-distance R | pNN: the capped search beside the uncapped one -- R a distance, pNN the NN-th
percentile of the uncapped call's k-th distances on the same batch (--cap-k: of the distances to the cap-k-th
neighbour instead, for "k = 100 capped at the median 10th-neighbour distance").  After the warm-up the two calls
alternate `--repeat` times in this one run; then the KMCUDA_AMD_KNN_STATS counters of both (the uncapped one's through
the capped entry point at FLT_MAX, which is the same search) and the mean number of real entries.  --radius also times
query_radius(R, sort=True), the alternative a caller has without the cap.

The matching knn_cuda() figure -- the same number of queries through the self-join -- is
    python scripts/config_d.py --samples 8000000 --shard 0/8   (1M of the 8M rows)"""
import argparse
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
    ap.add_argument("--check", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=2, help="query calls (the first one includes warm-up)")
    ap.add_argument("--max-distance", default=None, help="a distance, or pNN: a percentile of the k-th distances")
    ap.add_argument("--cap-k", type=int, default=None, help="pNN is taken over the distances to this neighbour")
    ap.add_argument("--nprobe", type=int, default=None, help="with --max-distance: the probed search")
    ap.add_argument("--radius", action="store_true", help="with --max-distance: time query_radius(sort=True) too")
    args = ap.parse_args()
    import torch
    from kmcuda_amd import KnnIndex, kmeans_cuda
    from kmcuda_amd.api import _DEVICE_ALLOCS
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    n, d, K, Q, k = args.samples, args.features, args.clusters, args.queries, args.k
    # the corpus exactly as scripts/config_d.py draws it (--data gaussian --sigma 1)
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    centres = torch.rand((K, d), device=dev, generator=gen) * 10.0
    for s in range(0, n, 1 << 20):
        e = min(n, s + (1 << 20))
        lab = torch.randint(0, K, (e - s,), device=dev, generator=gen)
        x[s:e].normal_(0.0, 1.0, generator=gen)
        x[s:e] += centres[lab]
    q = torch.empty((Q, d), dtype=torch.float32, device=dev)   # fresh draws from the same mixture
    for s in range(0, Q, 1 << 20):
        e = min(Q, s + (1 << 20))
        lab = torch.randint(0, K, (e - s,), device=dev, generator=gen)
        q[s:e].normal_(0.0, 1.0, generator=gen)
        q[s:e] += centres[lab]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cptr, aptr = kmeans_cuda((x.data_ptr(), 0, (n, d)), K, init="random", seed=777, tolerance=0.01, yinyang_t=0,
                             device=1, verbosity=0)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    # kmeans_cuda's device results are torch tensors the module keeps alive (centroids K x d, assignments n)
    cen, asg = _DEVICE_ALLOCS[cptr], _DEVICE_ALLOCS[aptr]
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    ix = KnnIndex(x, cen, asg)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    times = []
    for _ in range(max(1, args.repeat)):
        torch.cuda.synchronize()
        ta = time.perf_counter()
        nb, dist = ix.query(q, k)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - ta)
    print("kmeans_cuda %.3f s; KnnIndex build %.3f s; query %s s for %d queries (k=%d) => %.3e lists/s" %
          (t1 - t0, t3 - t2, " / ".join("%.3f" % t for t in times), Q, k, Q / min(times)), flush=True)
    if args.max_distance is not None:
        capped_runs(args, torch, ix, q, k, dist)
    if args.check:
        rows = torch.randperm(Q, device=dev, generator=gen)[:args.check]
        qq = q[rows].double()
        best_d = torch.full((len(rows), k), float("inf"), dtype=torch.float64, device=dev)
        best_i = torch.zeros((len(rows), k), dtype=torch.int64, device=dev)
        for s in range(0, n, 1 << 20):
            e = min(n, s + (1 << 20))
            xb = x[s:e].double()
            d2 = (qq * qq).sum(1, keepdim=True) + (xb * xb).sum(1)[None, :] - 2.0 * qq @ xb.T
            dd, ii = torch.topk(d2, k, dim=1, largest=False)
            cat_d, cat_i = torch.cat([best_d, dd], 1), torch.cat([best_i, ii + s], 1)
            best_d, sel = torch.topk(cat_d, k, dim=1, largest=False)
            best_i = torch.gather(cat_i, 1, sel)
        got = nb[rows].to(torch.int64) & 0xFFFFFFFF
        got_d2 = ((x[got].double() - qq[:, None, :]) ** 2).sum(2)
        ref_d2 = best_d
        tol = 1e-5 * torch.clamp(ref_d2, min=1.0)
        bad = ((got != best_i) & ((got_d2 - ref_d2).abs() > tol)).any(1)
        dd_err = (dist[rows].double() ** 2 - got_d2).abs() / torch.clamp(got_d2, min=1.0)
        print("brute-force check (float64): %d of %d queries differ; max relative error of the returned squared "
              "distances %.2e" % (int(bad.sum()), len(rows), float(dd_err.max())), flush=True)
    ix.close()


def capped_runs(args, torch, ix, q, k, dist):
    """The capped call against the uncapped one, alternating; the counters of both; the real entries."""
    kw = {} if args.nprobe is None else {"nprobe": args.nprobe}
    if args.max_distance.startswith("p"):
        col = (args.cap_k or k) - 1
        base = dist if args.nprobe is None else ix.query(q, k, **kw)[1]
        kth = base[:, col]
        cap = float(torch.quantile(kth[kth < 3.0e38][:4000000].double(), float(args.max_distance[1:]) / 100.0))
    else:
        cap = float(args.max_distance)
    ix.query(q, k, max_distance=cap, **kw)   # warm-up
    t_cap, t_plain = [], []
    for _ in range(max(1, args.repeat)):
        for times, extra in ((t_cap, {"max_distance": cap}), (t_plain, {})):
            torch.cuda.synchronize()
            ta = time.perf_counter()
            res = ix.query(q, k, **kw, **extra)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - ta)
    counts = ix.query(q, k, max_distance=cap, return_counts=True, **kw)[-1]
    fmt = lambda ts: " / ".join("%.3f" % t for t in ts)   # noqa: E731
    print("max_distance %.6g (%s%s): capped %s s; uncapped %s s; mean real entries %.2f of k=%d" % (
        cap, args.max_distance, "" if args.nprobe is None else ", nprobe=%d" % args.nprobe, fmt(t_cap), fmt(t_plain),
        float(counts.double().mean()), k), flush=True)
    os.environ["KMCUDA_AMD_KNN_STATS"] = "1"   # the library prints the counters at the end of a capped call
    print("counters, capped then uncapped (FLT_MAX through the capped entry point):", flush=True)
    ix.query(q, k, max_distance=cap, **kw)
    ix.query(q, k, max_distance=float("inf"), **kw)
    del os.environ["KMCUDA_AMD_KNN_STATS"]
    if args.radius:
        times = []
        for _ in range(max(1, args.repeat)):
            torch.cuda.synchronize()
            ta = time.perf_counter()
            offsets, _, _ = ix.query_radius(q, cap, sort=True)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - ta)
        print("query_radius(%.6g, sort=True): %s s; %.2f hits per query before the cut to k" % (
            cap, fmt(times), float(offsets[-1]) / len(q)), flush=True)


if __name__ == "__main__":
    main()
