#!/usr/bin/env python
"""Filtered search of the k-NN index (KnnIndex.query(allow=)) at the BASELINE config D shape, on
scripts/knn_query_bench.py's corpus and queries (N x 256 Gaussian mixture of K = 1024 unit Gaussians, clustered by
kmeans_cuda; `--queries` fresh draws; k = 10; everything device-resident).

For the exact query() and for query(nprobe=`--nprobe`), at every allowed fraction of `--fractions` (random rows), in ONE
process:
  * masked: index.query(..., allow=mask);
  * (a) the unmasked call of the same build;
  * (b) what a caller can do without the mask: KnnIndex(rows[mask], centroids, assignments[mask]) built (timed once)
    and queried;
  * the mask preparation alone: index.radii_allow(mask), i.e. the pack, the member distances and the masked radii, plus
    a copy of K floats.
After one warm-up call of every arm, `--repeat` rounds alternate the arms, host clock around a call that ends in a
synchronise; all raw times and their minimum are printed, one JSON line per arm.  `--unmasked-only`: the unmasked arms
alone (for a run against another build of the library)."""
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
    ap.add_argument("--nprobe", type=int, default=4)
    ap.add_argument("--fractions", type=float, nargs="+", default=[1.0, 0.5, 0.1, 0.01])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--unmasked-only", action="store_true")
    args = ap.parse_args()
    import torch
    from kmcuda_amd import KnnIndex, kmeans_cuda
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
    modes = [("query", None), ("nprobe=%d" % args.nprobe, args.nprobe)]

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    def report(arm, times, **more):
        best = min(times)
        line = {"arm": arm, "queries": Q, "k": k, "seconds": [round(t, 4) for t in times], "best_seconds": round(best, 4)}
        line.update(more)
        print(json.dumps(line), flush=True)

    # ---- (a) the unmasked calls ----
    arms = {}
    for name, p in modes:
        arms[name] = (lambda p=p: ix.query(q, k, nprobe=p, return_distances=False))
    if not args.unmasked_only:
        masks = {}
        for f in args.fractions:
            m = torch.rand((n,), device=dev, generator=gen) < f if f < 1.0 else torch.ones((n,), dtype=torch.bool, device=dev)
            masks[f] = m
            for name, p in modes:
                arms["%s allow=%g" % (name, f)] = (lambda p=p, m=m: ix.query(q, k, nprobe=p, return_distances=False, allow=m))
            arms["mask preparation %g" % f] = (lambda m=m: ix.radii_allow(m))
    for fn in arms.values():   # warm-up
        timed(fn)
    times = {name: [] for name in arms}
    for _ in range(max(1, args.repeat)):
        for name, fn in arms.items():
            times[name].append(timed(fn)[0])
    for name in arms:
        report(name, times[name])
    if args.unmasked_only:
        ix.close()
        return

    # ---- (b) an index on the allowed subset, one fraction at a time (its copies go before the next is built) ----
    for f in args.fractions:
        rows = torch.nonzero(masks[f]).squeeze(1)
        t_copy, (xs, as_) = timed(lambda: (x[rows].contiguous(), asg[rows].contiguous()))
        t_build, sub = timed(lambda: KnnIndex(xs, cen, as_))
        for name, p in modes:
            fn = (lambda p=p: sub.query(q, k, nprobe=p, return_distances=False))
            timed(fn)
            ts = [timed(fn)[0] for _ in range(max(1, args.repeat))]
            report("%s on a subset index %g" % (name, f), ts, rows=int(rows.numel()), gather_seconds=round(t_copy, 4),
                   build_seconds=round(t_build, 4))
        # the masked lists are the subset index's, row ids aside
        got = ix.query(q[:10000], k, return_distances=False, allow=masks[f]).to(torch.int64) & 0xFFFFFFFF
        want = rows[sub.query(q[:10000], k, return_distances=False).to(torch.int64) & 0xFFFFFFFF]
        print(json.dumps({"check": "masked lists equal the subset index's", "fraction": f,
                          "equal": bool((got == want).all())}), flush=True)
        sub.close()
        del xs, as_, sub, rows
        torch.cuda.empty_cache()
    ix.close()


if __name__ == "__main__":
    main()
