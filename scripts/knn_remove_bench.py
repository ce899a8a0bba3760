#!/usr/bin/env python
"""Rows removed from a k-NN index in place (KnnIndex.remove) at the BASELINE config D shape, on
scripts/knn_query_bench.py's corpus (N x 256 Gaussian mixture of K = 1024 unit Gaussians, clustered by kmeans_cuda;
everything device-resident), in ONE process:

  * for every list length of `--remove`: KnnIndex(corpus) + remove(random distinct ids, a device tensor), the remove
    timed with the host clock around a call that ends in a synchronise, `--repeat` times on a fresh index each (after
    one warm-up); one more remove under KMCUDA_AMD_KNN_REMOVE_TIME=1, whose line (HIP events: assignments, sort, copy
    and its bytes per second, member distances and radii) the library prints and this script echoes; the copy's rate
    against the 6.29 TB/s float4 copy of the MI355X;
  * KnnIndex(corpus, centroids, patched assignments) from the same device-resident buffers -- the only way to get that
    index without remove -- timed the same way;
  * one query() of `--queries` rows on both: the two indexes must answer alike.
Prints one JSON line per list length at the end."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_TBS = 6.29   # float4 copy, measured (MI355X)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=8000000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--remove", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    import torch
    from kmcuda_amd import KnnIndex, kmeans_cuda
    from kmcuda_amd.api import _DEVICE_ALLOCS
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    n, d, K, Q, k = args.samples, args.features, args.clusters, args.queries, args.k
    centres = torch.rand((K, d), device=dev, generator=gen) * 10.0

    def draw(rows):
        out = torch.empty((rows, d), dtype=torch.float32, device=dev)
        for s in range(0, rows, 1 << 20):
            e = min(rows, s + (1 << 20))
            lab = torch.randint(0, K, (e - s,), device=dev, generator=gen)
            out[s:e].normal_(0.0, 1.0, generator=gen)
            out[s:e] += centres[lab]
        return out

    x, q = draw(n), draw(Q)
    cptr, aptr = kmeans_cuda((x.data_ptr(), 0, (n, d)), K, init="random", seed=777, tolerance=0.01, yinyang_t=0,
                             device=1, verbosity=0)
    cen, asg = _DEVICE_ALLOCS[cptr], _DEVICE_ALLOCS[aptr]
    asg = asg.to(torch.int32)
    torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    reps = max(1, args.repeat)
    results = []
    for m in args.remove:
        ids = torch.randperm(n, device=dev, generator=gen)[:m].to(torch.int32)
        a_patched = asg.clone()
        a_patched[ids.to(torch.int64)] = K
        remove_s, create_s, rebuild_s, after_s, fresh_s = [], [], [], [], []
        for r in range(reps + 1):   # (round 0: warm-up)
            t_create, ix = timed(lambda: KnnIndex(x, cen, asg))
            if r == reps:
                os.environ["KMCUDA_AMD_KNN_REMOVE_TIME"] = "1"
            t_remove, lost = timed(lambda: ix.remove(ids))
            os.environ.pop("KMCUDA_AMD_KNN_REMOVE_TIME", None)
            sys.stdout.flush()
            assert lost == m and ix.info()[:2] == (n, n - m)
            ix.query(q, k)
            t_after, lists = timed(lambda: ix.query(q, k))
            ix.close()
            t_rebuild, ix2 = timed(lambda: KnnIndex(x, cen, a_patched))
            ix2.query(q, k)
            t_fresh, want = timed(lambda: ix2.query(q, k))
            if r == reps:   # the two indexes answer alike
                assert bool((want[0] == lists[0]).all()) and bool((want[1].view(torch.int32) == lists[1].view(torch.int32)).all())
            ix2.close()
            if r:
                remove_s.append(t_remove); create_s.append(t_create); rebuild_s.append(t_rebuild)
                after_s.append(t_after); fresh_s.append(t_fresh)
        results.append({
            "corpus": n, "features": d, "clusters": K, "removed": m,
            "remove_seconds": [round(t, 5) for t in remove_s], "remove_best": round(min(remove_s), 5),
            "create_corpus_seconds": [round(t, 5) for t in create_s],
            "rebuild_seconds": [round(t, 5) for t in rebuild_s], "rebuild_best": round(min(rebuild_s), 5),
            "rebuild_over_remove": round(min(rebuild_s) / min(remove_s), 2),
            "queries": Q, "k": k, "query_after_seconds": [round(t, 5) for t in after_s],
            "query_rebuilt_seconds": [round(t, 5) for t in fresh_s],
            "copy_reference_TBs": COPY_TBS,
        })
    for r in results:
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
