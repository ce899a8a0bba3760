#!/usr/bin/env python
"""Rows added to a k-NN index in place (KnnIndex.add) at the BASELINE config D shape, on
scripts/knn_query_bench.py's corpus (N x 256 Gaussian mixture of K = 1024 unit Gaussians, clustered by kmeans_cuda;
everything device-resident), in ONE process:

  * for every batch size of `--add`: KnnIndex(corpus) + add(batch), the add timed with the host clock around a call
    that ends in a synchronise, `--repeat` times on a fresh index each (after one warm-up); one more add under
    KMCUDA_AMD_KNN_ADD_TIME=1, whose line (HIP events: clusters, preparation, merge, the merge's bytes per second) the
    library prints and this script echoes; the merge's rate against the 6.29 TB/s float4 copy of the MI355X;
  * KnnIndex(corpus + batch) with kmeans_predict's assignments for the batch -- the only way to get that index
    without add -- timed the same way, and kmeans_predict(batch) alone;
  * one query() of `--queries` rows before and after the add (the same index object) and on the index of the
    concatenation: after the add it must take what it takes on that fresh index (the corpus has grown).
Prints one JSON line per batch size at the end."""
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
    ap.add_argument("--add", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    import torch
    from kmcuda_amd import KnnIndex, kmeans_cuda, kmeans_predict
    from kmcuda_amd.api import _DEVICE_ALLOCS
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    n, d, K, Q, k = args.samples, args.features, args.clusters, args.queries, args.k
    extra = max(args.add)
    centres = torch.rand((K, d), device=dev, generator=gen) * 10.0

    def draw(rows):
        out = torch.empty((rows, d), dtype=torch.float32, device=dev)
        for s in range(0, rows, 1 << 20):
            e = min(rows, s + (1 << 20))
            lab = torch.randint(0, K, (e - s,), device=dev, generator=gen)
            out[s:e].normal_(0.0, 1.0, generator=gen)
            out[s:e] += centres[lab]
        return out

    whole = draw(n + extra)   # (one buffer: the concatenation arm reads a prefix of it, no second copy of the corpus)
    x, q = whole[:n], draw(Q)
    cptr, aptr = kmeans_cuda((x.data_ptr(), 0, (n, d)), K, init="random", seed=777, tolerance=0.01, yinyang_t=0,
                             device=1, verbosity=0)
    cen, asg = _DEVICE_ALLOCS[cptr], _DEVICE_ALLOCS[aptr]
    torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    reps = max(1, args.repeat)
    results = []
    for m in args.add:
        b = whole[n:n + m]
        predict_s = [timed(lambda: kmeans_predict(b, cen))[0] for _ in range(reps + 1)][1:]
        a_b = kmeans_predict(b, cen)
        a_cat = torch.cat([asg.to(torch.int32), a_b])
        add_s, create_s, concat_s, before_s, after_s, fresh_s = [], [], [], [], [], []
        for r in range(reps + 1):   # (round 0: warm-up)
            t_create, ix = timed(lambda: KnnIndex(x, cen, asg))
            ix.query(q, k)
            t_before = timed(lambda: ix.query(q, k))[0]
            if r == reps:
                os.environ["KMCUDA_AMD_KNN_ADD_TIME"] = "1"
            t_add, first = timed(lambda: ix.add(b))
            os.environ.pop("KMCUDA_AMD_KNN_ADD_TIME", None)
            sys.stdout.flush()
            assert first == n and ix.info()[0] == n + m
            ix.query(q, k)
            t_after, lists = timed(lambda: ix.query(q, k))
            ix.close()
            t_concat, ix2 = timed(lambda: KnnIndex(whole[:n + m], cen, a_cat))
            ix2.query(q, k)
            t_fresh = timed(lambda: ix2.query(q, k))[0]
            if r == reps:   # the two indexes answer alike
                want = ix2.query(q, k)
                assert bool((want[0] == lists[0]).all()) and bool((want[1].view(torch.int32) == lists[1].view(torch.int32)).all())
            ix2.close()
            if r:
                add_s.append(t_add); create_s.append(t_create); concat_s.append(t_concat)
                before_s.append(t_before); after_s.append(t_after); fresh_s.append(t_fresh)
        results.append({
            "corpus": n, "features": d, "clusters": K, "added": m,
            "add_seconds": [round(t, 5) for t in add_s], "add_best": round(min(add_s), 5),
            "create_corpus_seconds": [round(t, 5) for t in create_s],
            "create_concatenation_seconds": [round(t, 5) for t in concat_s], "create_concatenation_best": round(min(concat_s), 5),
            "predict_batch_seconds": [round(t, 5) for t in predict_s],
            "concatenation_over_add": round((min(concat_s) + min(predict_s)) / min(add_s), 2),
            "queries": Q, "k": k, "query_before_seconds": [round(t, 5) for t in before_s],
            "query_after_seconds": [round(t, 5) for t in after_s],
            "query_concatenation_seconds": [round(t, 5) for t in fresh_s],
            "copy_reference_TBs": COPY_TBS,
        })
    for r in results:
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
