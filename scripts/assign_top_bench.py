#!/usr/bin/env python
"""kmeans_predict_top (kmamd_kmeans_assign_top) on one GPU: device-resident `--samples` x `--features`
fp32 rows (uniform in [0,1)) against `--clusters` centroids drawn from the rows.  GPU only: it fails without a device.
Per m of `--m`, host clock around calls that wait for the device, medians of `--repeat` calls after `--warmup`:

  filtered   the default call (the f32 matrix-core filter in front of the exact keys), with pairs_exact / pairs_total
             of kmamd_assign_top_stats
  exact      the same call with KMCUDA_AMD_ASSIGN_TOP=exact (the exhaustive exact kernel alone; `--repeat-exact` calls)

and, once: a bare kmeans_predict (the floor: one assignment pass, one winner per row) and one
kmamd_lloyd_assign_exact pass at the same shape (the yardstick: the same exhaustive exact distance work).
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--m", default="1,8,64")
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--repeat-exact", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--metric", default="L2")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("assign_top_bench.py needs a GPU")
    from kmcuda_amd import _lib, kmeans_predict, kmeans_predict_top
    from kmcuda_amd.engine import Engine
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(4321)
    n, d, K = args.samples, args.features, args.clusters
    x = torch.rand((n, d), dtype=torch.float32, device=dev, generator=gen)
    if args.metric == "angular":
        x /= x.norm(dim=1, keepdim=True)
    cen = x[torch.randperm(n, device=dev, generator=gen)[:K]].contiguous()
    print("%s: %d x %d fp32 rows, %d centroids" % (args.metric, n, d, K), flush=True)

    def timed(fn, reps, warmup):
        ts = []
        for i in range(warmup + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    def report(name, t, extra=""):
        print("  %-34s median %9.3f ms (min %.3f, max %.3f)%s" % (name, t[0], t[1], t[2], extra), flush=True)

    report("kmeans_predict (the floor)", timed(lambda: kmeans_predict(x, cen, metric=args.metric), args.repeat,
                                               args.warmup))
    eng = Engine(n, d, K, args.metric, device=0)
    asg = torch.full((n,), K, dtype=torch.int32, device=dev)
    prev = torch.empty((n,), dtype=torch.int32, device=dev)

    def exact_pass():
        eng.lloyd_assign(x, cen, asg, prev, exact=True)
        eng.sync()
    t_yard = timed(exact_pass, args.repeat_exact, 1)
    report("kmamd_lloyd_assign_exact pass", t_yard)
    eng.close()
    del eng, asg, prev

    for m in (int(v) for v in args.m.split(",")):
        res = {}

        def call():
            res["out"] = kmeans_predict_top(x, cen, m, metric=args.metric)
        t = timed(call, args.repeat, args.warmup)
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        L.kmamd_assign_top_stats(ctypes.byref(a), ctypes.byref(b))
        report("m = %2d filtered" % m, t, "; pairs_exact / pairs_total = %d / %d = %.5f; %s the exact pass" % (
            a.value, b.value, a.value / max(b.value, 1), "faster than" if t[0] < t_yard[0] else "NOT faster than"))
        filtered = res["out"]
        os.environ["KMCUDA_AMD_ASSIGN_TOP"] = "exact"
        try:
            report("m = %2d KMCUDA_AMD_ASSIGN_TOP=exact" % m, timed(call, args.repeat_exact, 1))
        finally:
            os.environ.pop("KMCUDA_AMD_ASSIGN_TOP", None)
        same = bool((res["out"][0] == filtered[0]).all()) and bool(
            (res["out"][1].view(torch.int32) == filtered[1].view(torch.int32)).all())
        print("  m = %2d same bits on both paths: %s" % (m, same), flush=True)
        del filtered, res


if __name__ == "__main__":
    main()
