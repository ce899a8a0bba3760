#!/usr/bin/env python
"""kmeans_predict (kmamd_kmeans_assign) on one GPU, device-resident `--samples` x `--features` fp32 rows
(uniform in [0,1), unit length under the angular metric) against `--clusters` centroids drawn from the rows.  GPU
only: it fails without a device.  Two measurements in one process, per metric:

(a) the distance pass alone (kmamd_assigned_distances) on the same rows and assignments: the LDS-tiled
    assigned_distance_kernel against member_distances_kernel (KMCUDA_AMD_ASSIGN_DIST=member, same build), `--repeat`
    launches of each IN ALTERNATION after `--warmup` of each, every launch bracketed by device events on its stream.
    Per variant: median time, N * D * 4 bytes over it, and the spread (max - min) of its repeats.  The tiled kernel
    "wins" only if its median is below the other's by more than the larger spread.
(b) the whole device-resident kmeans_predict call without and with distances, against one bare Engine.lloyd_assign pass
    (row cache off) on the same rows, again in alternation; host clock around calls that wait for the device.  The
    differences are what the call does beyond the bare assignment pass.
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
    ap.add_argument("--samples", type=int, default=8 << 20)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=20, help="timed launches / calls of each variant (at least 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--metrics", default="L2,angular")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("assign_bench.py needs a GPU")
    from kmcuda_amd import _lib, kmeans_predict
    from kmcuda_amd.api import _raise_for
    from kmcuda_amd.engine import Engine
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(4321)
    n, d, K, reps = args.samples, args.features, args.clusters, max(args.repeat, 20)
    vp = ctypes.c_void_p
    x = torch.rand((n, d), dtype=torch.float32, device=dev, generator=gen)
    pick = torch.randperm(n, device=dev, generator=gen)[:K]
    row_bytes = float(n) * d * 4

    def stats(ts):
        return statistics.median(ts), min(ts), max(ts)

    for metric in args.metrics.split(","):
        mid = 1 if metric == "angular" else 0
        if mid:
            x /= x.norm(dim=1, keepdim=True)
        cen = x[pick].contiguous()
        asg = kmeans_predict(x, cen, metric=metric)
        dist = {v: torch.empty((n,), dtype=torch.float32, device=dev) for v in ("tiled", "member")}
        torch.cuda.synchronize()
        print("%s: %d x %d fp32 rows, %d centroids, %d rows without a cluster" % (
            metric, n, d, K, int((asg == K).sum())), flush=True)

        # ---- (a) the distance kernels, alternating, device events ----
        def launch(variant):
            if variant == "member":
                os.environ["KMCUDA_AMD_ASSIGN_DIST"] = "member"
            try:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                _raise_for(L.kmamd_assigned_distances(mid, n, d, K, 0, vp(x.data_ptr()), vp(cen.data_ptr()),
                                                      vp(asg.data_ptr()), vp(dist[variant].data_ptr()), None),
                           "kmamd_assigned_distances")
                b.record()
            finally:
                os.environ.pop("KMCUDA_AMD_ASSIGN_DIST", None)
            return a, b
        for _ in range(args.warmup):
            for v in ("tiled", "member"):
                launch(v)
        torch.cuda.synchronize()
        events = {"tiled": [], "member": []}
        for _ in range(reps):
            for v in ("tiled", "member"):
                events[v].append(launch(v))
        torch.cuda.synchronize()
        same = bool((dist["tiled"].view(torch.int32) == dist["member"].view(torch.int32)).all())
        res = {}
        for v in ("tiled", "member"):
            ts = [a.elapsed_time(b) for a, b in events[v]]
            med, lo, hi = stats(ts)
            res[v] = (med, hi - lo)
            print("  (a) %-6s distance kernel: median %.3f ms (min %.3f, max %.3f, spread %.3f) over %d launches; "
                  "%.2f TB/s of row bytes" % (v, med, lo, hi, hi - lo, len(ts), row_bytes / (med * 1e-3) / 1e12), flush=True)
        gain, spread = res["member"][0] - res["tiled"][0], max(res["tiled"][1], res["member"][1])
        print("  (a) same bits: %s; member - tiled = %.3f ms against a spread of %.3f ms: the tiled kernel is %s" % (
            same, gain, spread, "faster by more than the spread" if gain > spread else "NOT faster by more than the spread"),
            flush=True)

        # ---- (b) the whole call against the bare assignment pass, alternating, host clock ----
        eng = Engine(n, d, K, metric, device=0)
        easg = torch.empty((n,), dtype=torch.int32, device=dev)
        eprev = torch.empty((n,), dtype=torch.int32, device=dev)

        def bare():
            easg.fill_(K)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.lloyd_assign(x, cen, easg, eprev)
            eng.sync()
            return time.perf_counter() - t0

        def call(with_distances):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kmeans_predict(x, cen, metric=metric, return_distances=with_distances)
            return time.perf_counter() - t0
        kinds = (("bare lloyd_assign pass", bare), ("kmeans_predict", lambda: call(False)),
                 ("kmeans_predict + distances", lambda: call(True)))
        for _ in range(args.warmup):
            for _name, fn in kinds:
                fn()
        times = {name: [] for name, _ in kinds}
        for _ in range(reps):
            for name, fn in kinds:
                times[name].append(fn() * 1e3)
        assert bool((easg == asg).all()), "the bare pass and kmeans_predict disagree"
        base = statistics.median(times["bare lloyd_assign pass"])
        for name, _ in kinds:
            med, lo, hi = stats(times[name])
            print("  (b) %-27s median %.3f ms (min %.3f, max %.3f, spread %.3f); %+.3f ms beyond the bare pass" % (
                name, med, lo, hi, hi - lo, med - base), flush=True)
        eng.close()
        del eng, easg, eprev, dist, asg


if __name__ == "__main__":
    main()
