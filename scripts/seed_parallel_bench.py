#!/usr/bin/env python
"""k-means|| seeding against k-means++ seeding of the same build, on one GPU: `--samples` x `--features`
device-resident fp32 rows (uniform in [0,1), unit length under the angular metric), `--clusters` clusters. Not bench.py;
that stays the yardstick of the Lloyd step.  GPU only.

    python scripts/seed_parallel_bench.py [--samples N] [--features D] [--clusters K] [--metrics L2,angular]
                                          [--repeat R] [--tolerance T] [--rounds 5] [--oversampling 2K]

Per metric and per init ("k-means++", "k-means||"):
  seeding      kmeans_cuda(init, tolerance=1, yinyang_t=0): upload-free set-up + seeding + ONE assignment pass, and the
               library's own split of it (kmamd_last_run_stats: the seconds before the loop); its average_distance is
               the average distance right after seeding.  k-means||: the stand-alone kmeans_seed_parallel call as well.
  whole call   kmeans_cuda(init, tolerance=T, yinyang_t=0.1): wall clock, iterations, average_distance at convergence.
and for k-means|| the per-round breakdown (KMCUDA_AMD_TIMING=1 laps of one more stand-alone call, each lap waiting for
the device): assignment, distance, the sampling kernels (term update, draw), the weighting pass, the recluster.
Medians of `--repeat` calls after one warm-up call; prints one JSON line per metric.
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _capture_stderr(fn):
    """fn() with the process's stderr (the library's laps included) going to a file; returns its text."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode(errors="replace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=8 << 20)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--metrics", default="L2,angular")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--tolerance", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--oversampling", type=float, default=None)
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("seed_parallel_bench.py needs a GPU")
    from kmcuda_amd import _lib, api, kmeans_seed_parallel
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(4321)
    n, d, K = args.samples, args.features, args.clusters
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    for s in range(0, n, 1 << 20):
        x[s:min(n, s + (1 << 20))].uniform_(0.0, 1.0, generator=gen)
    par = ("k-means||", args.rounds) + ((args.oversampling,) if args.oversampling else ())

    def last_run():
        it, loop, setup = ctypes.c_uint32(0), ctypes.c_double(0), ctypes.c_double(0)
        L.kmamd_last_run_stats(ctypes.byref(it), ctypes.byref(loop), ctypes.byref(setup), None, None)
        return it.value, loop.value, setup.value

    def call(init, tolerance, yy, metric):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cp, ap_, avg = api.kmeans_cuda((x.data_ptr(), 0, (n, d)), K, tolerance=tolerance, init=init, yinyang_t=yy,
                                       metric=metric, average_distance=True, seed=args.seed, device=1)
        wall = time.perf_counter() - t0
        api.free_device_ptr(cp)
        api.free_device_ptr(ap_)
        it, loop, setup = last_run()
        return dict(wall_s=wall, iterations=it, loop_s=loop, before_loop_s=setup, average_distance=avg)

    def median_of(runs, key):
        return statistics.median(r[key] for r in runs)

    for metric in args.metrics.split(","):
        if metric == "angular":
            x /= x.norm(dim=1, keepdim=True)
        out = {"metric": metric, "samples": n, "features": d, "clusters": K, "rounds": args.rounds,
               "oversampling": args.oversampling or 2.0 * K, "tolerance": args.tolerance, "repeat": args.repeat}
        for name, init in (("k-means++", "k-means++"), ("k-means||", par)):
            call(init, 1.0, 0.0, metric)   # warm-up: code objects, streams
            seeded = [call(init, 1.0, 0.0, metric) for _ in range(args.repeat)]
            whole = [call(init, args.tolerance, 0.1, metric) for _ in range(args.repeat)]
            out[name] = {
                "seeding_call_s": median_of(seeded, "wall_s"),                 # seeding + one assignment pass
                "seeding_before_loop_s": median_of(seeded, "before_loop_s"),   # the library's own split
                "average_distance_after_seeding": seeded[0]["average_distance"],
                "whole_call_s": median_of(whole, "wall_s"),
                "whole_call_loop_s": median_of(whole, "loop_s"),
                "iterations": whole[0]["iterations"],
                "average_distance_at_convergence": whole[0]["average_distance"],
            }
        # ---- the stand-alone call, and its laps ----
        kw = dict(rounds=args.rounds, oversampling=args.oversampling, metric=metric, seed=args.seed)
        ts = []
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, info = kmeans_seed_parallel(x, K, return_candidates=True, **kw)
            ts.append(time.perf_counter() - t0)
        out["k-means||"]["standalone_s"] = statistics.median(ts)
        out["k-means||"]["candidates"] = int(len(info["rows"]))
        out["k-means||"]["live_candidates"] = int((info["counts"] > 0).sum())
        out["k-means||"]["round_ends"] = [int(v) for v in info["round_ends"]]
        out["k-means||"]["fell_back"] = info["fell_back"]
        os.environ["KMCUDA_AMD_TIMING"] = "1"
        try:
            text = _capture_stderr(lambda: kmeans_seed_parallel(x, K, **kw))
        finally:
            os.environ.pop("KMCUDA_AMD_TIMING", None)
        laps = {}
        for what, ms in re.findall(r"\[timing\] k-means\|\| round \d+ (.*?): ([0-9.]+) ms", text):
            laps[what] = laps.get(what, 0.0) + float(ms)
        out["k-means||"]["laps_ms"] = {k: round(v, 3) for k, v in laps.items()}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
