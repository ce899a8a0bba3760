#!/usr/bin/env python
"""Mini-batch K-means (kmamd_minibatch_*) on one GPU, `--features`-feature fp32 rows (uniform in [0,1))
against `--clusters` centroids drawn from the rows.  GPU only: it fails without a device.

(a) per batch size of `--batches`, device-resident rows, three things IN ALTERNATION, host clock around calls that wait
    for the device, `--measurements` measurements of each, every one the median of `--repeat` calls:
      step       MiniBatchKMeans.partial_fit of the batch
      predict    a kmeans_predict call on the same rows against the same centroids (a stateless call: it builds its
                 engine and buffers every time, which the resident model does not)
      bare pass  one Engine.lloyd_assign pass of a kept engine on the same rows: the assignment floor
      composed   the update composed from the Lloyd kernels on the same batch: Engine.move_deltas with prev = K
                 everywhere (every row "moves in"), then Engine.apply_delta
    The update part of the step is the step minus the floor (both floors are printed); it is "no slower" than the
    composed update if it does not exceed it by more than the larger spread (max - min) of the measurements.
(b) MiniBatchKMeans.fit of `--fit-steps` steps x `--fit-batch` rows on a `--fit-rows`-row corpus, once resident on
    the device and once in host memory (`--fit-rows 0` skips it).
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--batches", default="65536,1048576")
    ap.add_argument("--measurements", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fit-rows", type=int, default=8 << 20)
    ap.add_argument("--fit-steps", type=int, default=100)
    ap.add_argument("--fit-batch", type=int, default=65536)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("minibatch_bench.py needs a GPU")
    from kmcuda_amd import MiniBatchKMeans, kmeans_predict
    from kmcuda_amd.engine import Engine
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(4321)
    d, K = args.features, args.clusters

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    # ---- (a) one step, the assignment floor, the composed update ----
    for n in [int(b) for b in args.batches.split(",") if b]:
        x = torch.rand((n, d), dtype=torch.float32, device=dev, generator=gen)
        seeds = x[torch.randperm(n, device=dev, generator=gen)[:K]].contiguous()
        model = MiniBatchKMeans(seeds)
        model.partial_fit(x)   # (cluster weights > 0 from here on)
        cen = model.centroids
        asg = kmeans_predict(x, cen)
        eng = Engine(n, d, K, "L2", device=0)
        none = torch.full((n,), K, dtype=torch.int32, device=dev)
        delta = torch.zeros((K * d,), dtype=torch.float64, device=dev)
        dcount = torch.zeros((K,), dtype=torch.int32, device=dev)
        ccounts = torch.zeros((K,), dtype=torch.int32, device=dev)
        cwork = cen.clone()

        def composed():
            eng.move_deltas(x, none, asg, delta, dcount)
            eng.apply_delta(delta, dcount, cwork, ccounts)
            eng.sync()
        easg = torch.empty((n,), dtype=torch.int32, device=dev)
        eprev = torch.empty((n,), dtype=torch.int32, device=dev)

        def bare():
            easg.fill_(K)
            eng.lloyd_assign(x, cen, easg, eprev)
            eng.sync()
        kinds = (("step", lambda: model.partial_fit(x)), ("predict", lambda: kmeans_predict(x, cen)),
                 ("bare pass", bare), ("composed", composed))
        for _ in range(args.warmup):
            for _name, fn in kinds:
                fn()
        meas = {name: [] for name, _ in kinds}
        for _ in range(args.measurements):
            calls = {name: [] for name, _ in kinds}
            for _ in range(args.repeat):
                for name, fn in kinds:
                    calls[name].append(clock(fn))
            for name in calls:
                meas[name].append(statistics.median(calls[name]))
        print("%d x %d fp32 rows on the device, %d centroids: %d measurements, each the median of %d calls" % (
            n, d, K, args.measurements, args.repeat), flush=True)
        for name, _ in kinds:
            ts = meas[name]
            print("  %-9s median %.3f ms (min %.3f, max %.3f, spread %.3f)  %s" % (
                name, statistics.median(ts), min(ts), max(ts), max(ts) - min(ts),
                " ".join("%.3f" % t for t in ts)), flush=True)
        for floor in ("predict", "bare pass"):
            upd = [s - p for s, p in zip(meas["step"], meas[floor])]
            spread = max(max(upd) - min(upd), max(meas["composed"]) - min(meas["composed"]))
            over = statistics.median(upd) - statistics.median(meas["composed"])
            print("  step - %s: median %.3f ms (min %.3f, max %.3f); minus composed = %+.3f ms against a spread of "
                  "%.3f ms: the step's update is %s" % (floor, statistics.median(upd), min(upd), max(upd), over, spread,
                                                        "no slower" if over <= spread else "SLOWER"), flush=True)
        model.close()
        eng.close()
        del x, model, eng, none, delta, asg

    # ---- (b) fit on a device corpus and on a host corpus ----
    if args.fit_rows:
        n = args.fit_rows
        x = torch.rand((n, d), dtype=torch.float32, device=dev, generator=gen)
        seeds = x[torch.randperm(n, device=dev, generator=gen)[:K]].contiguous()
        for where, corpus, start in (("device", x, seeds), ("host", None, None)):
            if where == "host":
                corpus, start = x.cpu().numpy(), seeds.cpu().numpy()
                del x
                torch.cuda.empty_cache()
            with MiniBatchKMeans(start) as model:
                model.fit(corpus, 2, args.fit_batch, seed=1)   # warm-up: buffers, engine, code objects
                ms = clock(lambda: model.fit(corpus, args.fit_steps, args.fit_batch, seed=1))
                print("fit of %d steps x %d rows on a %d x %d %s corpus: %.1f ms, %.3f ms per step" % (
                    args.fit_steps, args.fit_batch, n, d, where, ms, ms / args.fit_steps), flush=True)


if __name__ == "__main__":
    main()
