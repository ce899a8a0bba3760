#!/usr/bin/env python3
"""Batched K-means on device-resident rows: time per pass of kmeans_batched and per
kmeans_predict_batched call, against the loop they replace -- per problem one contiguous copy of the column block and
one kmeans_predict -- and against the row bytes moved per second.

    python scripts/kmeans_batched_bench.py                  # B=32, N=1M, D=8, k=256 and B=8, D=32, "columns"
    python scripts/kmeans_batched_bench.py --shapes 4:100000:8:256 --repeat 3

A pass is timed as (run of 1 + P passes - run of 1 pass) / P with tolerance=0 on uniform rows, which do not settle in
P passes (the iterations are checked); every figure is the median of --repeat runs behind a warm-up of each shape,
by a host clock around calls that end in a device synchronise.  kmeans_cuda has no cap on its passes, so the training
loop it would replace is not timed here; the predict loop is the same kernels' comparison.  There is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _median_ms(fn, repeat, sync):
    fn()
    sync()
    laps = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        sync()
        laps.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(laps), min(laps), max(laps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32:1000000:8:256,8:1000000:32:256", help="B:N:D:k[,B:N:D:k...]")
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    import torch
    from kmcuda_amd import kmeans_batched, kmeans_predict, kmeans_predict_batched
    if not torch.cuda.is_available():
        sys.exit("kmeans_batched_bench needs a GPU")
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    for shape in args.shapes.split(","):
        b, n, d, k = (int(v) for v in shape.split(":"))
        gen = torch.Generator(device=dev).manual_seed(1)
        x = torch.rand((n, b * d), generator=gen, device=dev)            # "columns": the rows as a PQ corpus holds them
        init = x[:k].reshape(k, b, d).transpose(0, 1).contiguous()      # (B, k, D): the first k rows of every block
        row_bytes = n * b * d * 4
        P = args.passes
        its = kmeans_batched(x, k, init=init, max_iter=1 + P, layout="columns")[2]
        assert int(its.min()) == 1 + P, "a problem settled inside the timed passes"
        one = _median_ms(lambda: kmeans_batched(x, k, init=init, max_iter=1, layout="columns"), args.repeat, sync)
        many = _median_ms(lambda: kmeans_batched(x, k, init=init, max_iter=1 + P, layout="columns"), args.repeat, sync)
        pred = _median_ms(lambda: kmeans_predict_batched(x, init, layout="columns"), args.repeat, sync)
        codes = _median_ms(lambda: kmeans_predict_batched(x, init, layout="columns", dtype=numpy.uint8), args.repeat,
                           sync)

        def loop():
            return [kmeans_predict(x[:, p * d:(p + 1) * d].contiguous(), init[p]) for p in range(b)]
        same = all(bool((a.view(-1) == c).all()) for a, c in
                   zip(loop(), kmeans_predict_batched(x, init, layout="columns").t()))
        looped = _median_ms(loop, args.repeat, sync) if k >= 2 else None
        pass_ms = (many[0] - one[0]) / P
        print(json.dumps({
            "shape": {"B": b, "N": n, "D": d, "k": k, "layout": "columns"},
            "pass_ms": pass_ms, "pass_row_GBps": 2 * row_bytes / pass_ms / 1e6,   # a pass reads the rows twice
            "fit_1_pass_ms": one, "fit_%d_passes_ms" % (1 + P): many,
            "predict_ms": pred, "predict_row_GBps": row_bytes / pred[0] / 1e6, "predict_uint8_ms": codes,
            "predict_loop_ms": looped, "predict_loop_same_assignments": same,
            "note": "[median, min, max] of %d runs; GB/s = row bytes over the median" % args.repeat}))


if __name__ == "__main__":
    main()
