#!/usr/bin/env python
"""A weighted Lloyd iteration against the unweighted iteration of the same build (8M x 256 fp32, K = 1024, L2, random
positive weights), on one GPU.  Not bench.py: that stays the yardstick of the unweighted step.

    python scripts/weighted_bench.py [--samples N] [--features D] [--clusters K] [--steps S] [--warmup W] [--rounds R]

Both legs run the step loop bench.py times (lloyd_assign, reduce_fill, reduce_apply_prepare with the stop test on the
device), on the same rows and the same seeds, alternating R rounds so that clock drift hits both; the figure per leg
is the median round.  Prints one JSON line.  The update kernels on their own (cluster_sums, move_scatter):

    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/weighted_bench.py --rounds 1 --leg weighted
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/weighted_bench.py --rounds 1 --leg plain
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from kmcuda_amd.distributed import HipBackend, ShardedLloyd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=8 * 1024 * 1024)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg", choices=["both", "plain", "weighted"], default="both")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, D, K = args.samples, args.features, args.clusters
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    samples = torch.empty((N, D), dtype=torch.float32, device=dev)
    for s in range(0, N, 1 << 20):
        samples[s:min(N, s + (1 << 20))].uniform_(0.0, 1.0, generator=gen)
    perm = torch.randperm(N, generator=gen, device=dev)[:K]
    seeds = samples[perm].clone()
    # log-uniform over three decades: 10 ** U(-1.5, 1.5)
    weights = torch.pow(10.0, torch.empty(N, dtype=torch.float32, device=dev).uniform_(-1.5, 1.5, generator=gen))
    total = float(weights.double().sum().item())

    def leg(weighted):
        backend = HipBackend(samples, K, "L2", device_index=0, weights=weights if weighted else None)
        loop = ShardedLloyd(backend, total if weighted else N)
        loop.set_centroids(seeds.clone())
        for _ in range(args.warmup):
            loop.step(0.0)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loop.step(0.0)
        torch.cuda.synchronize(dev)
        ms = (time.perf_counter() - t0) / args.steps * 1e3
        loop.drain()
        if loop.stopped:
            raise SystemExit("the stop rule fired inside the timed region")
        backend.engine.close()
        return ms

    legs = {"both": (False, True), "plain": (False,), "weighted": (True,)}[args.leg]
    ms = {False: [], True: []}
    for _ in range(args.rounds):
        for weighted in legs:
            ms[weighted].append(leg(weighted))
    out = {"metric": "weighted_lloyd_iteration_ms", "samples": N, "features": D, "clusters": K, "steps": args.steps,
           "warmup": args.warmup, "rounds": args.rounds}
    if ms[False]:
        out["plain_ms"] = statistics.median(ms[False])
        out["plain_rounds_ms"] = ms[False]
    if ms[True]:
        out["weighted_ms"] = statistics.median(ms[True])
        out["weighted_rounds_ms"] = ms[True]
    if ms[False] and ms[True]:
        out["weighted_over_plain"] = out["weighted_ms"] / out["plain_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
