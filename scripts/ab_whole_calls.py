#!/usr/bin/env python
"""Host-code A/B of two builds of the library (DESIGN_LOG 27, 28, 32): one process per build, all alive at once, the
calls alternating between them, one warm-up and `--calls` measured calls of every workload each; every call's outputs
are compared between the builds by CRC-32.

   python scripts/ab_whole_calls.py --lib parent=/path/to/parent/libKMCUDA.so --lib this=kmcuda_amd/libKMCUDA.so
   (a build may be named twice under two labels: a second process of it is the control)

Workloads: (i) bench.py's timed region -- a fresh engine, 5 warm-up and 20 timed ShardedLloyd.step(0.0) on 8M x 256
uniform rows, K = 1024 --, ms per step; whole kmeans_cuda() calls on device-resident uniform rows, init="random",
yinyang_t = 0.1, tolerance 0.01, ms per call with the library's own clock around its iteration loop beside it:
(ii) 100 000 x 256, K = 1024; (iii) the same under KMCUDA_AMD_VIRTUAL_SHARDS=3 (the host's enqueue time shows);
(iv) 13 000 x 256, K = 64 (the fixed host cost of a call dominates)."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = ("i", "ii", "iii", "iv")


def worker():
    sys.path.insert(0, ROOT)
    import torch
    from kmcuda_amd import _lib, kmeans_cuda
    from kmcuda_amd.distributed import HipBackend, ShardedLloyd
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    big = torch.empty((8000000, 256), dtype=torch.float32, device=dev)
    for s in range(0, big.shape[0], 1 << 20):
        big[s:s + (1 << 20)].uniform_(0.0, 1.0, generator=gen)
    seeds = big[torch.randperm(big.shape[0], generator=gen, device=dev)[:1024]].clone()
    rows = {"ii": big[:100000], "iii": big[:100000], "iv": big[:13000]}
    clusters = {"ii": 1024, "iii": 1024, "iv": 64}

    def crc(*tensors):
        c = 0
        for t in tensors:
            c = zlib.crc32(t.cpu().numpy().tobytes(), c)
        return c

    def steps():
        backend = HipBackend(big, 1024, "L2", device_index=0)
        loop = ShardedLloyd(backend, big.shape[0])
        loop.set_centroids(seeds.clone())
        for _ in range(5):
            loop.step(0.0)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(20):
            loop.step(0.0)
        torch.cuda.synchronize(dev)
        ms = (time.perf_counter() - t0) * 1e3 / 20
        loop.drain()
        out = {"ms": ms, "crc": crc(backend.centroids, backend.assignments)}
        backend.engine.close()
        return out

    def call(which):
        x, k = rows[which], clusters[which]
        cen = torch.empty((k, x.shape[1]), dtype=torch.float32, device=dev)
        asg = torch.empty(x.shape[0], dtype=torch.int32, device=dev)
        if which == "iii":
            os.environ["KMCUDA_AMD_VIRTUAL_SHARDS"] = "3"
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        kmeans_cuda((x.data_ptr(), 0, tuple(x.shape), cen.data_ptr(), asg.data_ptr()), k, init="random", seed=777,
                    tolerance=0.01, yinyang_t=0.1, device=1, verbosity=0)
        ms = (time.perf_counter() - t0) * 1e3
        os.environ.pop("KMCUDA_AMD_VIRTUAL_SHARDS", None)
        iters, loop_s = ctypes.c_uint32(0), ctypes.c_double(0)
        _lib.lib().kmamd_last_run_stats(ctypes.byref(iters), ctypes.byref(loop_s), None, None, None)
        return {"ms": ms, "loop_ms": loop_s.value * 1e3, "iterations": iters.value, "crc": crc(cen, asg)}

    print(json.dumps({"ready": _lib.LIB_PATH}), flush=True)
    for line in sys.stdin:
        which = line.strip()
        if which == "quit":
            break
        print(json.dumps(steps() if which == "i" else call(which)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", required=True, help="label=path, two or three times")
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    args = ap.parse_args()
    builds = [spec.split("=", 1) for spec in args.lib]
    procs = []
    for label, path in builds:
        env = dict(os.environ, KMCUDA_AMD_LIB=os.path.abspath(path))
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], env=env, stdin=subprocess.PIPE,
                             stdout=subprocess.PIPE, text=True)
        procs.append(p)
    try:
        for (label, _), p in zip(builds, procs):
            print("%s: %s" % (label, json.loads(p.stdout.readline())["ready"]), flush=True)

        def ask(p, which):
            p.stdin.write(which + "\n")
            p.stdin.flush()
            line = p.stdout.readline()
            if not line:
                raise SystemExit("a worker ended (exit %s)" % p.wait())
            return json.loads(line)

        for which in args.workloads.split(","):
            got = {label: [] for label, _ in builds}
            for n in range(args.calls + 1):   # (call 0: the warm-up)
                crcs = set()
                for (label, _), p in zip(builds, procs):
                    r = ask(p, which)
                    crcs.add(r["crc"])
                    if n:
                        got[label].append(r)
                    print("(%s) call %d %s: %s" % (which, n, label, json.dumps(r)), flush=True)
                if len(crcs) != 1:
                    raise SystemExit("(%s) call %d: the builds' outputs differ" % (which, n))
            for key in ("ms", "loop_ms"):
                for label, _ in builds:
                    v = [r[key] for r in got[label] if key in r]
                    if v:
                        print("(%s) %-7s %-8s median %.3f (min %.3f - max %.3f)" % (which, key, label, statistics.median(v),
                                                                                 min(v), max(v)), flush=True)
    finally:
        for p in procs:
            try:
                p.stdin.write("quit\n")
                p.stdin.flush()
            except OSError:
                pass
        for p in procs:
            p.wait()


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker()
    else:
        main()
