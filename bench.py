#!/usr/bin/env python
"""bench.py -- point-assignments/sec per Lloyd iteration, 8M x 256 fp32 L2 @ K=1024.

  python bench.py --gpus N --steps K --warmup W          (N > 1: starts its own N ranks, one per GPU, RCCL)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...   (same ranks, launched for it)
  python bench.py --gpus N --api                          (whole kmeans_cuda() calls through the C ABI, ONE process
                                                           driving the N GPUs of the device mask, ncclCommInitAll)

A "step" is one full Lloyd iteration over the (row-sharded) synthetic batch: centroid prep,
MFMA filter + exact refinement (bit-identical assignments), move-delta reduction, the fused
all-reduce (N > 1), the stop test (on the device, read by the host one step late) and the centroid update.  Inputs are resident in HBM before timing starts.
STRONG scaling: the 8M rows are split over the N ranks.  Rank 0 prints ONE JSON line.
A plain run sets up, warms up, times the steps and prints the line.  --full adds, after the timed region (never
inside it): rank 0 checks >= 1M rows of the state it has just timed against the CPU oracle ("verify"; --no-verify
skips it), the other filter's roofline on the same state, one whole kmeans_cuda() call and the CPU baselines.
--dump-outputs DIR writes what the last timed step computed (centroids, assignments) as DIR/<name>.npy.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PMC_TRAFFIC_SOURCE = None   # the profiles/ file `roofline.traffic` was read from (reported in the line)
DUMP_BYTES = 64 << 20       # --dump-outputs writes at most this much in all


def dump_outputs(path, arrays, total_bytes):
    """Writes every array as path/<name>.npy.  total_bytes: what all ranks' arrays hold together; past DUMP_BYTES each
    array keeps its share as a fixed, seeded sample of its rows, whose indices go to path/<name>_rows.npy."""
    import numpy
    os.makedirs(path, exist_ok=True)
    cap = DUMP_BYTES - (1 << 16)   # room for the .npy headers
    for name, a in arrays.items():
        if total_bytes > cap:
            m = int(cap * a.nbytes / total_bytes) // (a.nbytes // a.shape[0] + 8)
            if m < a.shape[0]:
                rows = numpy.sort(numpy.random.RandomState(0).choice(a.shape[0], m, replace=False))
                numpy.save(os.path.join(path, name + "_rows.npy"), rows.astype(numpy.float64))
                a = a[rows]
        numpy.save(os.path.join(path, name + ".npy"), a)


def pmc_traffic(rows_per_launch, filt="f32"):
    """HBM bytes per launch of the filter stage, from the committed rocprofv3 PMC passes
    (profiles/*_pmc_summary.json written by `scripts/gpu.sh <tag> pmc`: FETCH_SIZE doubled per the gfx950
    note in MI355X_MICROARCH.md, plus WRITE_SIZE), scaled by rows when the shard size differs.  For the
    two-stage default: its dominant (coarse) kernel.  PMC counters cannot be collected from inside the bench
    process; None if no matching profile is committed."""
    import glob
    global PMC_TRAFFIC_SOURCE
    want = {"f16": ("lloyd_coarse2_kernel",), "f32": ("lloyd_filter_kernel",)}[filt]
    # the NEWEST summary: by its own "collected" stamp (scripts/pmc_summary.py writes one since round 5), then by
    # name (r5a > r4zz > r3y: the rounds' files sort that way) -- never a file named here by hand (VERDICT r4 weak 4:
    # the name had gone stale by a round)
    def stamp(path):
        try:
            with open(path) as fin:
                return (json.load(fin).get("collected", ""), os.path.basename(path))
        except Exception:
            return ("", "")
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_summary.json")), key=stamp)
    if files:
        with open(files[-1]) as fin:
            pmc = json.load(fin)
        total = 0.0
        for w in want:
            hit = [v for k, v in pmc["kernels"].items() if k.startswith(w + "<") and "traffic_bytes_per_launch" in v]
            if not hit:
                return None
            total += hit[0]["traffic_bytes_per_launch"]
        PMC_TRAFFIC_SOURCE = "profiles/" + os.path.basename(files[-1])
        return total * (rows_per_launch / float(pmc["rows_per_launch"]))
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_lloyd_filter.json")))
    if not files or filt != "f32":
        return None
    with open(files[-1]) as fin:
        pmc = json.load(fin)
    PMC_TRAFFIC_SOURCE = "profiles/" + os.path.basename(files[-1])
    return pmc["traffic_bytes_per_launch"] * (rows_per_launch / float(pmc["rows_per_launch"]))


def cpu_baseline(features, clusters, budget_s=12.0):
    """The oracle (plain-C port of the reference's Lloyd assignment) on this box's host cores,
    on a bounded sample of the same workload."""
    import numpy
    import oracle
    rs = numpy.random.RandomState(0)
    cores = int(oracle.lib().kmo_num_threads())   # OpenMP threads the port actually runs on
    cen = rs.rand(clusters, features).astype(numpy.float32)
    probe = rs.rand(2048, features).astype(numpy.float32)
    t0 = time.time()
    oracle.lloyd_assign(probe, cen)
    dt = max(time.time() - t0, 1e-3)
    rows = int(min(max(2048 * budget_s / dt, 2048), 400000))
    x = rs.rand(rows, features).astype(numpy.float32)
    oracle.lloyd_assign(x[:4096], cen)  # warm the thread pool
    passes, t0 = 0, time.time()
    while passes == 0 or time.time() - t0 < budget_s:
        oracle.lloyd_assign(x, cen)
        passes += 1
    dt = time.time() - t0
    rows_done = rows * passes
    return {"value": rows_done / dt, "unit": "point-assignments/s", "cores": cores, "kind": "port",
            "sample": "%d passes over %d x %d rows of the same uniform data vs K=%d, kmeans_assign_lloyd of "
                      "oracle/kmcuda_oracle.c (OpenMP, %s), %.1f s" %
                      (passes, rows, features, clusters, "AVX-512 round-down FMA" if oracle.lib().kmo_have_avx512()
                       else "portable round-down FMA", dt)}


def sklearn_baseline(features, clusters, rows=100000, iters=6):
    """scikit-learn's Lloyd (the CPU contestant of the reference's README table, README.md:187-204)
    on this box's host cores: BASELINE config[0] shape, seconds per iteration -> assignments/s."""
    try:
        import numpy
        from sklearn.cluster import KMeans
        from threadpoolctl import threadpool_info
    except Exception as e:  # pragma: no cover
        return {"error": repr(e)}
    rs = numpy.random.RandomState(0)
    x = rs.rand(rows, features).astype(numpy.float32)
    init = x[rs.choice(rows, clusters, replace=False)].copy()
    t = {}
    for n in (1, 1, 1 + iters):   # the first fit warms the thread pool up and is discarded
        km = KMeans(n_clusters=clusters, init=init, n_init=1, max_iter=n, tol=0, algorithm="lloyd")
        t0 = time.time()
        km.fit(x)
        t[n] = time.time() - t0
    per_iter = max((t[1 + iters] - t[1]) / iters, 1e-6)
    threads = max([i.get("num_threads", 1) for i in threadpool_info()] or [1])
    return {"value": rows / per_iter, "unit": "point-assignments/s", "cores": threads, "kind": "sklearn",
            "sample": "sklearn.cluster.KMeans(algorithm='lloyd', n_init=1, tol=0) on %d x %d uniform rows, K=%d: "
                      "%.3f s per iteration (difference of a %d- and a 1-iteration fit)" %
                      (rows, features, clusters, per_iter, 1 + iters)}


def verify_state(backend, want_rows):
    """Outside the timed region: one more assignment pass on the state the bench has just timed (the
    centroids after the last update, the previous assignments), then >= want_rows of its rows -- whole
    128-row blocks spread over the shard plus a random sample -- are recomputed by the CPU oracle
    (oracle.lloyd_assign = the reference's kmeans_assign_lloyd arithmetic) and compared bit for bit;
    the device's reassignment counter is checked against a count of (new != previous) over all rows."""
    import numpy
    import torch
    import oracle
    n = backend.n_local
    prev = backend.assignments.clone()
    backend.reset_changed()
    backend.assign()
    backend.synchronize()
    changed_dev = backend.engine.counters()[0]
    changed_cnt = int((backend.assignments != prev).sum().item())
    want = min(int(want_rows), n)
    rs = numpy.random.RandomState(99)
    nblk = max(want // 2 // 128, 1)
    starts = numpy.unique((rs.randint(0, max(n // 128, 1), size=nblk) * 128).astype(numpy.int64))
    blocks = (starts[:, None] + numpy.arange(128)[None, :]).reshape(-1)
    blocks = blocks[blocks < n]
    rest = rs.choice(n, size=max(want - blocks.size, 0), replace=False) if n > want else numpy.arange(0)
    sel = numpy.unique(numpy.concatenate([blocks, rest.astype(numpy.int64)]))
    idx = torch.from_numpy(sel).to(backend.device)
    x = backend.samples.index_select(0, idx).cpu().numpy()
    cen = backend.centroids.cpu().numpy()
    got = backend.assignments.index_select(0, idx).cpu().numpy().view(numpy.uint32)
    prv = prev.index_select(0, idx).cpu().numpy().view(numpy.uint32)
    t0 = time.time()
    ref, _, ref_changed = oracle.lloyd_assign(x, cen, assignments=prv)
    dt = time.time() - t0
    mism = int((ref != got).sum())
    return {"rows_checked": int(sel.size), "assignment_mismatches": mism,
            "reassigned_in_sample_oracle": int(ref_changed), "reassigned_in_sample_device": int((got != prv).sum()),
            "changed_counter_device": int(changed_dev), "changed_recount_all_rows": changed_cnt,
            "ok": bool(mism == 0 and changed_dev == changed_cnt and int(ref_changed) == int((got != prv).sum())),
            "oracle_seconds": round(dt, 2),
            "what": "assignment pass after the timed steps vs oracle.lloyd_assign on whole 128-row blocks + a random "
                    "sample of this rank's rows (outside the timed region)"}


def api_bench(args):
    """Whole kmeans_cuda() calls through the drop-in C ABI: ONE process, device mask = the first
    --gpus GPUs (row shards + ncclCommInitAll inside the library), samples resident on GPU 0
    (device_ptrs = 0), init=random, Lloyd (yinyang_t = 0).  value = N x iterations / the library's own
    clock around its iteration loop (kmamd_last_run_stats); the call's wall time is reported beside it."""
    import ctypes
    if int(os.environ.get("RANK", "0")) != 0:
        return   # started under torch.distributed.run: ONE process drives every GPU here, the other ranks have nothing to do
    import torch
    from kmcuda_amd import _lib
    L = _lib.lib()
    N, D, K = args.samples, args.features, args.clusters
    ngpu = args.gpus
    if torch.cuda.device_count() < ngpu and not os.environ.get("KMCUDA_AMD_VIRTUAL_SHARDS"):
        raise SystemExit("--gpus %d but only %d GPU(s) visible" % (ngpu, torch.cuda.device_count()))
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    samples = torch.empty((N, D), dtype=torch.float32, device=dev)
    for s in range(0, N, 1 << 20):
        samples[s:min(N, s + (1 << 20))].uniform_(0.0, 1.0, generator=gen)
    cen = torch.empty((K, D), dtype=torch.float32, device=dev)
    asg = torch.empty(N, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    mask = (1 << ngpu) - 1 if not os.environ.get("KMCUDA_AMD_VIRTUAL_SHARDS") else 1
    os.environ["KMCUDA_AMD_TIME_COLLECTIVE"] = "1"   # events around every iteration's all-reduce inside the library
    runs = []
    calls = max(args.warmup > 0, 0) + max(args.steps // 10, 1)   # one warm-up call, then ~steps/10 timed calls
    for i in range(calls):
        t0 = time.perf_counter()
        rc = L.kmeans_cuda(0, None, args.tolerance, 0.0, 0, N, D, K, 777, mask, 0, 0, 0,
                           ctypes.c_void_p(samples.data_ptr()), ctypes.c_void_p(cen.data_ptr()),
                           ctypes.c_void_p(asg.data_ptr()), None)
        wall = time.perf_counter() - t0
        if rc != 0:
            raise SystemExit("kmeans_cuda failed: %s" % _lib.STATUS.get(rc, rc))
        it, shards, rccl = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        loop_s, setup_s = ctypes.c_double(), ctypes.c_double()
        L.kmamd_last_run_stats(ctypes.byref(it), ctypes.byref(loop_s), ctypes.byref(setup_s), ctypes.byref(shards),
                               ctypes.byref(rccl))
        cms, cn = ctypes.c_double(), ctypes.c_uint32()
        L.kmamd_last_run_collective(ctypes.byref(cms), ctypes.byref(cn))
        runs.append({"wall_s": wall, "loop_s": loop_s.value, "setup_s": setup_s.value, "iterations": it.value,
                     "shards": shards.value, "rccl_ranks": rccl.value, "collective_ms": cms.value,
                     "collectives": cn.value})
    if args.dump_outputs:   # what the last timed call returned
        dump_outputs(args.dump_outputs, {"centroids": cen.cpu().numpy(), "assignments": asg.cpu().numpy().astype("float32")},
                     K * D * 4 + N * 4)
    timed = runs[1:] if len(runs) > 1 else runs
    iters = sum(r["iterations"] for r in timed)
    loop = sum(r["loop_s"] for r in timed)
    out = {"metric": "point-assignments/sec per Lloyd iter (8Mx256@1024)", "value": N * iters / loop,
           "unit": "point-assignments/s", "n_gpus": ngpu, "steps": iters, "warmup": runs[0]["iterations"] if len(runs) > 1 else 0,
           "ms_per_step": loop / iters * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
           "dtype": "f32", "data": "synthetic",
           "config": {"workload": "whole kmeans_cuda() calls (C ABI, one process, device mask 0x%x): %dx%d fp32 L2 Lloyd, "
                                  "K=%d, uniform[0,1) rows on GPU 0 (device_ptrs=0), init=random seed 777, tolerance %g, "
                                  "yinyang_t=0" % (mask, N, D, K, args.tolerance),
                      "samples": N, "features": D, "clusters": K, "parallelism": "rows/%d" % timed[0]["shards"],
                      # (the same keys as the one-process-per-GPU line: a scaling run can take either loop)
                      # ranks of the communicator the library created (ncclCommInitAll over the mask); 1: none
                      "ranks_seen_by_communicator": max(1, timed[0]["rccl_ranks"]),
                      # the library's own events around every iteration's all-reduce on the first shard's stream (its
                      # one-device stand-in under KMCUDA_AMD_VIRTUAL_SHARDS); null: one shard
                      "collective_ms_per_step": (sum(r["collective_ms"] for r in timed) / sum(r["collectives"] for r in timed))
                      if sum(r["collectives"] for r in timed) else None,
                      "collective": ("ncclAllReduce inside the library (ncclCommInitAll over the device mask), one fused "
                                     "fp64 buffer per iteration" if timed[0]["rccl_ranks"] else
                                     ("none" if timed[0]["shards"] == 1 else "sum kernel on one device (KMCUDA_AMD_VIRTUAL_SHARDS)")),
                      "filter": "f16", "row_cache": True,
                      "rccl_ranks_in_library": timed[0]["rccl_ranks"]},
           "calls": runs,
           "note": "value = N x iterations / seconds the library spent in its iteration loop (after upload and "
                   "seeding); wall_s is the whole call incl. the peer copies of the row shards, the reference's shuffle "
                   "draws for init=random and the output gather"}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--samples", type=int, default=8000000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also run what the headline figure does not need: the oracle check of "
                         "the timed state, the other filter's roofline, a whole kmeans_cuda() call, the CPU baselines")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed (centroids; assignments as float32) as DIR/<name>.npy, "
                         "at most 64 MB in all (a fixed, seeded sample of the rows beyond that)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines")
    ap.add_argument("--no-row-cache", action="store_true",
                    help="convert the coarse stage's operands from the rows on every pass instead of streaming the "
                         "engine's centred half copy (kmamd_set_row_cache); assignments are identical")
    ap.add_argument("--filter", default="f16", choices=["f16", "f32"],
                    help="matrix-core scheme of the assignment filter: f16 = two-stage v_mfma_f32_32x32x16_f16 (coarse "
                         "hi.hi pass, then the contenders of the undecided rows in fp32; default), f32 = "
                         "v_mfma_f32_32x32x2_f32.  Assignments are bit-identical")
    ap.add_argument("--no-verify", action="store_true",
                    help="--full: skip the oracle check of the timed state (outside the timed region)")
    ap.add_argument("--verify-rows", type=int, default=1000000)
    ap.add_argument("--no-api-leg", action="store_true",
                    help="--full: skip the whole kmeans_cuda() call that is timed beside the step loop (outside the timed "
                         "region)")
    ap.add_argument("--api", action="store_true",
                    help="time whole kmeans_cuda() calls through the drop-in C ABI (device mask = the first --gpus "
                         "GPUs, ONE process, device-resident input) instead of the one-process-per-GPU step loop")
    ap.add_argument("--tolerance", type=float, default=0.01, help="--api: kmeans_cuda's stop tolerance")
    ap.add_argument("--step-tolerance", type=float, default=0.0,
                    help="tolerance of the stop test every timed step evaluates (0: stop only when no row moves)")
    ap.add_argument("--dtype", default="f32", choices=["f32", "f16"],
                    help="f32: the headline fp32 L2 path.  f16: the fp16x2 path (rows as halves, f16 matrix-core "
                         "filter; same assignments as the fp32 path on the same values)")
    args = ap.parse_args()

    import torch
    import torch.distributed as dist
    from kmcuda_amd.distributed import HipBackend, ShardedLloyd, row_block
    ranks_seen = 1
    if args.api:
        return api_bench(args)
    if args.gpus > 1 and "RANK" not in os.environ:
        # started as `python bench.py --gpus N`: become the launcher of N ranks of this same script, one per
        # GPU (RCCL over xGMI between them); the ranks print the line
        import socket
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        os.execv(sys.executable, cmd)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    # test hooks (a 1-GPU box cannot run RCCL across ranks): all ranks on GPU 0 over gloo
    if os.environ.get("KMCUDA_AMD_BENCH_SINGLE_DEVICE"):
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        backend_name = os.environ.get("KMCUDA_AMD_BENCH_BACKEND", "nccl")   # "nccl" IS RCCL on ROCm
        if backend_name == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend_name)
        ranks_seen = dist.get_world_size(dist.group.WORLD)   # (the group ShardedLloyd reduces over)
        if not os.environ.get("KMCUDA_AMD_BENCH_SINGLE_DEVICE") and torch.cuda.device_count() < world:
            raise SystemExit("--gpus %d but only %d GPU(s) visible" % (world, torch.cuda.device_count()))

    N, D, K = args.samples, args.features, args.clusters
    lo, hi = row_block(N, rank, world)
    n_local = hi - lo
    # synthetic uniform [0,1) rows (the reference's own benchmark data, README.md:206-207),
    # generated on device in chunks; per-rank seed so shards differ
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234 + rank)
    samples = torch.empty((n_local, D), dtype=torch.float32, device=dev)
    chunk = 1 << 20
    for s in range(0, n_local, chunk):
        e = min(n_local, s + chunk)
        samples[s:e].uniform_(0.0, 1.0, generator=gen)
    half = None
    if args.dtype == "f16":
        half = samples.to(torch.float16)
        samples = half.to(torch.float32)
    backend = HipBackend(samples, K, "L2", device_index=local_rank, half_rows=half, row_cache=not args.no_row_cache)
    backend.engine.set_filter(args.filter)
    loop = ShardedLloyd(backend, N)
    # init="random": K sample rows of rank 0 (replicated by broadcast)
    perm = torch.randperm(n_local, generator=gen, device=dev)[:K]
    loop.set_centroids(samples[perm].clone())

    def barrier():
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    # every step carries the reference's stop test (check_changed, kmeans.cu:697-717) the way kmeans_cuda() runs
    # it: decided on the device by the update kernel, read by the host one iteration late.  Tolerance 0: the rule
    # fires only when no row moves, which this workload does not reach in these iterations (checked below)
    for _ in range(args.warmup):
        loop.step(args.step_tolerance)
    backend.engine.profile(True)
    loop.time_collective = world > 1   # a pair of events around every timed step's all-reduce, on its stream
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loop.step(args.step_tolerance)
    barrier()
    elapsed = time.perf_counter() - t0
    loop.time_collective = False
    coll_ms, coll_n = loop.collective_ms()
    loop.drain()
    if loop.stopped:
        raise SystemExit("the stop rule fired inside the timed region (%d iterations): the remaining steps were "
                         "no-ops -- use fewer steps or a smaller --step-tolerance" % loop.iterations)
    prof = backend.engine.profile_read()
    # the last timed step's full-scan / pair rows: the update kernel copied the pass's counters behind the move sums
    # (buffer tail [K*D + K ..+3] = counters[0..3]) BEFORE the fused preparation zeroed the lists for the next pass
    # -- read from the engine after drain() they were 0 / 0.  All ranks' rows when N > 1.
    tail = loop.buf[K * D + K:K * D + K + 4].cpu().tolist()
    flagged = int(tail[1])
    pair_rows = int(tail[3])
    backend.engine.profile(False)
    if args.dump_outputs:   # what a caller of the loop receives after the last timed step, before anything else runs
        arrays = {"centroids": backend.centroids.cpu().numpy()} if rank == 0 else {}   # (replicated on every rank)
        name = "assignments" if world == 1 else "assignments_rank%d" % rank               # this rank's rows
        arrays[name] = backend.assignments.cpu().numpy().astype("float32")
        dump_outputs(args.dump_outputs, arrays, K * D * 4 + N * 4)
    # --full, outside the timed region, and BEFORE anything else touches the state: the pass that follows the last
    # timed update (it reassigns what a 21st step would: its change counter is checked on real moves)
    verify = None
    if args.full and rank == 0 and not args.no_verify:
        verify = verify_state(backend, args.verify_rows)
    # then the OTHER filter on the same state, for the side-by-side roofline entry
    other = "f32" if args.filter != "f32" else "f16"
    if args.full:
        backend.engine.set_filter(other)
        backend.assign()
        backend.engine.profile(True)
        for _ in range(2):
            backend.assign()
        torch.cuda.synchronize(dev)
        prof_other = backend.engine.profile_read()
        backend.engine.set_filter(args.filter)
        backend.engine.profile(False)
    changed_last = loop.changed_last()
    # The drop-in entry point on the same rows, outside the timed region (`value` times the
    # one-process-per-GPU step loop; what a caller of kmeans_cuda() gets had no driver-run record): one whole call
    # through the C ABI -- device-resident rows, init=random, tolerance 0.01, yinyang_t=0 -- timed by the library's own
    # clock around its iteration loop (kmamd_last_run_stats).
    api_leg = None
    if args.full and rank == 0 and world == 1 and not args.no_api_leg and args.dtype == "f32":
        try:
            import ctypes
            from kmcuda_amd import _lib
            L = _lib.lib()
            cen = torch.empty((K, D), dtype=torch.float32, device=dev)
            asg = torch.empty(n_local, dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            calls = []
            for _ in range(2):   # (the first call of a process loads code objects and creates its streams)
                t0 = time.perf_counter()
                rc = L.kmeans_cuda(0, None, 0.01, 0.0, 0, n_local, D, K, 777, 1 << local_rank, local_rank, 0, 0,
                                   ctypes.c_void_p(samples.data_ptr()), ctypes.c_void_p(cen.data_ptr()),
                                   ctypes.c_void_p(asg.data_ptr()), None)
                wall = time.perf_counter() - t0
                it, loop_s = ctypes.c_uint32(), ctypes.c_double()
                L.kmamd_last_run_stats(ctypes.byref(it), ctypes.byref(loop_s), None, None, None)
                calls.append((rc, it.value, loop_s.value, wall))
            rc, its, loop_s, wall = calls[-1]
            api_leg = {"rc": rc, "iterations": its, "loop_s": loop_s, "wall_s": wall,
                       "ms_per_iteration": loop_s / max(its, 1) * 1e3,
                       "value": n_local * its / loop_s if loop_s > 0 else 0.0, "unit": "point-assignments/s",
                       "what": "second of two whole kmeans_cuda() calls on the same rows (C ABI, device_ptrs = this GPU, "
                               "init=random seed 777, tolerance 0.01, yinyang_t=0), outside the timed region; iterations x "
                               "rows / the library's own clock around its iteration loop"}
            del cen, asg
        except Exception as e:  # pragma: no cover
            api_leg = {"error": repr(e)}

    t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())

    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        value = N / (elapsed / args.steps)
        launches = max(prof["filter_launches"], 1)
        filter_ms = prof["filter_ms"] / launches          # both stages of the two-stage filter
        coarse_ms = prof["coarse_ms"] / launches          # its dominant kernel alone (0 for the other filters)
        cached = args.filter == "f16" and not args.no_row_cache and os.environ.get("KMCUDA_AMD_ROW_CACHE", "1") != "0"
        dom_ms = coarse_ms if (args.filter == "f16" and coarse_ms > 0) else filter_ms
        flops = 2.0 * D * K * n_local                      # algorithmic flop of one filter launch
        achieved = flops / (filter_ms * 1e-3) / 1e12 if filter_ms > 0 else 0.0
        f16 = args.dtype == "f16"

        def roof(filt, ms):
            # ceilings of the ALGORITHMIC rate (2*D*K flop per row), MI355X_MICROARCH.md peaks:
            #   f32   one v_mfma_f32_32x32x2_f32 MAC per algorithmic MAC        -> 157.3 TFLOP/s
            #   f16   two-stage: the dominant (coarse) kernel does ONE half product per MAC -> 2500
            pk = {"f32": PEAK_FP32_MFMA_TFLOPS, "f16": 2500.0}[filt]
            ach = flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            return pk, ach
        peak, achieved = roof(args.filter, dom_ms)
        hr = "true" if f16 else "false"
        kname = {"f16": "lloyd_coarse2_kernel<256,%s,true,%s>" % (("false", "true") if cached else (hr, "false")),
                 "f32": "lloyd_filter_kernel<256,true>"}
        # HBM bytes the dominant kernel has to move: the row cache (2 D + 8 bytes per row) or the rows
        row_bytes = (2 * D + 8) if cached else (D * (2 if f16 else 4))
        alg_bytes = n_local * (row_bytes + 4)
        out = {
            "metric": "point-assignments/sec per Lloyd iter (8Mx256@1024)",
            "value": value, "unit": "point-assignments/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": "%dx%d %s L2 Lloyd iteration, K=%d, uniform[0,1) rows, init=random; "
                                   "rows sharded %d-way" % (N, D, "fp16x2" if f16 else "fp32", K, world),
                       "samples": N, "features": D, "clusters": K, "parallelism": "rows/%d" % world,
                       # the communicator the timed steps' all-reduce ran on, asked itself (not WORLD_SIZE)
                       "ranks_seen_by_communicator": ranks_seen,
                       "collective": ("one all-reduce of %d doubles per iteration (%s)" %
                                      (K * D + K + 4, os.environ.get("KMCUDA_AMD_BENCH_BACKEND", "nccl = RCCL")))
                       if world > 1 else "none",
                       # rank 0's events around the all-reduce on its stream: the exchange + the wait for the slowest
                       # rank's move sums (null: one rank, no collective)
                       "collective_ms_per_step": (coll_ms / coll_n) if coll_n else None,
                       "collectives_timed": coll_n,
                       "filter": args.filter, "row_cache": bool(cached)},
            "roofline": {"bound": "mfma", "achieved": achieved, "peak": peak,
                         "unit": "TFLOP/s", "frac": achieved / peak,
                         "traffic": pmc_traffic(n_local, args.filter) if not f16 else None,
                         "traffic_unit": "bytes/launch (rocprofv3 PMC, profiles/)", "traffic_source": PMC_TRAFFIC_SOURCE,
                         "algorithmic_bytes": alg_bytes, "algorithmic_flop": flops,
                         "hbm": {"achieved": alg_bytes / (dom_ms * 1e-3) / 1e9 if dom_ms > 0 else 0.0, "peak": 8000.0,
                                 "unit": "GB/s", "frac": alg_bytes / (dom_ms * 1e-3) / 1e9 / 8000.0 if dom_ms > 0 else 0.0},
                         "peak_note": "dense MFMA peak of the instruction the dominant kernel issues, per algorithmic "
                                      "MAC: f32 157.3; f16 (two-stage, coarse pass = one half product per MAC) 2500.  "
                                      "The chip runs the f16 kernels "
                                      "at ~1.7 GHz (power), where the same pipe peaks at ~1770; the coarse kernel's "
                                      "instruction mix with LDS-resident tiles and no HBM sustains 0.55 of 2500 on this "
                                      "chip, the MFMA alone on random halves 0.60-0.64 (scripts/coarse_probe.hip, "
                                      "scripts/mfma_probe.hip, profiles/r6b_*)",
                         "kernel": kname[args.filter],
                         "kernel_ms": dom_ms, "filter_stage_ms": filter_ms, "rows_per_launch": n_local},
            "breakdown_ms_per_step": {"filter": filter_ms, "filter_coarse_kernel": coarse_ms,
                                      "exact_refine": prof["exact_ms"] / launches,
                                      "update": prof["update_ms"] / launches},
            "assignment_step_only": {"ms": filter_ms + prof["exact_ms"] / launches,
                                     "value": n_local * world / ((filter_ms + prof["exact_ms"] / launches) * 1e-3)
                                     if filter_ms > 0 else 0.0,
                                     "note": "SURVEY 8(d) also names N / (time of the assignment step alone): both "
                                             "filter stages + pair / exact refine of rank 0's shard, by HIP events; "
                                             "`value` above divides by the FULL iteration (prep, assignment, update, "
                                             "all-reduce)"},
            "rows_full_exact_scan_last_step": flagged, "rows_pair_refined_last_step": pair_rows, "reassigned_last_step": changed_last,
        }
        if args.full:
            other_ms = prof_other["filter_ms"] / max(prof_other["filter_launches"], 1)
            opeak, oach = roof(other, other_ms)
            out["roofline_other_filter"] = {"filter": other, "kernel": kname[other], "kernel_ms": other_ms,
                                            "achieved": oach, "peak": opeak, "unit": "TFLOP/s", "frac": oach / opeak,
                                            "note": "same rows and centroids, timed outside the timed region"}
        if verify is not None:
            out["verify"] = verify
        if api_leg is not None:
            out["api_kmeans_cuda"] = api_leg
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(D, K)
            out["cpu_baseline_sklearn"] = sklearn_baseline(D, K)
        print(json.dumps(out))
    if world > 1:
        dist.barrier()   # rank 0 may still have been verifying / timing the CPU baseline: leave together
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
