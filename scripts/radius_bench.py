#!/usr/bin/env python
"""Radius search on the k-NN index (kmcuda_amd.KnnIndex.query_radius) on one GPU: a `--samples` x
`--features` L2 corpus (Gaussian mixture of `--clusters` unit Gaussians, centres uniform in [0,10)^D, clustered by
kmeans_cuda), `--queries` FRESH draws from the same mixture, at the radius whose median hit count is `--hits`
(the median distance to the `--hits`-th neighbour, from index.query).

Prints the times of the count pass, the fill pass with and without distances, and of index.query(k = --hits) on the
same index and build; the ratio (count + fill with distances) / query; and, from one more count and fill under
KMCUDA_AMD_KNN_STATS, the radius searches' counters.  Every time is a host clock around a synchronous call on device tensors
(the calls wait for the device before they return); the first call of each kind is warm-up and is reported apart.

`--allow-fraction f` (several allowed) adds the MASKED radius search (kmamd_knn_index_radius_count_allow / _fill_allow,
DESIGN.md 4.18) beside the unmasked one: for every fraction a device-resident mask that allows about f of the rows --
`--mask-layout random`: every row with probability f; `runs`: the row ids in contiguous runs of 4096, a run allowed with
probability f (a mask that is not random: ids drawn together come from the same stretch of the corpus) --, its masked
count and fill (with distances, at the offsets of its own count), the mask preparation alone (radii_allow: the same
pack, member pass and reduction, plus a K-float copy), and the counters of one masked count.  `--unmasked-only` stops
after the count and fill timings (for a comparison of two builds)."""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--clusters", type=int, default=256)
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--hits", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3, help="timed calls of each kind after one warm-up call")
    ap.add_argument("--allow-fraction", type=float, action="append", default=[],
                    help="also time the masked search with about this fraction of the rows allowed (repeatable)")
    ap.add_argument("--mask-layout", choices=("random", "runs"), default="random",
                    help="runs: the allowed ids come in contiguous runs of 4096 ids")
    ap.add_argument("--unmasked-only", action="store_true", help="count and fill only")
    args = ap.parse_args()
    import torch
    from kmcuda_amd import KnnIndex, kmeans_cuda
    from kmcuda_amd.api import _DEVICE_ALLOCS, _raise_for
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    n, d, K, Q, k = args.samples, args.features, args.clusters, args.queries, args.hits

    def draw(rows):
        out = torch.empty((rows, d), dtype=torch.float32, device=dev)
        for s in range(0, rows, 1 << 20):
            e = min(rows, s + (1 << 20))
            lab = torch.randint(0, K, (e - s,), device=dev, generator=gen)
            out[s:e].normal_(0.0, 1.0, generator=gen)
            out[s:e] += centres[lab]
        return out

    centres = torch.rand((K, d), device=dev, generator=gen) * 10.0
    x, q = draw(n), draw(Q)
    torch.cuda.synchronize()
    cptr, aptr = kmeans_cuda((x.data_ptr(), 0, (n, d)), K, init="random", seed=777, tolerance=0.01, yinyang_t=0,
                             device=1, verbosity=0)
    cen, asg = _DEVICE_ALLOCS[cptr], _DEVICE_ALLOCS[aptr]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ix = KnnIndex(x, cen, asg)
    torch.cuda.synchronize()
    print("corpus %d x %d in %d clusters, %d queries; KnnIndex build %.3f s" % (n, d, K, Q, time.perf_counter() - t0), flush=True)

    def timed(fn):
        """(warm-up time, timed runs)"""
        out = []
        for _ in range(args.repeat + 1):
            torch.cuda.synchronize()
            ta = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - ta)
        return out[0], out[1:]

    nb, dist = ix.query(q, k)
    r = float(dist[:, k - 1].median())
    vp = ctypes.c_void_p
    counts = torch.zeros((Q,), dtype=torch.int32, device=dev)
    qa = torch.empty((Q,), dtype=torch.int32, device=dev)

    def count():
        _raise_for(ix.lib.kmamd_knn_index_radius_count(ix.h, r, Q, vp(q.data_ptr()), None, vp(counts.data_ptr()),
                                                       vp(qa.data_ptr()), 0), "count")
    count()
    offsets = torch.zeros((Q + 1,), dtype=torch.int64, device=dev)
    torch.cumsum(counts.to(torch.int64), 0, out=offsets[1:])
    total = int(offsets[-1])
    out_nb = torch.empty((total,), dtype=torch.int32, device=dev)
    out_d = torch.empty((total,), dtype=torch.float32, device=dev)

    def fill(with_distances):
        # (the clusters the count computed, as query_radius hands them over)
        _raise_for(ix.lib.kmamd_knn_index_radius_fill(ix.h, r, Q, vp(q.data_ptr()), vp(qa.data_ptr()), vp(offsets.data_ptr()),
                                                      vp(out_nb.data_ptr()), vp(out_d.data_ptr()) if with_distances else None, 0),
                   "fill")
    c = counts.to(torch.int64)
    print("radius %.6g: hits per query min %d / median %d / mean %.1f / max %d, %d in all, %d queries without a hit" %
          (r, int(c.min()), int(c.median()), float(c.double().mean()), int(c.max()), total, int((c == 0).sum())), flush=True)
    results = {}
    arms = (("count", count), ("fill with distances", lambda: fill(True)),
            ("fill without distances", lambda: fill(False)), ("query(k=%d)" % k, lambda: ix.query(q, k)),
            ("query_radius (count + fill, Python)", lambda: ix.query_radius(q, r)))
    for name, fn in arms[:2] if args.unmasked_only else arms:
        warm, runs = timed(fn)
        results[name] = min(runs)
        print("%-40s warm-up %.4f s; %s s" % (name, warm, " / ".join("%.4f" % t for t in runs)), flush=True)
    both = results["count"] + results["fill with distances"]
    if args.unmasked_only:
        print("count + fill with distances = %.4f s (best of %d each)" % (both, args.repeat), flush=True)
        ix.close()
        return
    print("count + fill with distances = %.4f s; query(k=%d) = %.4f s; ratio %.2f (best of %d each)" %
          (both, k, results["query(k=%d)" % k], both / results["query(k=%d)" % k], args.repeat), flush=True)
    # the counters of one pass of each (printed by the library)
    os.environ["KMCUDA_AMD_KNN_STATS"] = "1"
    count()
    fill(True)
    del os.environ["KMCUDA_AMD_KNN_STATS"]
    print("all pairs: %d" % (n * Q), flush=True)
    # ---- the masked search ----
    for f in args.allow_fraction:
        if args.mask_layout == "random":
            mask = torch.rand((n,), device=dev, generator=gen) < f
        else:
            runs_ok = torch.rand(((n + 4095) // 4096,), device=dev, generator=gen) < f
            mask = runs_ok.repeat_interleave(4096)[:n].contiguous()
        m8 = mask.view(torch.uint8)
        mcounts = torch.zeros((Q,), dtype=torch.int32, device=dev)

        def mcount():
            _raise_for(ix.lib.kmamd_knn_index_radius_count_allow(ix.h, r, Q, vp(q.data_ptr()), vp(qa.data_ptr()),
                                                                 vp(mcounts.data_ptr()), None, 0, vp(m8.data_ptr())), "count")
        mcount()
        moffsets = torch.zeros((Q + 1,), dtype=torch.int64, device=dev)
        torch.cumsum(mcounts.to(torch.int64), 0, out=moffsets[1:])
        mtotal = int(moffsets[-1])
        mnb = torch.empty((max(mtotal, 1),), dtype=torch.int32, device=dev)
        md = torch.empty((max(mtotal, 1),), dtype=torch.float32, device=dev)

        def mfill():
            _raise_for(ix.lib.kmamd_knn_index_radius_fill_allow(ix.h, r, Q, vp(q.data_ptr()), vp(qa.data_ptr()),
                                                                vp(moffsets.data_ptr()), vp(mnb.data_ptr()),
                                                                vp(md.data_ptr()), 0, vp(m8.data_ptr())), "fill")
        print("mask %s, fraction %g: %d of %d rows allowed, %d hits in all (unmasked %d)" %
              (args.mask_layout, f, int(mask.sum()), n, mtotal, total), flush=True)
        mres = {}
        for name, fn in (("masked count", mcount), ("masked fill with distances", mfill),
                         ("mask preparation alone (radii_allow)", lambda: ix.radii_allow(mask))):
            warm, runs = timed(fn)
            mres[name] = min(runs)
            print("%-40s warm-up %.4f s; %s s" % (name, warm, " / ".join("%.4f" % t for t in runs)), flush=True)
        print("fraction %g: masked count %.4f s (unmasked %.4f, x%.2f), masked fill %.4f s (unmasked %.4f, x%.2f), two "
              "mask preparations %.4f s" % (f, mres["masked count"], results["count"], mres["masked count"] / results["count"],
                                            mres["masked fill with distances"], results["fill with distances"],
                                            mres["masked fill with distances"] / results["fill with distances"],
                                            2 * mres["mask preparation alone (radii_allow)"]), flush=True)
        os.environ["KMCUDA_AMD_KNN_STATS"] = "1"
        mcount()
        del os.environ["KMCUDA_AMD_KNN_STATS"]
    ix.close()


if __name__ == "__main__":
    main()
