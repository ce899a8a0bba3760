#!/usr/bin/env python3
"""IVF-PQ search on device-resident operands against pq_search on the same shape in the same session,
with recall against an exact torch brute force over the full rows, and the two floors of the probed scan.

    python scripts/ivfpq_bench.py                      # N=1M x 256, K=1024, M=32 x 8, Q=10000 and 100, k=10
    python scripts/ivfpq_bench.py --rows 100000 --clusters 128 --queries 1000 --repeat 3
    python scripts/ivfpq_bench.py --precomputed --queries 10000      # both table builds, lap by lap in turn
    python scripts/ivfpq_bench.py --bits 4 --subspaces 64 --refine 4 --queries 10000
    python scripts/ivfpq_bench.py --no-residual --table-dtype float16 --refine 4,16 --queries 10000

Data: a Gaussian mixture of `clusters` components (centres 2 * randn, unit noise); the mixture's centres serve as the
coarse centroids (no K-means is run: the subject is the search); queries are fresh draws of the mixture.  Codebooks are
trained on --train-rows rows: on residuals for the index, on the raw rows for pq_search.  Every time is the median
[min, max] of --repeat runs behind a warm-up, by a host clock around calls that end in a device synchronise.
`search_ms` is IvfPqIndex.search (kmeans_predict_top + the probed scan), `scan_ms` ivfpq_search with the probes given.
Floors: Q nprobe (N / K) M table lookups of 4 bytes against the LDS rate (256 CUs x 128 B/clk x 2.4 GHz), and the table
build's Q nprobe 256 D 3 lane operations against 256 CUs x 64 lanes x 2.4 GHz.  --precomputed adds the
precomputed-term variant to every line: `pre_search_ms` / `pre_scan_ms` are timed in turn with the
other two, lap by lap, `pre_recall` is against the same exact ground truth, and `pre_table_floor_ms` is the variant's
table build, Q nprobe M KB of query terms and as many of index terms read at 6.29 TB/s.  --bits 4:
16 codewords per sub-space, the codes of the index and of pq_search packed two to a byte; the table-build floor then
counts 16 codewords.  --refine F adds `refine_recall`, the recall of search(refine=F); with several factors, F1,F2, a
recall per factor.  --table-dtype float16
 adds the search over tables of halves to every line, timed in turn with the others, lap by lap:
`f16_ms` of pq_search, `f16_search_ms` / `f16_scan_ms`, `f16_recall` and `f16_refine_recall` against the same exact
ground truth, `scan_over_f16_scan`.  --no-residual adds a second index over the same rows and coarse
centroids with non-residual lists (codebooks from ivfpq_train(residual=False)), timed in turn with the others:
`nr_search_ms` / `nr_scan_ms`, `nr_recall`, `nr_refine_recall`, `scan_over_nr_scan`, with --table-dtype float16 also
`nr_f16_*` (against `f16_scan_ms`: `f16_scan_over_nr_f16_scan`), and `nr_table_copy_floor_ms`, the Q nprobe M KB of
table lines (half that in halves) a scan's blocks copy, against 6.29 TB/s.  There is no CPU path."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LDS_BYTES_PER_S = 256 * 128 * 2.4e9
LANE_OPS_PER_S = 256 * 64 * 2.4e9
COPY_BYTES_PER_S = 6.29e12


def _median_ms_in_turn(fns, repeat, sync):
    """(median, min, max) per function: a warm-up each, then `repeat` rounds of one lap each, in turn."""
    for fn in fns:
        fn()
    sync()
    laps = [[] for _ in fns]
    for _ in range(repeat):
        for fn, mine in zip(fns, laps):
            t0 = time.perf_counter()
            fn()
            sync()
            mine.append((time.perf_counter() - t0) * 1e3)
    return [(statistics.median(mine), min(mine), max(mine)) for mine in laps]


def _median_ms(fn, repeat, sync):
    return _median_ms_in_turn([fn], repeat, sync)[0]


def exact_topk(queries, rows, k, chunk=256):
    import torch
    norms = (rows * rows).sum(1)
    out = []
    for q0 in range(0, queries.shape[0], chunk):
        q = queries[q0:q0 + chunk]
        out.append(torch.topk(norms[None] - 2 * (q @ rows.T), k, dim=1, largest=False).indices)
    return torch.cat(out)


def recall(found, truth):
    hit = (found.long()[:, :, None] == truth[:, None, :]).any(2)
    return float(hit.float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--subspaces", type=int, default=32)
    ap.add_argument("--queries", default="10000,100")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nprobe", default="1,4,16,64")
    ap.add_argument("--train-rows", type=int, default=100000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--bits", type=int, default=8, choices=(8, 4))
    ap.add_argument("--refine", default="", help="also report the recall of search(refine=this); F or F1,F2,...")
    ap.add_argument("--no-residual", action="store_true", help="time an index of non-residual lists beside the search")
    ap.add_argument("--precomputed", action="store_true", help="time the precomputed-term variant beside the search")
    ap.add_argument("--table-dtype", default="float32", choices=("float32", "float16"),
                    help="float16: time the search over fp16 tables beside the fp32 one")
    args = ap.parse_args()
    half = args.table_dtype == "float16"
    refines = [int(v) for v in args.refine.split(",") if v]
    import torch
    from kmcuda_amd import (IvfPqIndex, ivfpq_search, ivfpq_terms, ivfpq_train, kmeans_batched,
                            kmeans_predict_batched, kmeans_predict_top, pq_pack4, pq_search)
    from kmcuda_amd.ivfpq import query_tile, row_split
    from kmcuda_amd.pq import query_tile as pre_query_tile
    if not torch.cuda.is_available():
        sys.exit("ivfpq_bench needs a GPU")
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    n, d, kc, m, k = args.rows, args.features, args.clusters, args.subspaces, args.k
    bits, ksub = args.bits, 16 if args.bits == 4 else 256
    if bits == 4 and args.precomputed:
        sys.exit("the precomputed-term variant has no 4-bit codes")
    if bits == 4 and half:
        sys.exit("fp16 tables serve the byte codes only")
    if bits == 4 and args.no_residual:
        sys.exit("non-residual lists hold byte codes only")
    gen = torch.Generator(device=dev).manual_seed(1)
    centres = 2 * torch.randn((kc, d), generator=gen, device=dev)

    def draw(count):
        labels = torch.randint(0, kc, (count,), generator=gen, device=dev)
        return centres[labels] + torch.randn((count, d), generator=gen, device=dev)
    rows = draw(n)
    train = rows[:args.train_rows].contiguous()
    t0 = time.perf_counter()
    books = ivfpq_train(train, centres, m, ksub=ksub, max_iter=10, seed=1)
    index = IvfPqIndex(rows, centres, books, bits=bits, keep_rows=bool(refines))
    sync()
    build_s = time.perf_counter() - t0
    if args.no_residual:
        t0 = time.perf_counter()
        nr_books = ivfpq_train(train, centres, m, ksub=ksub, max_iter=10, seed=1, residual=False)
        nr = IvfPqIndex(rows, centres, nr_books, keep_rows=bool(refines), residual=False)
        sync()
        nr_build_s = time.perf_counter() - t0
        nr16 = copy.copy(nr)
        nr16.table_dtype = "float16"
    if args.precomputed:
        t0 = time.perf_counter()
        terms = ivfpq_terms(centres, books)
        sync()
        terms_s = time.perf_counter() - t0
        pre = copy.copy(index)            # the same lists, searched from the terms
        pre.terms = terms
    if half:
        f16 = copy.copy(index)            # the same lists, scanned over tables of halves
        f16.table_dtype = "float16"
    raw_books, _, _ = kmeans_batched(train, ksub, init="random", layout="columns", problems=m, max_iter=10, seed=1)
    raw_codes = kmeans_predict_batched(rows, raw_books, layout="columns", dtype="uint8")
    if bits == 4:
        raw_codes = pq_pack4(raw_codes & 15)
    lens = (index.offsets[1:] - index.offsets[:-1]).long()
    print(json.dumps({"index": {"N": n, "D": d, "K": kc, "M": m, "dsub": d // m, "bits": bits,
                                "train_and_build_s": build_s,
                                "list_rows": [int(lens.min()), float(lens.float().mean()), int(lens.max())],
                                **({"nr_train_and_build_s": nr_build_s} if args.no_residual else {}),
                                **({"terms_s": terms_s, "terms_mb": terms.numel() * 4 / 2 ** 20}
                                   if args.precomputed else {})}}),
          flush=True)
    for nq in (int(v) for v in args.queries.split(",")):
        queries = draw(nq)
        truth = exact_topk(queries, rows, k)
        flat_fns = [lambda: pq_search(queries, raw_books, raw_codes, k, bits=bits)]
        if half:
            flat_fns.append(lambda: pq_search(queries, raw_books, raw_codes, k, table_dtype="float16"))
        flat_laps = _median_ms_in_turn(flat_fns, args.repeat, sync)
        flat = flat_laps[0]
        print(json.dumps({"pq_search": {"Q": nq, "k": k, "ms": flat, "us_per_query": flat[0] * 1e3 / nq,
                                        "recall": recall(flat_fns[0]()[0], truth),
                                        **({"f16_ms": flat_laps[1], "f16_recall": recall(flat_fns[1]()[0], truth),
                                            "ms_over_f16_ms": flat[0] / flat_laps[1][0]} if half else {})},
                          "note": "[median, min, max] of %d runs" % args.repeat}), flush=True)
        for nprobe in (int(v) for v in args.nprobe.split(",")):
            probes = kmeans_predict_top(queries, centres, nprobe, return_distances=False)
            fns = [lambda: index.search(queries, k, nprobe=nprobe),
                   lambda: ivfpq_search(queries, centres, books, index.codes, index.ids, index.offsets, probes, k,
                                        bits=bits)]
            if args.precomputed:
                fns += [lambda: pre.search(queries, k, nprobe=nprobe),
                        lambda: ivfpq_search(queries, centres, books, index.codes, index.ids, index.offsets, probes, k,
                                             terms=terms)]
            if half:
                fns += [lambda: f16.search(queries, k, nprobe=nprobe),
                        lambda: ivfpq_search(queries, centres, books, index.codes, index.ids, index.offsets, probes, k,
                                             table_dtype="float16")]
            if args.no_residual:      # behind everything else: laps[-2:] with fp32 tables, laps[-4:] with both
                for ix in (nr, nr16) if half else (nr,):
                    fns += [lambda ix=ix: ix.search(queries, k, nprobe=nprobe),
                            lambda ix=ix: ivfpq_search(queries, centres, ix.codebooks, ix.codes, ix.ids, ix.offsets,
                                                       probes, k, table_dtype=ix.table_dtype, residual=False)]
            laps = _median_ms_in_turn(fns, args.repeat, sync)
            whole, scan = laps[:2]

            def refined(ix):
                found = {f: recall(ix.search(queries, k, nprobe=nprobe, refine=f)[0], truth) for f in refines}
                return found[refines[0]] if len(refines) == 1 else found
            found = index.search(queries, k, nprobe=nprobe)[0]
            qt = query_tile(m, k, bits=bits)
            extra = {}
            if refines:
                extra["refine_recall"] = refined(index)
            if args.precomputed:
                pqt = pre_query_tile(m, k)
                extra = {**extra, "pre_search_ms": laps[2], "pre_scan_ms": laps[3],
                         "scan_over_pre_scan": scan[0] / laps[3][0],
                         "pre_recall": recall(pre.search(queries, k, nprobe=nprobe)[0], truth), "pre_pair_tile": pqt,
                         "pre_row_split": row_split(nq * nprobe, pqt, int(index.codes.shape[0])),
                         "pre_table_floor_ms": 2 * nq * nprobe * m * 1024 / COPY_BYTES_PER_S * 1e3}
            if half:
                hqt = query_tile(m, k, table_dtype="float16")
                f16_laps = laps[-6:-4] if args.no_residual else laps[-2:]
                extra = {**extra, "f16_search_ms": f16_laps[0], "f16_scan_ms": f16_laps[1],
                         "scan_over_f16_scan": scan[0] / f16_laps[1][0],
                         "f16_recall": recall(f16.search(queries, k, nprobe=nprobe)[0], truth), "f16_pair_tile": hqt,
                         "f16_row_split": row_split(nq * nprobe, hqt, int(index.codes.shape[0]))}
                if refines:
                    extra["f16_refine_recall"] = refined(f16)
            if args.no_residual:
                rows_l = int(nr.codes.shape[0])
                for ix, tag, mine, base in ((nr, "nr_", laps[-4:-2] if half else laps[-2:], scan),) + (
                        ((nr16, "nr_f16_", laps[-2:], extra["f16_scan_ms"]),) if half else ()):
                    tile = query_tile(m, k, table_dtype=ix.table_dtype, residual=False)
                    extra = {**extra, tag + "search_ms": mine[0], tag + "scan_ms": mine[1],
                             ("scan_over_" if ix is nr else "f16_scan_over_") + tag + "scan": base[0] / mine[1][0],
                             tag + "recall": recall(ix.search(queries, k, nprobe=nprobe)[0], truth),
                             tag + "pair_tile": tile, tag + "row_split": row_split(nq * nprobe, tile, rows_l),
                             tag + "table_copy_floor_ms": nq * nprobe * m * (512 if ix is nr16 else 1024)
                             / COPY_BYTES_PER_S * 1e3}
                    if refines:
                        extra[tag + "refine_recall"] = refined(ix)
            print(json.dumps({
                "ivfpq": {"Q": nq, "k": k, "nprobe": nprobe, "pair_tile": qt,
                          "row_split": row_split(nq * nprobe, qt, int(index.codes.shape[0]))},
                "search_ms": whole, "scan_ms": scan, "scan_us_per_query": scan[0] * 1e3 / nq,
                "recall": recall(found, truth), "pq_search_over_scan": flat[0] / scan[0],
                "lds_floor_ms": nq * nprobe * (n / kc) * m * 4 / LDS_BYTES_PER_S * 1e3,
                "table_build_floor_ms": nq * nprobe * ksub * d * 3 / LANE_OPS_PER_S * 1e3, **extra}), flush=True)


if __name__ == "__main__":
    main()
