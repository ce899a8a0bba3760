#!/usr/bin/env python3
"""pq_search on device-resident operands against a torch formulation of the same ADC on the same
device -- tables by broadcasting, one index gather per sub-space summed into a (queries, rows) matrix, topk -- chunked
over the queries to fit memory, and against the two floors of the scan.

    python scripts/pq_search_bench.py                  # N=1M, ksub=256, M x dsub = 32x8 and 8x32, Q=10000, k=10, 100
    python scripts/pq_search_bench.py --shapes 100000:8:4:256:1000:10 --repeat 3
    python scripts/pq_search_bench.py --bits 4 --shapes 1000000:32:8:16:10000:10,1000000:64:4:16:10000:10

Every figure is the median [min, max] of --repeat runs behind a warm-up, by a host clock around calls that end in a
device synchronise.  The torch side runs the first --baseline-queries queries only (its time is per query all the same)
and is the check as well: on those queries the distances agree to rounding (torch sums in another order) and the
indices agree wherever the distances are not within rounding of a tie.  Floors: Q N M table lookups of 4 bytes against
the LDS rate (256 CUs x 128 B/clk x 2.4 GHz), and N M ceil(Q / QT) code bytes against 8 TB/s, the HBM rate -- a floor
only where they miss the caches, which the block order is there to avoid.  --bits 4: ksub <= 16, the
codes packed two to a byte, half the code bytes in that floor.  --table-dtype float16: the search
over tables of halves is the subject -- its lookups are 2 bytes in the LDS floor and it agrees with torch to fp16
rounding, 2^-11 per entry -- and the fp32-table search is timed beside it, lap by lap in turn (`fp32_tables_ms`,
`fp32_over_fp16`).  There is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LDS_BYTES_PER_S = 256 * 128 * 2.4e9
HBM_BYTES_PER_S = 8e12


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


def torch_adc(queries, books, codes_long, k, chunk):
    import torch
    m, ksub, dsub = books.shape
    idx, dist = [], []
    for q0 in range(0, queries.shape[0], chunk):
        x = queries[q0:q0 + chunk].view(-1, m, 1, dsub)
        tables = ((x - books[None]) ** 2).sum(-1)                       # (chunk, M, ksub)
        d = torch.zeros((x.shape[0], codes_long.shape[0]), device=queries.device)
        for s in range(m):
            d += tables[:, s, codes_long[:, s]]
        top = torch.topk(d, k, dim=1, largest=False)
        idx.append(top.indices)
        dist.append(top.values)
    return torch.cat(idx), torch.cat(dist)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000000:32:8:256:10000:10,1000000:32:8:256:10000:100,"
                                        "1000000:8:32:256:10000:10,1000000:8:32:256:10000:100",
                    help="N:M:dsub:ksub:Q:k[,...]")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--baseline-queries", type=int, default=512)
    ap.add_argument("--baseline-chunk", type=int, default=64)
    ap.add_argument("--bits", type=int, default=8, choices=(8, 4))
    ap.add_argument("--table-dtype", default="float32", choices=("float32", "float16"))
    args = ap.parse_args()
    half = args.table_dtype == "float16"
    if half and args.bits == 4:
        sys.exit("fp16 tables serve the byte codes only")
    rtol = 2.0 ** -10 if half else 1e-5
    import torch
    from kmcuda_amd import pq_pack4, pq_search
    from kmcuda_amd.pq import query_tile
    if not torch.cuda.is_available():
        sys.exit("pq_search_bench needs a GPU")
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    for shape in args.shapes.split(","):
        n, m, dsub, ksub, nq, k = (int(v) for v in shape.split(":"))
        gen = torch.Generator(device=dev).manual_seed(1)
        books = torch.randn((m, ksub, dsub), generator=gen, device=dev)
        codes = torch.randint(0, ksub, (n, m), generator=gen, device=dev, dtype=torch.uint8)
        queries = torch.randn((nq, m * dsub), generator=gen, device=dev)
        stored = pq_pack4(codes) if args.bits == 4 else codes
        fns = [lambda: pq_search(queries, books, stored, k, bits=args.bits, table_dtype=args.table_dtype)]
        if half:
            fns.append(lambda: pq_search(queries, books, stored, k))
        laps = _median_ms_in_turn(fns, args.repeat, sync)
        ours = laps[0]
        idx, dist = fns[0]()

        nb = min(nq, args.baseline_queries)
        codes_long = codes.long()
        base = _median_ms(lambda: torch_adc(queries[:nb], books, codes_long, k, args.baseline_chunk), args.repeat, sync)
        t_idx, t_dist = torch_adc(queries[:nb], books, codes_long, k, args.baseline_chunk)
        close = bool(torch.allclose(dist[:nb], t_dist, rtol=rtol, atol=0))
        # a differing index is acceptable only between rows whose distances are within rounding of each other
        differ = idx[:nb].long() != t_idx
        tied = bool(torch.allclose(dist[:nb][differ], t_dist[differ], rtol=rtol, atol=0))
        qt = query_tile(m, k, bits=args.bits, table_dtype=args.table_dtype)
        print(json.dumps({
            "shape": {"N": n, "M": m, "dsub": dsub, "ksub": ksub, "Q": nq, "k": k, "bits": args.bits,
                      "table_dtype": args.table_dtype, "query_tile": qt},
            "pq_search_ms": ours, "pq_search_us_per_query": ours[0] * 1e3 / nq,
            "torch_ms": base, "torch_queries": nb, "torch_us_per_query": base[0] * 1e3 / nb,
            **({"fp32_tables_ms": laps[1], "fp32_over_fp16": laps[1][0] / ours[0]} if half else {}),
            "lds_floor_ms": nq * n * m * (2 if half else 4) / LDS_BYTES_PER_S * 1e3,
            "code_bytes_floor_ms": n * int(stored.shape[1]) * -(-nq // qt) / HBM_BYTES_PER_S * 1e3,
            "distances_agree": close, "indices_differ": int(differ.sum()), "differing_indices_are_ties": tied,
            "note": "[median, min, max] of %d runs" % args.repeat}), flush=True)
        assert close and tied, "pq_search and the torch formulation disagree"


if __name__ == "__main__":
    main()
