"""ivfpq_search(residual=False) and IvfPqIndex(residual=False) against a plain numpy restatement, bit
for bit: pq_search's table of the query itself, the ascending sum over the probed lists, the order by (distance, id)."""
import numpy
import pytest

from kmcuda_amd import (IvfPqIndex, ivfpq_search, ivfpq_train, kmeans_batched, kmeans_predict_batched, knn_rerank,
                        pq_search)
from kmcuda_amd.ivfpq import query_tile, row_split

pytestmark = pytest.mark.gpu

K = 9
LENS = (0, 1, 255, 257, 700, 3, 40, 64, 300)     # an empty list, one row, around a 256-row step, three steps
L = sum(LENS)
OFFSETS = numpy.concatenate([[0], numpy.cumsum(LENS)]).astype(numpy.uint32)
DTYPES = ("float32", "float16")


def _definition(queries, books, codes, ids, probes, k, table_dtype):
    m_, ksub, dsub = books.shape
    idx = numpy.full((len(queries), k), 0xFFFFFFFF, numpy.uint32)
    dist = numpy.full((len(queries), k), numpy.nan, numpy.float32)
    with numpy.errstate(invalid="ignore", over="ignore"):
        t = queries.reshape(len(queries), m_, 1, dsub) - books
        t = t * t
        table = numpy.full((len(queries), m_, 256), numpy.inf, numpy.float32)
        table[..., :ksub] = t[..., 0]
        for j in range(1, dsub):
            table[..., :ksub] = table[..., :ksub] + t[..., j]
        if table_dtype == "float16":
            table = table.astype(numpy.float16).astype(numpy.float32)
    for q in range(len(queries)):
        keys = [numpy.zeros(0, numpy.uint64)]
        for p in dict.fromkeys(int(v) for v in probes[q] if v < K):
            lo, hi = int(OFFSETS[p]), int(OFFSETS[p + 1])
            rows = codes[lo:hi]
            d = table[q, 0, rows[:, 0]]
            for m in range(1, m_):
                d = d + table[q, m, rows[:, m]]
            bits = d.view(numpy.uint32).astype(numpy.uint64)
            bits[numpy.isnan(d)] = 0x7FC00000
            keys.append(bits << numpy.uint64(32) | ids[lo:hi])
        best = numpy.sort(numpy.concatenate(keys))[:k]
        idx[q, :len(best)] = best & numpy.uint64(0xFFFFFFFF)
        dist[q, :len(best)] = (best >> numpy.uint64(32)).astype(numpy.uint32).view(numpy.float32)
    return idx, dist


def _data(m, dsub, nq, ksub):
    rs = numpy.random.RandomState(0)
    books = rs.randn(m, ksub, dsub).astype(numpy.float32)
    codes = rs.randint(0, ksub, (L, m)).astype(numpy.uint8)
    if ksub < 256:
        codes[rs.rand(L) < 0.03, rs.randint(0, m)] = rs.randint(ksub, 256)       # bytes that name no codeword
    queries = rs.randn(nq, m * dsub).astype(numpy.float32)
    queries[1, ::dsub] = numpy.nan
    return queries, rs.randn(K, m * dsub).astype(numpy.float32), books, codes, rs.permutation(L).astype(numpy.uint32)


def _probes(nq, nprobe):
    """Fillers (K) and repeats; everybody's first probe is the 700-row list (more pairs than any tile), one query alone
    probes the one-row list (fewer than any tile), query 7 reaches three rows at most, query 6 has no valid probe."""
    probes = numpy.random.RandomState(1).randint(0, K + 1, (nq, nprobe)).astype(numpy.uint32)
    probes[probes == 1] = 3
    probes[:, 0] = 4
    probes[5, -1] = 1
    probes[7] = numpy.array([0, 5, 0, 5, K], numpy.uint32)[:nprobe]
    probes[6] = K + 3
    return probes


# (M, dsub, Q, nprobe, k, ksub): fp32 tiles of 16, 16, 8, 4 (k = 256), 4 and 2, fp16 tiles of 16, 16, 16, 8, 4 and 4;
# byte, dword and 16-byte code loads; Q no multiple of a tile; the last: 2050 pairs, so no row split at either tile
CASES = [(3, 3, 37, 5, 10, 200), (4, 4, 37, 5, 10, 256), (4, 4, 9, 1, 10, 200), (8, 2, 37, 5, 10, 200),
         (8, 2, 37, 5, 256, 256), (32, 4, 37, 5, 10, 200), (32, 4, 9, 1, 10, 256), (64, 2, 37, 5, 10, 256),
         (64, 2, 410, 5, 10, 200)]


@pytest.mark.parametrize("table_dtype", DTYPES)
@pytest.mark.parametrize("m,dsub,nq,nprobe,k,ksub,kind",
                         [c + ("numpy",) for c in CASES] + [c + ("torch",) for c in CASES if c[0] == 8])
def test_matches_the_definition(monkeypatch, m, dsub, nq, nprobe, k, ksub, kind, table_dtype):
    if (m, nq, k) == (32, 37, 10):
        monkeypatch.setenv("KMCUDA_AMD_IVFPQ_QUERY_CHUNK", "16")      # three query chunks
    tile = query_tile(m, k, table_dtype=table_dtype, residual=False)
    want = {3: 16, 4: 16, 8: 8 if k == 10 else 4, 32: 4, 64: 2}[m] if table_dtype == "float32" else \
        {3: 16, 4: 16, 8: 16 if k == 10 else 8, 32: 4, 64: 4}[m]
    assert tile == want and (row_split(nq * nprobe, tile, L) == 1) == (nq == 410)
    queries, centroids, books, codes, ids = _data(m, dsub, nq, ksub)
    probes = _probes(nq, nprobe)
    args = [queries, centroids, books, codes, ids, OFFSETS, probes]
    if kind == "torch":
        import torch
        args = [torch.from_numpy(a.view(numpy.int32) if a.dtype == numpy.uint32 else a).cuda() for a in args]
    idx, dist = ivfpq_search(*args, k, table_dtype=table_dtype, residual=False)
    if kind == "torch":
        idx, dist = idx.cpu().numpy().view(numpy.uint32), dist.cpu().numpy()
    w_idx, w_dist = _definition(queries, books, codes, ids, probes, k, table_dtype)
    assert idx.dtype == numpy.uint32 and dist.dtype == numpy.float32 and (idx == w_idx).all()
    nan = numpy.isnan(w_dist)
    assert (numpy.isnan(dist) == nan).all() and (dist.view(numpy.uint32)[~nan] == w_dist.view(numpy.uint32)[~nan]).all()
    assert (w_idx[6] == 0xFFFFFFFF).all() and (w_idx[7] == 0xFFFFFFFF)[3:].all() and not nan[0].any()


@pytest.mark.parametrize("table_dtype", DTYPES)
@pytest.mark.parametrize("m,dsub", [(8, 4), (64, 2)])
def test_every_cluster_probed_is_pq_search(m, dsub, table_dtype):
    queries, centroids, books, codes, _ = _data(m, dsub, 21, 200)
    probes = numpy.tile(numpy.arange(K, dtype=numpy.uint32), (21, 1))
    got = ivfpq_search(queries, centroids, books, codes, numpy.arange(L, dtype=numpy.uint32), OFFSETS, probes, 10,
                       table_dtype=table_dtype, residual=False)
    flat = pq_search(queries, books, codes, 10, table_dtype=table_dtype)
    assert got[0].tobytes() == flat[0].tobytes() and got[1].tobytes() == flat[1].tobytes()


def test_index_and_train():
    rs = numpy.random.RandomState(3)
    m, dsub, n = 8, 4, 3000
    rows = rs.randn(n, m * dsub).astype(numpy.float32)
    centroids, labels = rows[:K].copy(), rs.randint(0, K + 1, n).astype(numpy.uint32)      # label K: in no list
    books = ivfpq_train(rows, centroids, m, 64, labels, seed=5, max_iter=3, residual=False)
    want, _, _ = kmeans_batched(rows[labels < K], 64, init="random", max_iter=3, tolerance=0.0, seed=5,
                                layout="columns", problems=m)
    assert books.tobytes() == want.tobytes()
    index = IvfPqIndex(rows, centroids, books, labels, keep_rows=True, residual=False)
    assert index.residual is False and IvfPqIndex(rows, centroids, books, labels).residual is True
    assert (index.ids == numpy.flatnonzero(labels < K)[numpy.argsort(labels[labels < K], kind="stable")]).all()
    assert (index.codes == kmeans_predict_batched(rows, books, layout="columns", dtype=numpy.uint8)[index.ids]).all()
    queries = rs.randn(20, m * dsub).astype(numpy.float32)
    probes = rs.randint(0, K, (20, 3)).astype(numpy.uint32)
    idx, dist = index.search(queries, 10, probes=probes)
    w_idx, w_dist = ivfpq_search(queries, centroids, books, index.codes, index.ids, index.offsets, probes, 10,
                                 residual=False)
    assert idx.tobytes() == w_idx.tobytes() and dist.tobytes() == w_dist.tobytes()
    short, _ = index.search(queries, 20, probes=probes)
    r_idx, r_dist = index.search(queries, 10, probes=probes, refine=2)
    k_idx, k_dist = knn_rerank(queries, rows, short, 10)
    assert r_idx.tobytes() == k_idx.tobytes() and r_dist.tobytes() == k_dist.tobytes()
