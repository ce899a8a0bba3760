"""ivfpq_search(table_dtype="float16") and IvfPqIndex(table_dtype="float16") against a plain numpy
restatement of 4.22 with the rounding inserted, bit for bit; then search(refine=) against knn_rerank."""
import numpy
import pytest

from kmcuda_amd import IvfPqIndex, ivfpq_search, knn_rerank
from kmcuda_amd.ivfpq import query_tile, row_split

pytestmark = pytest.mark.gpu

K = 5
LENS = (0, 1, 255, 257, 700)     # an empty list, one row, one step less a row, a step and a row, three steps
L = sum(LENS)
OFFSETS = numpy.concatenate([[0], numpy.cumsum(LENS)]).astype(numpy.uint32)


def _definition(queries, centroids, books, codes, ids, offsets, probes, k):
    """(indices, distances, a flag: some table held a subnormal half, a flag: some finite entry became +inf)"""
    m_, ksub, dsub = books.shape
    idx = numpy.full((len(queries), k), 0xFFFFFFFF, numpy.uint32)
    dist = numpy.full((len(queries), k), numpy.nan, numpy.float32)
    tiny = huge = False
    for q, x in enumerate(queries):
        keys = [numpy.zeros(0, numpy.uint64)]
        for p in dict.fromkeys(int(v) for v in probes[q] if v < len(centroids)):
            lo, hi = int(offsets[p]), int(offsets[p + 1])
            rows = codes[lo:hi]
            with numpy.errstate(invalid="ignore", over="ignore"):
                t = (x - centroids[p]).reshape(m_, 1, dsub) - books
                t = t * t
                table = numpy.full((m_, 256), numpy.inf, numpy.float32)
                table[:, :ksub] = t[..., 0]
                for j in range(1, dsub):
                    table[:, :ksub] = table[:, :ksub] + t[..., j]
                half = table.astype(numpy.float16).astype(numpy.float32)
                tiny |= bool(((half > 0) & (half < 2.0 ** -14)).any())
                huge |= bool((numpy.isinf(half) & numpy.isfinite(table)).any())
                d = half[0, rows[:, 0]]
                for m in range(1, m_):
                    d = d + half[m, rows[:, m]]
            bits = d.view(numpy.uint32).astype(numpy.uint64)
            bits[numpy.isnan(d)] = 0x7FC00000
            keys.append(bits << numpy.uint64(32) | ids[lo:hi])
        best = numpy.sort(numpy.concatenate(keys))[:k]
        idx[q, :len(best)] = best & numpy.uint64(0xFFFFFFFF)
        dist[q, :len(best)] = (best >> numpy.uint64(32)).astype(numpy.uint32).view(numpy.float32)
    return idx, dist, tiny, huge


def _probes(nq, nprobe, seed=1):
    """Fillers (K) and repeated ids; nobody probes cluster 2, every eighth query only the lists of no and of one row
    (padding at any k > 1), all others cluster 4; query 6 has no valid probe at all."""
    probes = numpy.random.RandomState(seed).randint(0, K + 1, (nq, nprobe)).astype(numpy.uint32)
    probes[probes == 2] = 3
    probes[:, 0] = 4
    lone = numpy.arange(nq) % 8 == 7
    probes[lone] = numpy.where(probes[lone] < K, probes[lone] % 2, K)
    probes[6] = K + 3
    return probes


def _check(m, dsub, nq, nprobe, k, ksub, scale=1.0):
    rs = numpy.random.RandomState(0)
    centroids = (rs.randn(K, m * dsub) * scale).astype(numpy.float32)
    books = (rs.randn(m, ksub, dsub) * scale).astype(numpy.float32)
    codes = rs.randint(0, ksub, (L, m)).astype(numpy.uint8)
    if ksub < 256:
        codes[rs.rand(L) < 0.03, rs.randint(0, m)] = rs.randint(ksub, 256)       # bytes that name no codeword
    ids = rs.permutation(L).astype(numpy.uint32)
    queries = (rs.randn(nq, m * dsub) * scale).astype(numpy.float32)
    queries[1, ::dsub] = numpy.nan
    probes = _probes(nq, nprobe)
    idx, dist = ivfpq_search(queries, centroids, books, codes, ids, OFFSETS, probes, k, table_dtype="float16")
    w_idx, w_dist, tiny, huge = _definition(queries, centroids, books, codes, ids, OFFSETS, probes, k)
    assert idx.dtype == numpy.uint32 and dist.dtype == numpy.float32 and (idx == w_idx).all()
    nan = numpy.isnan(w_dist)
    assert (numpy.isnan(dist) == nan).all() and (dist.view(numpy.uint32)[~nan] == w_dist.view(numpy.uint32)[~nan]).all()
    assert (w_idx[6] == 0xFFFFFFFF).all() and (w_idx[7] == 0xFFFFFFFF)[1:].all()
    return tiny, huge


# (M, dsub): tiles of 16, 16, 8, 4 and 4; byte, dword and 16-byte code loads; codeword loads of 4 and of 16 bytes
SHAPES = [(3, 5), (8, 4), (16, 8), (32, 8), (64, 2)]
# (Q, nprobe, k, ksub): few pairs, every list cut into row splits; then 8500 pairs, no split
CASES = [shape + s for shape in SHAPES for s in ((9, 1, 10, 200), (70, K, 256, 256))] + [(8, 4, 1700, K, 10, 256)]


@pytest.mark.parametrize("m,dsub,nq,nprobe,k,ksub", CASES)
def test_matches_the_definition(monkeypatch, m, dsub, nq, nprobe, k, ksub):
    if (m, nq) == (8, 70):
        monkeypatch.setenv("KMCUDA_AMD_IVFPQ_QUERY_CHUNK", "16")      # five query chunks
    tile = query_tile(m, k, table_dtype="float16")
    assert tile == {3: 16 if k == 10 else 8, 8: 16 if k == 10 else 8, 16: 8 if k == 10 else 4, 32: 4, 64: 4}[m]
    assert (row_split(nq * nprobe, tile, L) == 1) == (nq == 1700)
    _check(m, dsub, nq, nprobe, k, ksub)


@pytest.mark.parametrize("scale", [1e-3, 100.0])
def test_subnormal_and_overflowing_entries(scale):
    tiny, huge = _check(8, 4, 9, 3, 10, 200, scale)
    assert tiny if scale < 1 else huge


def test_index_search_and_refine():
    """The index passes its table_dtype on; refine=2 is knn_rerank of that index's own shortlist."""
    rs = numpy.random.RandomState(3)
    m, dsub, n = 8, 4, 3000
    rows = rs.randn(n, m * dsub).astype(numpy.float32)
    centroids, books = rows[:K].copy(), rs.randn(m, 64, dsub).astype(numpy.float32)
    index = IvfPqIndex(rows, centroids, books, keep_rows=True, table_dtype="float16")
    plain = IvfPqIndex(rows, centroids, books)
    assert index.table_dtype == "float16" and plain.table_dtype == "float32"
    queries = rs.randn(20, m * dsub).astype(numpy.float32)
    probes = rs.randint(0, K, (20, 3)).astype(numpy.uint32)
    idx, dist = index.search(queries, 10, probes=probes)
    w_idx, w_dist, _, _ = _definition(queries, centroids, books, index.codes, index.ids, index.offsets, probes, 10)
    assert (idx == w_idx).all() and dist.tobytes() == w_dist.tobytes()
    assert dist.tobytes() != plain.search(queries, 10, probes=probes)[1].tobytes()
    short, _ = index.search(queries, 20, probes=probes)
    r_idx, r_dist = index.search(queries, 10, probes=probes, refine=2)
    k_idx, k_dist = knn_rerank(queries, rows, short, 10)
    assert r_idx.tobytes() == k_idx.tobytes() and r_dist.tobytes() == k_dist.tobytes()
