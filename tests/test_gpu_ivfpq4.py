"""ivfpq_search(bits=4) against one plain numpy float32 restatement of its definition -- indices and
distance bits equal, NaN on the padding -- and, up to 64 sub-spaces, against the search over the same codes one to a
byte, byte for byte; then the pipeline from training to a refined search."""
import numpy
import pytest

from kmcuda_amd import IvfPqIndex, ivfpq_search, ivfpq_train, pq_pack4
from kmcuda_amd.ivfpq import query_tile, row_split

pytestmark = pytest.mark.gpu

K = 5
LENS = (0, 1, 255, 257, 700)     # an empty list, one row, one step less a row, a step and a row, three steps
L = sum(LENS)
OFFSETS = numpy.concatenate([[0], numpy.cumsum(LENS)]).astype(numpy.uint32)


def _definition(queries, centroids, books, codes, ids, offsets, probes, k):
    """(indices, distances) of the definition: explicit ascending sums over j and m, one table per (query, probe);
    `codes` one to a byte."""
    m_, ksub, dsub = books.shape
    idx = numpy.full((len(queries), k), 0xFFFFFFFF, numpy.uint32)
    dist = numpy.full((len(queries), k), numpy.nan, numpy.float32)
    for q, x in enumerate(queries):
        keys = [numpy.zeros(0, numpy.uint64)]
        for p in dict.fromkeys(int(v) for v in probes[q] if v < len(centroids)):
            lo, hi = int(offsets[p]), int(offsets[p + 1])
            rows = codes[lo:hi]
            with numpy.errstate(invalid="ignore", over="ignore"):
                t = (x - centroids[p]).reshape(m_, 1, dsub) - books
                t = t * t
                table = numpy.full((m_, 16), numpy.inf, numpy.float32)
                table[:, :ksub] = t[..., 0]
                for j in range(1, dsub):
                    table[:, :ksub] = table[:, :ksub] + t[..., j]
                d = table[0, rows[:, 0]]
                for m in range(1, m_):
                    d = d + table[m, rows[:, m]]
            bits = d.view(numpy.uint32).astype(numpy.uint64)
            bits[numpy.isnan(d)] = 0x7FC00000
            keys.append(bits << numpy.uint64(32) | ids[lo:hi])
        best = numpy.sort(numpy.concatenate(keys))[:k]
        idx[q, :len(best)] = best & numpy.uint64(0xFFFFFFFF)
        dist[q, :len(best)] = (best >> numpy.uint64(32)).astype(numpy.uint32).view(numpy.float32)
    return idx, dist


def _probes(nq, nprobe, seed=1):
    """Caller probes with fillers (K) and repeated ids.  No query probes cluster 2; every eighth probes the lists of
    no and of one row only (padding at any k > 1), all others cluster 4."""
    probes = numpy.random.RandomState(seed).randint(0, K + 1, (nq, nprobe)).astype(numpy.uint32)
    probes[probes == 2] = 3
    probes[:, 0] = 4
    lone = numpy.arange(nq) % 8 == 7
    probes[lone] = numpy.where(probes[lone] < K, probes[lone] % 2, K)
    return probes


# (M, dsub): code rows of 1, 4, 4, 9, 3, 2, 16, 32, 33 and 64 bytes -- byte, dword and 16-byte loads, odd and even M;
# sub-spaces of one table pass with and without 16-byte codeword loads (4, 8; 1, 2, 3) and of two (12; 11)
SHAPES = [(1, 3), (7, 2), (8, 4), (17, 1), (6, 12), (3, 11), (32, 8), (63, 1), (65, 1), (128, 2)]
# (Q, nprobe, k, ksub): few pairs, every list cut into row splits; then 8500 pairs at a tile of 16, no split
CASES = [shape + s for shape in SHAPES for s in ((9, 1, 10, 13), (70, K, 256, 16))] + [(8, 4, 1700, K, 10, 16)]


@pytest.mark.parametrize("m,dsub,nq,nprobe,k,ksub", CASES)
def test_matches_the_definition(m, dsub, nq, nprobe, k, ksub):
    assert (row_split(nq * nprobe, query_tile(m, k, bits=4), L) == 1) == (nq == 1700)
    rs = numpy.random.RandomState(0)
    centroids = rs.randn(K, m * dsub).astype(numpy.float32)
    books = rs.randn(m, ksub, dsub).astype(numpy.float32)
    codes = rs.randint(0, ksub, (L, m)).astype(numpy.uint8)
    if ksub < 16:
        codes[rs.rand(L) < 0.03, rs.randint(0, m)] = rs.randint(ksub, 16)      # nibbles that name no codeword
    ids = rs.permutation(L).astype(numpy.uint32)
    packed = pq_pack4(codes)
    if m % 2:
        packed[:, -1] |= (rs.randint(0, 16, L) << 4).astype(numpy.uint8)       # ignored
    queries = rs.randn(nq, m * dsub).astype(numpy.float32)
    probes = _probes(nq, nprobe)
    idx, dist = ivfpq_search(queries, centroids, books, packed, ids, OFFSETS, probes, k, bits=4)
    w_idx, w_dist = _definition(queries, centroids, books, codes, ids, OFFSETS, probes, k)
    assert idx.dtype == numpy.uint32 and dist.dtype == numpy.float32 and (idx == w_idx).all()
    nan = numpy.isnan(w_dist)
    assert (numpy.isnan(dist) == nan).all() and (dist.view(numpy.uint32)[~nan] == w_dist.view(numpy.uint32)[~nan]).all()
    assert (w_idx[7] == 0xFFFFFFFF)[1:].all()                                  # at most one row in reach of query 7
    if m <= 64:
        b_idx, b_dist = ivfpq_search(queries, centroids, books, codes, ids, OFFSETS, probes, k)
        assert idx.tobytes() == b_idx.tobytes() and dist.tobytes() == b_dist.tobytes()


def test_train_build_search_refine():
    """Rows that are a coarse centre plus a product of 4 sub-space blobs: a row's own codes name the nearest codeword
    of every sub-space, so nothing in reach scores below them; the refined search finds the row itself."""
    rs = numpy.random.RandomState(7)
    m, dsub, n = 4, 8, 2000
    coarse = (100 * rs.randn(K, m * dsub)).astype(numpy.float32)
    blobs = 10 * rs.randn(m, 16, dsub)
    rows = blobs[numpy.arange(m), rs.randint(0, 16, (n, m))] + 0.1 * rs.randn(n, m, dsub)
    rows = (coarse[rs.randint(0, K, n)] + rows.reshape(n, m * dsub)).astype(numpy.float32)
    books = ivfpq_train(rows, coarse, m, ksub=16, seed=1, max_iter=10)
    index = IvfPqIndex(rows, coarse, books, bits=4, keep_rows=True)
    assert index.bits == 4 and index.codes.shape == (n, m // 2) and index.codes.dtype == numpy.uint8
    assert sorted(index.ids) == list(range(n))
    sample = numpy.arange(0, n, 97)
    idx, _ = index.search(rows[sample], 5, nprobe=K)
    where = numpy.argsort(index.ids)                     # list position of every row
    assert (index.codes[where[idx[:, 0]]] == index.codes[where[sample]]).all()
    idx, dist = index.search(rows[sample], 5, nprobe=K, refine=2)
    assert (idx[:, 0] == sample).all() and (dist[:, 0] == 0).all()
