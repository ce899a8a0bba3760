"""pq_search(table_dtype="float16") against a plain numpy restatement of its definition, bit for bit:
the fp32 tables rounded once by astype(float16), widened again and summed in ascending m in float32."""
import numpy
import pytest

from kmcuda_amd import pq_search
from kmcuda_amd.pq import query_tile

pytestmark = pytest.mark.gpu


def _tables(queries, books):
    """(T32, T16 widened), each (Q, M, 256) float32: explicit ascending loop over j, +inf for c >= ksub"""
    (nq, _), (m_, ksub, dsub) = queries.shape, books.shape
    x, y = queries.reshape(nq, m_, 1, dsub), books[None]
    t32 = numpy.full((nq, m_, 256), numpy.inf, numpy.float32)
    with numpy.errstate(invalid="ignore", over="ignore"):
        for j in range(dsub):
            t = x[..., j] - y[..., j]
            acc = t * t if j == 0 else acc + t * t
        t32[:, :, :ksub] = acc
        return t32, t32.astype(numpy.float16).astype(numpy.float32)


def _inputs(m, dsub, ksub, n, nq, scale=1.0, seed=0):
    """Some codes >= ksub (never in row n // 2); query 0 reconstructs row n // 2, the last of two or more is NaN."""
    rs = numpy.random.RandomState(seed)
    books = (rs.randn(m, ksub, dsub) * scale).astype(numpy.float32)
    codes = rs.randint(0, ksub, (n, m)).astype(numpy.uint8)
    if ksub < 256:
        bad = rs.rand(n) < 0.03
        bad[n // 2] = False
        codes[bad, rs.randint(0, m)] = rs.randint(ksub, 256)
    queries = (rs.randn(nq, m * dsub) * scale).astype(numpy.float32)
    queries[0] = books[numpy.arange(m), codes[n // 2]].reshape(-1)
    if nq >= 2:
        queries[-1, ::dsub] = numpy.nan
    return queries, books, codes


def _check(m, dsub, ksub, n, q_what, k, tile, scale=1.0):
    qt = query_tile(m, k, table_dtype="float16")
    assert qt == tile
    nq = {"one": 1, "qt-1": qt - 1, "qt": qt, "qt+1": qt + 1, "tiles": 2 * qt + 3}[q_what]
    queries, books, codes = _inputs(m, dsub, ksub, n, nq, scale)
    idx, dist = pq_search(queries, books, codes, k, table_dtype="float16")
    assert idx.dtype == numpy.uint32 and dist.dtype == numpy.float32 and idx.shape == dist.shape == (nq, k)
    t32, t16 = _tables(queries, books)
    with numpy.errstate(invalid="ignore"):
        for s in range(m):
            d32 = t16[:, s, codes[:, s]] if s == 0 else d32 + t16[:, s, codes[:, s]]
    order = numpy.argsort(d32, axis=1, kind="stable")[:, :k]
    want = numpy.take_along_axis(d32, order, 1)
    assert (idx == order).all()
    nan = numpy.isnan(want)
    assert (numpy.isnan(dist) == nan).all() and (dist.view(numpy.uint32)[~nan] == want.view(numpy.uint32)[~nan]).all()
    assert dist[0, 0] == 0 and (codes[idx[0, 0]] == codes[n // 2]).all()
    if nq >= 2:
        assert (idx[-1] == numpy.arange(k)).all() and numpy.isnan(dist[-1]).all()
    return queries, books, codes, dist, t32[:, :, :ksub], t16[:, :, :ksub]


# (M, dsub, ksub, N, Q, k, the tile of the rule); N = 257 is two row chunks, N = 200 000 many, merged in batches
CASES = [
    (1, 1, 1, 1, "one", 1, 16),
    (3, 3, 200, 1000, "qt+1", 10, 16),          # byte loads, +inf codes
    (8, 4, 256, 257, "qt+1", 10, 16),           # the last M at a tile of 16
    (9, 2, 256, 600, "qt-1", 2, 8),             # the first at 8
    (16, 8, 256, 513, "tiles", 10, 8),          # 16-byte loads at a tile of 8
    (19, 1, 256, 300, "qt", 256, 4),            # the first M at 4; the largest k
    (32, 8, 256, 257, "qt+1", 10, 4),           # two blocks per CU
    (39, 1, 256, 300, "qt+1", 10, 4),           # the first M with one block
    (64, 2, 256, 1000, "tiles", 100, 4),        # the widest row
    (4, 3, 16, 200000, "tiles", 10, 16),
    (4, 3, 16, 257, "tiles", 2, 16),            # run with three query chunks
]


@pytest.mark.parametrize("m,dsub,ksub,n,q_what,k,tile", CASES)
def test_matches_the_definition(monkeypatch, m, dsub, ksub, n, q_what, k, tile):
    if (n, k) == (257, 2):
        monkeypatch.setenv("KMCUDA_AMD_PQ_QUERY_CHUNK", "16")
    queries, books, codes, dist, _, _ = _check(m, dsub, ksub, n, q_what, k, tile)
    if m == 32:                                 # the option is not ignored
        assert dist.tobytes() != pq_search(queries, books, codes, k)[1].tobytes()


@pytest.mark.parametrize("m,dsub,ksub,n,q_what,k,tile", [CASES[1], CASES[6]])
@pytest.mark.parametrize("scale", [1e-3, 100.0])
def test_subnormal_and_overflowing_entries(m, dsub, ksub, n, q_what, k, tile, scale):
    _, _, _, _, t32, t16 = _check(m, dsub, ksub, n, q_what, k, tile, scale)
    live = t16[:-1]                             # the last query is NaN
    if scale < 1:
        assert ((live > 0) & (live < 2.0 ** -14)).any()
    else:
        assert numpy.isfinite(live).any() and (numpy.isinf(live) & numpy.isfinite(t32[:-1])).any()


def test_same_bytes_twice_and_from_device_tensors():
    import torch
    queries, books, codes = _inputs(9, 4, 100, 5000, 9, seed=1)
    idx, dist = pq_search(queries, books, codes, 100, table_dtype="float16")
    again = pq_search(queries, books, codes, 100, table_dtype="float16")
    assert idx.tobytes() == again[0].tobytes() and dist.tobytes() == again[1].tobytes()
    dev = torch.device("cuda", 0)
    t_idx, t_dist = pq_search(*(torch.from_numpy(a).to(dev) for a in (queries, books, codes)), 100,
                              table_dtype="float16")
    assert t_idx.is_cuda and t_idx.dtype == torch.int32 and t_dist.dtype == torch.float32
    assert t_idx.cpu().numpy().tobytes() == idx.tobytes() and t_dist.cpu().numpy().tobytes() == dist.tobytes()
