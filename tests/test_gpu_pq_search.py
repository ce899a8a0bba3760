"""pq_search against two plain numpy restatements of its definition: float32, bit for bit, and
float64, within the derived rounding bound."""
import numpy
import pytest

from kmcuda_amd import kmeans_batched, kmeans_predict_batched, pq_search
from kmcuda_amd.pq import query_tile

pytestmark = pytest.mark.gpu


def _adc(queries, books, codes, dtype):
    """d (Q, N) of the definition in `dtype`: explicit ascending loops over j and m, tables padded to 256 with +inf."""
    (nq, _), (m_, ksub, dsub) = queries.shape, books.shape
    x, y = queries.astype(dtype).reshape(nq, m_, 1, dsub), books.astype(dtype)[None]
    tables = numpy.full((nq, m_, 256), numpy.inf, dtype)
    with numpy.errstate(invalid="ignore", over="ignore"):
        for j in range(dsub):
            t = x[..., j] - y[..., j]
            acc = t * t if j == 0 else acc + t * t
        tables[:, :, :ksub] = acc
        for m in range(m_):
            term = tables[:, m, codes[:, m]]
            d = term if m == 0 else d + term
    return d


def _inputs(m, dsub, ksub, n, nq, seed=0):
    """A corpus with some code bytes >= ksub (never in row n // 2); query 0 is the reconstruction of row n // 2, the
    last of two or more queries holds a NaN."""
    rs = numpy.random.RandomState(seed)
    books = rs.randn(m, ksub, dsub).astype(numpy.float32)
    codes = rs.randint(0, ksub, (n, m)).astype(numpy.uint8)
    if ksub < 256:
        bad = rs.rand(n) < 0.03
        bad[n // 2] = False
        codes[bad, rs.randint(0, m)] = rs.randint(ksub, 256)
    queries = rs.randn(nq, m * dsub).astype(numpy.float32)
    queries[0] = books[numpy.arange(m), codes[n // 2]].reshape(-1)
    if nq >= 2:
        queries[-1, ::dsub] = numpy.nan          # in every sub-space: NaN beats the +inf of a byte >= ksub
    return queries, books, codes


def _qt(m, k, what):
    qt = query_tile(m, k)
    return {"one": 1, "qt-1": max(1, qt - 1), "qt": qt, "qt+1": qt + 1, "tiles": 2 * qt + 3}[what]


# (M, dsub, ksub, N, Q, k, queries per chunk or None).  Row chunks: ceil(512 / query tiles) of them, in whole 256-row
# tiles -- so with a few queries N = 257 is two chunks, N = 1000 and 3000 are 4 and 12 chunks of one step, and
# N = 200 000 under three query tiles is 157 chunks of five steps, whose 1570 keys per query the merge takes in batches.
CASES = [
    (1, 1, 1, 1, "one", 1, None),
    (3, 3, 2, 1000, "qt+1", 10, None),          # at most 8 distinct code rows: the row index decides nearly everything
    (4, 8, 255, 255, "qt-1", 2, None),
    (8, 3, 255, 600, "qt+1", 10, None),
    (17, 3, 256, 256, "qt", 256, None),
    (32, 8, 256, 257, "qt+1", 10, None),        # 16-byte code loads
    (32, 1, 2, 3000, "one", 256, None),
    (64, 64, 255, 1000, "tiles", 100, None),    # the smallest query tile
    (3, 8, 256, 200000, "tiles", 10, None),
    (4, 3, 256, 257, "tiles", 2, 16),           # three query chunks
]


@pytest.mark.parametrize("m,dsub,ksub,n,q_what,k,chunk", CASES)
def test_matches_the_definition(monkeypatch, m, dsub, ksub, n, q_what, k, chunk):
    if chunk:
        monkeypatch.setenv("KMCUDA_AMD_PQ_QUERY_CHUNK", str(chunk))
    k = min(k, n)
    nq = _qt(m, k, q_what)
    queries, books, codes = _inputs(m, dsub, ksub, n, nq)
    idx, dist = pq_search(queries, books, codes, k)
    assert idx.dtype == numpy.uint32 and dist.dtype == numpy.float32 and idx.shape == dist.shape == (nq, k)

    d32 = _adc(queries, books, codes, numpy.float32)
    order = numpy.argsort(d32, axis=1, kind="stable")[:, :k]
    want = numpy.take_along_axis(d32, order, 1)
    assert (idx == order).all()
    nan = numpy.isnan(want)
    assert (numpy.isnan(dist) == nan).all() and (dist.view(numpy.uint32)[~nan] == want.view(numpy.uint32)[~nan]).all()
    assert dist[0, 0] == 0 and (codes[idx[0, 0]] == codes[n // 2]).all()
    if nq >= 2 and m >= 2:
        assert (idx[-1] == numpy.arange(k)).all() and numpy.isnan(dist[-1]).all()
    rows_inf = numpy.isinf(d32[0])
    assert not rows_inf[idx[0, :min(k, int((~rows_inf).sum()))]].any()     # every finite row before a row at +inf

    d64 = _adc(queries, books, codes, numpy.float64)
    gamma = (dsub + m + 2) * 2.0 ** -24
    true = numpy.take_along_axis(d64, idx.astype(numpy.int64), 1)
    finite = numpy.isfinite(dist)
    assert (numpy.abs(dist[finite] - true[finite]) <= gamma * true[finite]).all()
    kth = numpy.sort(d64, axis=1)[:, k - 1]
    ok = ~numpy.isnan(kth)
    assert (dist[ok, k - 1] <= (1 + 2 * gamma) * kth[ok]).all()


def test_same_bytes_twice_and_from_device_tensors():
    import torch
    queries, books, codes = _inputs(8, 4, 256, 5000, 9, seed=1)
    idx, dist = pq_search(queries, books, codes, 100)
    again = pq_search(queries, books, codes, 100)
    assert idx.tobytes() == again[0].tobytes() and dist.tobytes() == again[1].tobytes()
    dev = torch.device("cuda", 0)
    t_idx, t_dist = pq_search(*(torch.from_numpy(a).to(dev) for a in (queries, books, codes)), 100)
    assert t_idx.is_cuda and t_idx.dtype == torch.int32 and t_dist.dtype == torch.float32
    assert t_idx.cpu().numpy().tobytes() == idx.tobytes() and t_dist.cpu().numpy().tobytes() == dist.tobytes()


def test_train_encode_search():
    """Blobs that are products of 4 well separated sub-space blobs: a corpus row's own code is the nearest codeword in
    every sub-space, so no row scores below it."""
    rs = numpy.random.RandomState(2)
    m, dsub, ksub, n = 4, 8, 4, 2000
    centres = 10 * rs.randn(m, ksub, dsub)
    x = (centres[numpy.arange(m), rs.randint(0, ksub, (n, m))] + 0.1 * rs.randn(n, m, dsub)).astype(numpy.float32)
    x = x.reshape(n, m * dsub)
    books, _, _ = kmeans_batched(x, ksub, init=centres.astype(numpy.float32), layout="columns", max_iter=20)
    codes = kmeans_predict_batched(x, books, layout="columns", dtype=numpy.uint8)
    rows = numpy.arange(0, n, 97)
    idx, dist = pq_search(x[rows], books, codes, 5)
    own = _adc(x[rows], books, codes, numpy.float32)[numpy.arange(len(rows)), rows]
    assert dist[:, 0].tobytes() == own.tobytes()
    assert (codes[idx[:, 0]] == codes[rows]).all()
