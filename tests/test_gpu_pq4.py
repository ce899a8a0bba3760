"""pq_search(bits=4) against a plain numpy float32 restatement of its definition, bit for bit, and,
up to 64 sub-spaces, against pq_search on the same codes one to a byte, byte for byte."""
import numpy
import pytest

from kmcuda_amd import pq_pack4, pq_search
from kmcuda_amd.pq import query_tile

pytestmark = pytest.mark.gpu


def _adc(queries, books, codes):
    """d (Q, N) of the definition in float32: explicit ascending loops over j and m, tables padded to 16 with +inf;
    `codes` one to a byte."""
    (nq, _), (m_, ksub, dsub) = queries.shape, books.shape
    x, y = queries.reshape(nq, m_, 1, dsub), books[None]
    tables = numpy.full((nq, m_, 16), numpy.inf, numpy.float32)
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
    """(queries, codebooks, packed codes, the same codes one to a byte).  Some nibbles >= ksub (never in row n // 2); a
    random high nibble in every row's last byte when m is odd; query 0 is the reconstruction of row n // 2, the last
    of two or more queries holds a NaN in every sub-space."""
    rs = numpy.random.RandomState(seed)
    books = rs.randn(m, ksub, dsub).astype(numpy.float32)
    codes = rs.randint(0, ksub, (n, m)).astype(numpy.uint8)
    if ksub < 16:
        bad = rs.rand(n) < 0.03
        bad[n // 2] = False
        codes[bad, rs.randint(0, m)] = rs.randint(ksub, 16)
    packed = pq_pack4(codes)
    if m % 2:
        packed[:, -1] |= (rs.randint(0, 16, n) << 4).astype(numpy.uint8)
    queries = rs.randn(nq, m * dsub).astype(numpy.float32)
    queries[0] = books[numpy.arange(m), codes[n // 2]].reshape(-1)
    if nq >= 2:
        queries[-1, ::dsub] = numpy.nan
    return queries, books, packed, codes


# (M, dsub, ksub, N, Q, k, queries per chunk or None).  Rows are 1-, 2-, 4-, 4-, 16-, 33-, 64- and 2-byte wide: byte,
# dword and 16-byte loads; few queries cut N = 257 into two row chunks and N = 200 000 into 171 chunks of five steps,
# whose keys the merge takes in batches.
CASES = [
    (1, 1, 1, 1, "one", 1, None),
    (3, 3, 2, 1000, "qt+1", 10, None),          # odd M; at most 8 distinct code rows: the row index decides
    (7, 8, 15, 255, "qt-1", 2, None),
    (8, 3, 15, 600, "qt+1", 10, None),
    (32, 8, 16, 257, "qt+1", 10, None),
    (65, 1, 16, 256, "qt", 256, None),          # beyond the byte codes' 64 sub-spaces; the largest k
    (128, 2, 16, 1000, "tiles", 100, None),     # the widest row, the smallest tile
    (4, 3, 16, 200000, "tiles", 10, None),
    (4, 3, 16, 257, "tiles", 2, 16),            # three query chunks
]


@pytest.mark.parametrize("m,dsub,ksub,n,q_what,k,chunk", CASES)
def test_matches_the_definition(monkeypatch, m, dsub, ksub, n, q_what, k, chunk):
    if chunk:
        monkeypatch.setenv("KMCUDA_AMD_PQ_QUERY_CHUNK", str(chunk))
    qt = query_tile(m, k, bits=4)
    assert qt == (16 if m <= 32 else 4 if m == 128 else 8)
    nq = {"one": 1, "qt-1": qt - 1, "qt": qt, "qt+1": qt + 1, "tiles": 2 * qt + 3}[q_what]
    queries, books, packed, codes = _inputs(m, dsub, ksub, n, nq)
    idx, dist = pq_search(queries, books, packed, k, bits=4)
    assert idx.dtype == numpy.uint32 and dist.dtype == numpy.float32 and idx.shape == dist.shape == (nq, k)

    d32 = _adc(queries, books, codes)
    order = numpy.argsort(d32, axis=1, kind="stable")[:, :k]
    want = numpy.take_along_axis(d32, order, 1)
    assert (idx == order).all()
    nan = numpy.isnan(want)
    assert (numpy.isnan(dist) == nan).all() and (dist.view(numpy.uint32)[~nan] == want.view(numpy.uint32)[~nan]).all()
    assert dist[0, 0] == 0 and (codes[idx[0, 0]] == codes[n // 2]).all()
    if nq >= 2:
        assert (idx[-1] == numpy.arange(k)).all() and numpy.isnan(dist[-1]).all()
    if m <= 64:
        b_idx, b_dist = pq_search(queries, books, codes, k)
        assert idx.tobytes() == b_idx.tobytes() and dist.tobytes() == b_dist.tobytes()


def test_same_bytes_twice_and_from_device_tensors():
    import torch
    queries, books, packed, _ = _inputs(9, 4, 16, 5000, 9, seed=1)
    idx, dist = pq_search(queries, books, packed, 100, bits=4)
    again = pq_search(queries, books, packed, 100, bits=4)
    assert idx.tobytes() == again[0].tobytes() and dist.tobytes() == again[1].tobytes()
    dev = torch.device("cuda", 0)
    t_idx, t_dist = pq_search(*(torch.from_numpy(a).to(dev) for a in (queries, books, packed)), 100, bits=4)
    assert t_idx.is_cuda and t_idx.dtype == torch.int32 and t_dist.dtype == torch.float32
    assert t_idx.cpu().numpy().tobytes() == idx.tobytes() and t_dist.cpu().numpy().tobytes() == dist.tobytes()
