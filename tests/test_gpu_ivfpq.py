"""IVF-PQ search against one plain numpy float32 restatement of its definition: indices and distance
bits equal, NaN on the padding."""
import numpy
import pytest

from kmcuda_amd import IvfPqIndex, ivfpq_search, ivfpq_train, kmeans_predict, kmeans_predict_top, pq_search
from kmcuda_amd.ivfpq import query_tile, row_split

pytestmark = pytest.mark.gpu

K = 5
LENS = (0, 1, 255, 257, 700)     # an empty list, one row, one step less a row, a step and a row, three steps
L = sum(LENS)
OFFSETS = numpy.concatenate([[0], numpy.cumsum(LENS)]).astype(numpy.uint32)


def _definition(queries, centroids, books, codes, ids, offsets, probes, k):
    """(indices, distances) of the definition: explicit ascending sums over j and m, one table per (query, probe)."""
    m_, ksub, dsub = books.shape
    idx = numpy.full((len(queries), k), 0xFFFFFFFF, numpy.uint32)
    dist = numpy.full((len(queries), k), numpy.nan, numpy.float32)
    for q, x in enumerate(queries):
        keys = [numpy.zeros(0, numpy.uint64)]
        for p in dict.fromkeys(int(v) for v in probes[q] if v < len(centroids)):
            lo, hi = min(int(offsets[p]), len(codes)), min(int(offsets[p + 1]), len(codes))
            rows = codes[lo:max(lo, hi)]
            with numpy.errstate(invalid="ignore", over="ignore"):
                t = (x - centroids[p]).reshape(m_, 1, dsub) - books
                t = t * t
                table = numpy.full((m_, 256), numpy.inf, numpy.float32)
                table[:, :ksub] = t[..., 0]
                for j in range(1, dsub):
                    table[:, :ksub] = table[:, :ksub] + t[..., j]
                d = table[0, rows[:, 0]]
                for m in range(1, m_):
                    d = d + table[m, rows[:, m]]
            bits = d.view(numpy.uint32).astype(numpy.uint64)
            bits[numpy.isnan(d)] = 0x7FC00000
            keys.append(bits << numpy.uint64(32) | ids[lo:max(lo, hi)])
        best = numpy.sort(numpy.concatenate(keys))[:k]
        idx[q, :len(best)] = best & numpy.uint64(0xFFFFFFFF)
        dist[q, :len(best)] = (best >> numpy.uint64(32)).astype(numpy.uint32).view(numpy.float32)
    return idx, dist


def _same(got, want):
    (idx, dist), (w_idx, w_dist) = got, want
    assert idx.dtype == numpy.uint32 and dist.dtype == numpy.float32 and idx.shape == dist.shape == w_idx.shape
    assert (idx == w_idx).all()
    nan = numpy.isnan(w_dist)
    assert (numpy.isnan(dist) == nan).all() and (dist.view(numpy.uint32)[~nan] == w_dist.view(numpy.uint32)[~nan]).all()


def _index(m, dsub, ksub, duplicated=False, seed=0):
    rs = numpy.random.RandomState(seed)
    centroids = rs.randn(K, m * dsub).astype(numpy.float32)
    books = rs.randn(m, ksub, dsub).astype(numpy.float32)
    codes = rs.randint(0, ksub, (L, m)).astype(numpy.uint8)
    if ksub < 256:
        codes[rs.rand(L) < 0.03, rs.randint(0, m)] = rs.randint(ksub, 256)     # bytes that name no codeword
    if duplicated:
        codes = codes[OFFSETS[4] + rs.randint(0, 4, L)]                        # four distinct rows: the id decides
    return centroids, books, codes, rs.permutation(L).astype(numpy.uint32)


def _probes(nq, nprobe, seed=1):
    """Caller probes with fillers (K) and repeated ids.  No query probes cluster 2; every eighth probes the lists of
    no and of one row only (padding at any k > 1), all others cluster 4."""
    probes = numpy.random.RandomState(seed).randint(0, K + 1, (nq, nprobe)).astype(numpy.uint32)
    probes[probes == 2] = 3
    probes[:, 0] = 4
    lone = numpy.arange(nq) % 8 == 7
    probes[lone] = numpy.where(probes[lone] < K, probes[lone] % 2, K)
    return probes


# (Q, nprobe, k, ksub, queries per chunk or None, duplicated code rows)
SCENARIOS = [
    (1, 1, 1, 256, None, False),
    (3, 3, 10, 200, None, False),
    (70, K, 256, 256, None, False),      # more pairs of cluster 4 than any tile
    (70, 3, 10, 256, 32, True),          # three query chunks
]


@pytest.mark.parametrize("nq,nprobe,k,ksub,chunk,duplicated", SCENARIOS)
@pytest.mark.parametrize("m,dsub", [(1, 3), (4, 4), (8, 2), (17, 1), (32, 2), (64, 1)])
def test_matches_the_definition(monkeypatch, m, dsub, nq, nprobe, k, ksub, chunk, duplicated):
    if chunk:
        monkeypatch.setenv("KMCUDA_AMD_IVFPQ_QUERY_CHUNK", str(chunk))
    assert query_tile(m, 10) == {1: 16, 4: 16, 8: 8, 17: 4, 32: 4, 64: 2}[m]
    assert row_split(nq * nprobe, query_tile(m, k), L) > 1
    centroids, books, codes, ids = _index(m, dsub, ksub, duplicated)
    queries = numpy.random.RandomState(2).randn(nq, m * dsub).astype(numpy.float32)
    probes = _probes(nq, nprobe)
    want = _definition(queries, centroids, books, codes, ids, OFFSETS, probes, k)
    _same(ivfpq_search(queries, centroids, books, codes, ids, OFFSETS, probes, k), want)
    assert (want[0][:, -1] == 0xFFFFFFFF).any() == (nq == 70)      # k beyond the rows query 7 reaches


@pytest.mark.parametrize("m,dsub,nq,nprobe", [(64, 1, 1100, 1), (32, 2, 70, 3), (17, 1, 3, K)])
def test_one_row_split_device_tensors_and_unaligned_lists(m, dsub, nq, nprobe):
    """Torch operands; the code matrix starts 4 bytes into its buffer, so no row is 16-byte aligned; lists that end
    before they start or past L; Q = 1100 at a tile of 2 reaches 512 tiles on its own: no row split."""
    import torch
    assert (row_split(nq * nprobe, query_tile(m, 10), L) == 1) == (nq == 1100)
    centroids, books, codes, ids = _index(m, dsub, 256, seed=3)
    queries = numpy.random.RandomState(4).randn(nq, m * dsub).astype(numpy.float32)
    probes = _probes(nq, nprobe)
    offsets = numpy.array([900, 0, 256, 513, 1100, 0xFFFFFFF0], numpy.uint32)
    want = _definition(queries, centroids, books, codes, ids, offsets, probes, 10)
    dev = torch.device("cuda", 0)
    raw = torch.zeros(4 + L * m, dtype=torch.uint8, device=dev)
    raw[4:] = torch.from_numpy(codes).to(dev).reshape(-1)
    ops = [torch.from_numpy(a).to(dev) for a in (queries, centroids, books)]
    ints = [torch.from_numpy(a.view(numpy.int32)).to(dev) for a in (ids, offsets, probes)]
    t_idx, t_dist = ivfpq_search(*ops, raw[4:].view(L, m), *ints, 10)
    assert t_idx.is_cuda and t_idx.dtype == torch.int32 and t_dist.dtype == torch.float32
    _same((t_idx.cpu().numpy().view(numpy.uint32), t_dist.cpu().numpy()), want)


def test_zero_centroids_equal_pq_search():
    """With all-zero centroids the residual is the query: probing every list is pq_search over the same codes."""
    _, books, codes, _ = _index(8, 4, 256, seed=5)
    ids = (3 * numpy.arange(L) + 1).astype(numpy.uint32)      # ascending: ties fall the same way in both
    queries = numpy.random.RandomState(6).randn(9, 32).astype(numpy.float32)
    probes = numpy.tile(numpy.arange(K, dtype=numpy.uint32), (9, 1))
    idx, dist = ivfpq_search(queries, numpy.zeros((K, 32), numpy.float32), books, codes, ids, OFFSETS, probes, 100)
    p_idx, p_dist = pq_search(queries, books, codes, 100)
    assert (idx == ids[p_idx]).all() and dist.tobytes() == p_dist.tobytes()


def test_train_build_search():
    rs = numpy.random.RandomState(7)
    centres = (4 * rs.randn(K, 16)).astype(numpy.float32)
    rows = (centres[rs.randint(0, K, 2000)] + rs.randn(2000, 16)).astype(numpy.float32)
    books = ivfpq_train(rows, centres, 4, ksub=16, seed=1, max_iter=10)
    assert books.shape == (4, 16, 4) and books.dtype == numpy.float32
    index = IvfPqIndex(rows, centres, books)
    assert index.codes.shape == (2000, 4) and sorted(index.ids) == list(range(2000)) and index.offsets[-1] == 2000
    queries = rows[::100].copy()
    queries[-1, 0] = numpy.nan                       # no cluster: kmeans_predict_top fills its probes with K
    got = index.search(queries, 10, nprobe=2)
    probes = kmeans_predict_top(queries, centres, 2, return_distances=False)
    _same(got, _definition(queries, centres, books, index.codes, index.ids, index.offsets, probes, 10))
    assert (got[0][-1] == 0xFFFFFFFF).all() and numpy.isnan(got[1][-1]).all()
    # the index itself: a list holds the rows of its cluster, a row's bytes name the codeword nearest to its residual
    cluster = numpy.repeat(numpy.arange(K), numpy.diff(index.offsets.astype(numpy.int64)))
    assert (cluster == kmeans_predict(rows, centres)[index.ids]).all()
    res = (rows[index.ids].astype(numpy.float64) - centres[cluster]).reshape(2000, 4, 1, 4)
    d = ((res - books.astype(numpy.float64)) ** 2).sum(-1)                    # (rows, M, ksub)
    chosen = numpy.take_along_axis(d, index.codes[..., None].astype(numpy.int64), 2)[..., 0]
    assert (chosen <= d.min(-1) * (1 + 1e-5) + 1e-6).all()
