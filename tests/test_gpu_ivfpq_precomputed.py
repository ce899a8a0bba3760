"""IVF-PQ search from precomputed terms against one plain numpy float32 restatement of its definition:
the terms, the indices and the distance bits equal, every distance within the running-error bound of the exact one."""
import numpy
import pytest

from kmcuda_amd import IvfPqIndex, ivfpq_search, ivfpq_terms, ivfpq_train, kmeans_predict_top, knn_rerank
from test_gpu_ivfpq import K, L, OFFSETS, _index, _probes, _same

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3), (8, 2), (17, 1), (32, 2), (64, 1)]      # (M, dsub): pair tiles 16 / 8 / 4 / 4 / 2
TWO, ZERO = numpy.float32(2), numpy.float32(0)


def _chain(terms):
    """The sum over the last axis in ascending index, from the first term."""
    acc = terms[..., 0]
    for j in range(1, terms.shape[-1]):
        acc = acc + terms[..., j]
    return acc


def _terms(centroids, books):
    m_, _, dsub = books.shape
    g = centroids.reshape(len(centroids), m_, 1, dsub)
    return _chain(books * books)[None] + TWO * _chain(g * books[None])


def _definition(queries, centroids, books, codes, ids, offsets, probes, k, terms, sums=None):
    """(indices, distances) of the definition; `sums` collects the sums before the clamp."""
    m_, ksub, dsub = books.shape
    idx = numpy.full((len(queries), k), 0xFFFFFFFF, numpy.uint32)
    dist = numpy.full((len(queries), k), numpy.nan, numpy.float32)
    for q, x in enumerate(queries):
        keys = [numpy.zeros(0, numpy.uint64)]
        with numpy.errstate(invalid="ignore", over="ignore"):
            b = _chain(x.reshape(m_, 1, dsub) * books)
        for p in dict.fromkeys(int(v) for v in probes[q] if v < len(centroids)):
            lo, hi = min(int(offsets[p]), len(codes)), min(int(offsets[p + 1]), len(codes))
            rows = codes[lo:max(lo, hi)]
            with numpy.errstate(invalid="ignore", over="ignore"):
                table = numpy.full((m_, 256), numpy.inf, numpy.float32)
                table[:, :ksub] = terms[p] - TWO * b
                r = x - centroids[p]
                d = table[0, rows[:, 0]]
                for m in range(1, m_):
                    d = d + table[m, rows[:, m]]
                d = _chain(r * r) + d
            if sums is not None:
                sums.append(d)
            d = numpy.where(d <= 0, ZERO, d)
            bits = d.view(numpy.uint32).astype(numpy.uint64)
            bits[numpy.isnan(d)] = 0x7FC00000
            keys.append(bits << numpy.uint64(32) | ids[lo:max(lo, hi)])
        best = numpy.sort(numpy.concatenate(keys))[:k]
        idx[q, :len(best)] = best & numpy.uint64(0xFFFFFFFF)
        dist[q, :len(best)] = (best >> numpy.uint64(32)).astype(numpy.uint32).view(numpy.float32)
    return idx, dist


def _within_the_error_bound(got, queries, centroids, books, codes, ids):
    """|d - exact| <= (D + M + dsub + 8) 2^-24 S, S the float64 sum of the absolute terms of the three chains."""
    idx, dist = got
    m_, _, dsub = books.shape
    q, slot = numpy.nonzero(numpy.isfinite(dist))
    pos = numpy.argsort(ids)[idx[q, slot]]
    x = queries[q].astype(numpy.float64)
    g = centroids[numpy.searchsorted(OFFSETS, pos, "right") - 1].astype(numpy.float64)
    y = books.astype(numpy.float64)[numpy.arange(m_)[None], codes[pos]].reshape(len(pos), -1)
    exact = ((x - g - y) ** 2).sum(1)
    s = ((x - g) ** 2).sum(1) + (y * y + 2 * abs(g * y) + 2 * abs(x * y)).sum(1)
    assert (abs(dist[q, slot] - exact) <= (m_ * dsub + m_ + dsub + 8) * 2.0 ** -24 * s).all()


@pytest.mark.parametrize("nq,nprobe,k,ksub,chunk", [(1, 1, 1, 256, None), (3, 3, 10, 200, None),
                                                    (70, K, 256, 256, None), (70, 3, 10, 256, 32)])
@pytest.mark.parametrize("m,dsub", SHAPES)
def test_matches_the_definition(monkeypatch, m, dsub, nq, nprobe, k, ksub, chunk):
    if chunk:
        monkeypatch.setenv("KMCUDA_AMD_IVFPQ_QUERY_CHUNK", str(chunk))
    centroids, books, codes, ids = _index(m, dsub, ksub)
    queries = numpy.random.RandomState(2).randn(nq, m * dsub).astype(numpy.float32)
    probes = _probes(nq, nprobe)
    terms = ivfpq_terms(centroids, books)
    want_terms = _terms(centroids, books)
    assert terms.dtype == numpy.float32 and terms.shape == (K, m, ksub) and terms.tobytes() == want_terms.tobytes()
    want = _definition(queries, centroids, books, codes, ids, OFFSETS, probes, k, want_terms)
    got = ivfpq_search(queries, centroids, books, codes, ids, OFFSETS, probes, k, terms=terms)
    _same(got, want)
    assert (want[0][:, -1] == 0xFFFFFFFF).any() == (nq == 70)      # k beyond the rows query 7 reaches
    _within_the_error_bound(got, queries, centroids, books, codes, ids)


@pytest.mark.parametrize("m,dsub", SHAPES)
def test_cancellation_is_clamped_to_zero(m, dsub):
    """Queries that are reconstructions of stored rows: the true distance to that row is 0 and the sum of the three
    terms falls on either side of it."""
    centroids, books, codes, ids = _index(m, dsub, 256)
    pos = numpy.random.RandomState(0).choice(L, 64, replace=False)
    cluster = numpy.searchsorted(OFFSETS, pos, "right") - 1
    queries = centroids[cluster] + books[numpy.arange(m)[None], codes[pos]].reshape(64, -1)
    probes = cluster[:, None].astype(numpy.uint32)
    terms, sums = _terms(centroids, books), []
    want = _definition(queries, centroids, books, codes, ids, OFFSETS, probes, 10, terms, sums)
    assert any((d < 0).any() for d in sums)
    got = ivfpq_search(queries, centroids, books, codes, ids, OFFSETS, probes, 10, terms=ivfpq_terms(centroids, books))
    _same(got, want)
    assert not (got[1].view(numpy.uint32) >> 31).any()


def test_device_tensors_and_an_unaligned_code_matrix():
    import torch
    m, dsub, nq, nprobe = 32, 2, 70, 3
    centroids, books, codes, ids = _index(m, dsub, 256, seed=3)
    queries = numpy.random.RandomState(4).randn(nq, m * dsub).astype(numpy.float32)
    probes = _probes(nq, nprobe)
    want = _definition(queries, centroids, books, codes, ids, OFFSETS, probes, 10, _terms(centroids, books))
    dev = torch.device("cuda", 0)
    raw = torch.zeros(4 + L * m, dtype=torch.uint8, device=dev)      # no code row is 16-byte aligned
    raw[4:] = torch.from_numpy(codes).to(dev).reshape(-1)
    ops = [torch.from_numpy(a).to(dev) for a in (queries, centroids, books)]
    ints = [torch.from_numpy(a.view(numpy.int32)).to(dev) for a in (ids, OFFSETS, probes)]
    terms = ivfpq_terms(ops[1], ops[2])
    assert terms.is_cuda and terms.dtype == torch.float32 and tuple(terms.shape) == (K, m, 256)
    t_idx, t_dist = ivfpq_search(*ops, raw[4:].view(L, m), *ints, 10, terms=terms)
    assert t_idx.is_cuda and t_idx.dtype == torch.int32 and t_dist.dtype == torch.float32
    _same((t_idx.cpu().numpy().view(numpy.uint32), t_dist.cpu().numpy()), want)


def test_index_end_to_end_and_refined():
    rs = numpy.random.RandomState(7)
    centres = (4 * rs.randn(K, 16)).astype(numpy.float32)
    rows = (centres[rs.randint(0, K, 2000)] + rs.randn(2000, 16)).astype(numpy.float32)
    books = ivfpq_train(rows, centres, 4, ksub=16, seed=1, max_iter=10)
    index = IvfPqIndex(rows, centres, books, precomputed=True, keep_rows=True)
    assert index.terms.tobytes() == _terms(centres, books).tobytes()
    queries = rows[::100].copy()
    queries[-1, 0] = numpy.nan                       # no cluster: kmeans_predict_top fills its probes with K
    probes = kmeans_predict_top(queries, centres, 2, return_distances=False)
    for k in (10, 40):
        want = _definition(queries, centres, books, index.codes, index.ids, index.offsets, probes, k, index.terms)
        _same(index.search(queries, k, nprobe=2), want)
        assert (want[0][-1] == 0xFFFFFFFF).all() and numpy.isnan(want[1][-1]).all()
    _same(index.search(queries, 10, nprobe=2, refine=4), knn_rerank(queries, rows, want[0], 10))
