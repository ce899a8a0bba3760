"""knn_rerank against the CPU oracle: oracle.distance per valid (query, candidate) pair, the keys
bits(d) << 32 | id sorted in numpy.  Indices equal, distance bits equal, NaN on the padding."""
import functools

import numpy
import pytest

import oracle
from kmcuda_amd import IvfPqIndex, ivfpq_train, knn_rerank

pytestmark = pytest.mark.gpu

N, QMAX, DMAX = 200, 80, 260
_RS = numpy.random.RandomState(0)
ROWS = _RS.randn(N, DMAX).astype(numpy.float32)
ROWS[[10, 11, 150]] = ROWS[[3, 3, 149]]          # duplicated rows: the id decides
ROWS[50] = numpy.nan                             # behind +inf
QUERIES = _RS.randn(QMAX, DMAX).astype(numpy.float32)
QUERIES[2] = ROWS[3]                             # distance +0 to rows 3, 10 and 11


@functools.lru_cache(None)
def _distances(d):
    """QMAX x N: oracle.distance of every query to every row over the first d features."""
    return numpy.array([[oracle.distance(q[:d], x[:d]) for x in ROWS] for q in QUERIES], numpy.float32)


def _candidates(nq, r, seed=1):
    """Repeated ids (a copied column), ids >= N, 0xFFFFFFFF; query 0 has no valid candidate, query 1 at most two."""
    rs = numpy.random.RandomState(seed)
    cand = rs.randint(0, N, (nq, r)).astype(numpy.uint32)
    cand[:, r // 2] = cand[:, 0]
    junk = rs.rand(nq, r)
    cand[junk < 0.05] = 0xFFFFFFFF
    cand[(junk >= 0.05) & (junk < 0.1)] = N + rs.randint(0, 3)
    cand[0] = numpy.where(numpy.arange(r) % 2, numpy.uint32(N), numpy.uint32(0xFFFFFFFF))
    if nq > 1:
        cand[1, 2:] = 0xFFFFFFFF
    return cand


def _definition(dist, cand, k):
    idx = numpy.full((len(cand), k), 0xFFFFFFFF, numpy.uint32)
    out = numpy.full((len(cand), k), numpy.nan, numpy.float32)
    for q, ids in enumerate(cand):
        ids = ids[ids < N].astype(numpy.uint64)
        d = dist[q, ids.astype(numpy.int64)]
        bits = d.view(numpy.uint32).astype(numpy.uint64)
        bits[numpy.isnan(d)] = 0x7FC00000
        bits[d == 0] = 0
        best = numpy.sort(bits << numpy.uint64(32) | ids)[:k]
        idx[q, :len(best)] = best & numpy.uint64(0xFFFFFFFF)
        out[q, :len(best)] = (best >> numpy.uint64(32)).astype(numpy.uint32).view(numpy.float32)
    return idx, out


def _same(got, want):
    (idx, dist), (w_idx, w_dist) = got, want
    assert idx.dtype == numpy.uint32 and dist.dtype == numpy.float32 and idx.shape == dist.shape == w_idx.shape
    assert (idx == w_idx).all()
    nan = numpy.isnan(w_dist)
    assert (numpy.isnan(dist) == nan).all() and (dist.view(numpy.uint32)[~nan] == w_dist.view(numpy.uint32)[~nan]).all()


@pytest.mark.parametrize("r", [1, 7, 129, 256, 257, 1024])     # queries per block step 256, 36, 1, 1; 2 and 4 passes
@pytest.mark.parametrize("d", [1, 4, 36, 256, 260])             # the fallback; 1, 2, 8, 9 chunks, partial last ones
@pytest.mark.parametrize("k_full", [False, True])
def test_matches_the_oracle(d, r, k_full):
    nq = min(2 * max(256 // r, 1) + 1, QMAX)     # the last block step is partial
    k = min(r, 256) if k_full else 1
    cand = _candidates(nq, r)
    want = _definition(_distances(d), cand, k)
    got = knn_rerank(numpy.ascontiguousarray(QUERIES[:nq, :d]), numpy.ascontiguousarray(ROWS[:, :d]), cand, k)
    _same(got, want)
    assert (want[0][0] == 0xFFFFFFFF).all() and numpy.isnan(got[1][0]).all()


def test_device_tensors_and_misaligned_rows():
    """Torch operands; the row matrix starts 4 bytes into its buffer, so no row is 16-byte aligned."""
    import torch
    d, r, k, nq = 36, 40, 10, 13
    q, x, cand = numpy.ascontiguousarray(QUERIES[:nq, :d]), numpy.ascontiguousarray(ROWS[:, :d]), _candidates(nq, r)
    want = knn_rerank(q, x, cand, k)
    _same(want, _definition(_distances(d), cand, k))
    dev = torch.device("cuda", 0)
    raw = torch.zeros(1 + N * d, dtype=torch.float32, device=dev)
    raw[1:] = torch.from_numpy(x).to(dev).reshape(-1)
    assert raw[1:].data_ptr() % 16 == 4
    for ints in (cand.view(numpy.int32), cand.astype(numpy.int64)):
        t_idx, t_dist = knn_rerank(torch.from_numpy(q).to(dev), raw[1:].view(N, d), torch.from_numpy(ints).to(dev), k)
        assert t_idx.is_cuda and t_idx.dtype == torch.int32 and t_dist.dtype == torch.float32
        _same((t_idx.cpu().numpy().view(numpy.uint32), t_dist.cpu().numpy()), want)


def test_every_id_once_is_brute_force():
    nq, d, k = 5, 256, 10
    dist = _distances(d)[:nq]
    cand = numpy.stack([numpy.random.RandomState(q).permutation(N) for q in range(nq)]).astype(numpy.uint32)
    idx, got = knn_rerank(numpy.ascontiguousarray(QUERIES[:nq, :d]), numpy.ascontiguousarray(ROWS[:, :d]), cand, k)
    order = numpy.argsort(numpy.where(numpy.isnan(dist), numpy.inf, dist), axis=1, kind="stable")[:, :k]
    assert (idx == order).all()
    assert got.tobytes() == numpy.take_along_axis(dist, order, 1).tobytes()
    assert list(idx[2, :3]) == [3, 10, 11] and (got[2, :3] == 0).all()


def test_index_search_refine():
    rs = numpy.random.RandomState(7)
    centres = (4 * rs.randn(5, 16)).astype(numpy.float32)
    rows = (centres[rs.randint(0, 5, 2000)] + rs.randn(2000, 16)).astype(numpy.float32)
    books = ivfpq_train(rows, centres, 4, ksub=16, seed=1, max_iter=10)
    index = IvfPqIndex(rows, centres, books, keep_rows=True)
    queries = rows[::100] + numpy.float32(0.1)
    _same(index.search(queries, 10, nprobe=2, refine=None), index.search(queries, 10, nprobe=2))
    got = index.search(queries, 10, nprobe=2, refine=4)
    _same(got, knn_rerank(queries, rows, index.search(queries, 40, nprobe=2)[0], 10))
    assert (got[1] == [[oracle.distance(q, rows[i]) for i in ids] for q, ids in zip(queries, got[0])]).all()
    with pytest.raises(ValueError):
        IvfPqIndex(rows, centres, books).search(queries, 10, nprobe=2, refine=4)
