"""oracle.knn_query (kmo_knn_query, oracle/kmcuda_oracle.c): the executable form of DESIGN.md 4.8 point 2, checked
WITHOUT relying on its cluster prune being right.

On tie-free data (asserted here) the list of a query is fixed by the distances alone: the stable argsort of
oracle.distance(q, x_j) over the corpus rows that have a cluster, and the returned distances are those values bit for
bit.  A prune that dropped a cluster it should visit, a heap that lost an entry or a visiting order that mattered
would all show.  Then: corpus rows as queries give oracle.knn's lists behind themselves; any legal cluster id gives
the same answer; non-finite queries, rows without a cluster, filler slots and a NaN centroid behave as 4.8 states."""
import ctypes

import numpy
import pytest

import oracle

NONE = 0xFFFFFFFF
FLT_MAX = numpy.finfo(numpy.float32).max


def _unit(x):
    return (x / numpy.linalg.norm(x, axis=1, keepdims=True)).astype(numpy.float32)


def _data(metric, n=400, q=90, d=8, K=12, seed=0):
    """Blob rows, centroids = K of the rows, the oracle's nearest-centroid assignments; candidate queries: fresh blob
    draws and a few far rows."""
    rs = numpy.random.RandomState(seed)
    centres = rs.randn(K, d) * 3
    x = (centres[rs.randint(0, K, n)] + rs.randn(n, d)).astype(numpy.float32)
    qs = numpy.concatenate([centres[rs.randint(0, K, q - 8)] + rs.randn(q - 8, d), rs.randn(8, d) * 40]).astype(numpy.float32)
    if metric != "L2":
        x, qs = _unit(x), _unit(qs)
    c = x[rs.choice(n, K, replace=False)].copy()
    a, _, _ = oracle.lloyd_assign(x, c, metric=metric)
    assert (a < K).all()
    return x, c, a, qs


def _all_distances(qs, x, metric):
    return numpy.array([[oracle.distance(q, row, metric=metric) for row in x] for q in qs], numpy.float32)


_TIE_FREE = {}


def tie_free(metric):
    if metric not in _TIE_FREE:
        x, c, a, qs = _data(metric)
        d = _all_distances(qs, x, metric)
        # 400 float32 distances collide now and then (and acosf is libm's): of 90 drawn queries keep the first 60
        # that have no two corpus rows at the same distance, far rows included
        free = numpy.array([numpy.unique(row).size == row.size for row in d])
        sel = numpy.concatenate([numpy.nonzero(free[:-8])[0][:52], len(qs) - 8 + numpy.nonzero(free[-8:])[0]])
        qs, d = qs[sel], d[sel]
        assert 56 <= len(qs) <= 60
        for i in range(len(qs)):   # tie-free
            assert numpy.unique(d[i]).size == d.shape[1], (metric, i)
        _TIE_FREE[metric] = (x, c, a, qs, d)
    return _TIE_FREE[metric]


def _bits(v):
    return numpy.ascontiguousarray(v, dtype=numpy.float32).view(numpy.uint32)


@pytest.mark.parametrize("metric", ["L2", "angular"])
@pytest.mark.parametrize("k", [1, 7, 400])
def test_tie_free_lists_are_the_sorted_distances(metric, k):
    x, c, a, qs, d = tie_free(metric)
    nb, dist = oracle.knn_query(k, x, c, a, qs, metric=metric)
    want = numpy.argsort(d, axis=1, kind="stable")[:, :k]
    assert nb.dtype == numpy.uint32 and dist.dtype == numpy.float32 and nb.shape == dist.shape == (len(qs), k)
    assert (nb == want).all()
    assert (_bits(dist) == _bits(numpy.take_along_axis(d, want, axis=1))).all()


@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_rows_without_a_cluster_are_no_candidates(metric):
    """Finite rows whose assignment is K or 0xFFFFFFFF: never returned; at k = N the tail is index 0 at FLT_MAX."""
    x, c, a, qs, d = tie_free(metric)
    a = a.copy()
    out = numpy.array([0, 17, 18, 250, 399])   # row 0 among them: a filler index 0 is then no corpus answer
    a[out] = [NONE, len(c), NONE, len(c) + 5, len(c)]
    keep = numpy.setdiff1d(numpy.arange(len(x)), out)
    order = keep[numpy.argsort(d[:, keep], axis=1, kind="stable")]
    for k in (7, len(x)):
        nb, dist = oracle.knn_query(k, x, c, a, qs, metric=metric)
        m = min(k, len(keep))
        assert (nb[:, :m] == order[:, :m]).all()
        assert (_bits(dist[:, :m]) == _bits(numpy.take_along_axis(d, order[:, :m], axis=1))).all()
        assert (nb[:, m:] == 0).all() and (dist[:, m:] == FLT_MAX).all()
    assert k - m == 5


@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_corpus_rows_as_queries(metric):
    """Own clusters, k + 1: column 0 is the row itself, columns 1..k are oracle.knn(k) (tie-free data)."""
    x, c, a, _, _ = tie_free(metric)
    for k in (1, 6, 40):
        ref, _ = oracle.knn(k, x, c, a, metric=metric)
        nb, dist = oracle.knn_query(k + 1, x, c, a, x, query_assignments=a, metric=metric)
        assert (nb[:, 0] == numpy.arange(len(x))).all()
        assert (nb[:, 1:] == ref).all()
        assert (numpy.diff(dist, axis=1) > 0).all()
        if metric == "L2":
            assert (dist[:, 0] == 0).all()


@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_any_cluster_id_gives_the_same_answer(metric):
    x, c, a, qs, _ = tie_free(metric)
    K = len(c)
    base = oracle.knn_query(9, x, c, a, qs, metric=metric)
    own, _, _ = oracle.lloyd_assign(qs, c, metric=metric)
    same = oracle.knn_query(9, x, c, a, qs, query_assignments=own, metric=metric)
    assert (same[0] == base[0]).all() and (_bits(same[1]) == _bits(base[1])).all()
    rs = numpy.random.RandomState(3)
    for qa in [rs.randint(0, K, len(qs)), numpy.zeros(len(qs), int), numpy.full(len(qs), K - 1),
               (own + 1) % K]:
        nb, dist = oracle.knn_query(9, x, c, a, qs, query_assignments=qa.astype(numpy.uint32), metric=metric)
        assert (nb == base[0]).all() and (_bits(dist) == _bits(base[1])).all()


def test_non_finite_queries_and_ids_beyond_k():
    x, c, a, qs, d = tie_free("L2")
    qs = qs[:12].copy()
    qs[1, 0] = numpy.nan
    qs[3, 5] = numpy.nan          # (not feature 0: lloyd_assign does not call this row insane)
    qs[5, 2] = numpy.inf
    qs[7, 7] = -numpy.inf
    bad = numpy.array([1, 3, 5, 7])
    good = numpy.setdiff1d(numpy.arange(12), bad)
    want = numpy.argsort(d[:12], axis=1, kind="stable")[:, :5]
    for qa in (None, numpy.zeros(12, numpy.uint32)):
        nb, dist = oracle.knn_query(5, x, c, a, qs, query_assignments=qa)
        assert (nb[bad] == NONE).all() and numpy.isnan(dist[bad]).all()
        assert (nb[good] == want[good]).all()
    qa = numpy.zeros(12, numpy.uint32)
    qa[[2, 4]] = [len(c), NONE]
    nb, dist = oracle.knn_query(5, x, c, a, qs, query_assignments=qa)
    none = numpy.array([1, 2, 3, 4, 5, 7])
    assert (nb[none] == NONE).all() and numpy.isnan(dist[none]).all()
    rest = numpy.setdiff1d(numpy.arange(12), none)
    assert (nb[rest] == want[rest]).all()


def test_nan_centroid_cluster_is_skipped_by_the_others():
    """C[c][c_q] is NaN for a cluster c whose centroid is NaN: queries of other clusters never see its members
    (knn.cu:219-221); a query placed IN that cluster sees only them (every other centroid distance is NaN too)."""
    x, c, a, qs, d = tie_free("L2")
    c = c.copy()
    c[3, 1] = numpy.nan
    members = numpy.nonzero(a == 3)[0]
    others = numpy.nonzero(a != 3)[0]
    assert members.size > 2
    q = numpy.concatenate([qs[:20], x[members[:2]]])        # two queries ARE members of that cluster
    dq = numpy.concatenate([d[:20], _all_distances(x[members[:2]], x, "L2")])
    qa = (1 + numpy.arange(len(q)) % 2).astype(numpy.uint32)  # clusters 1 and 2
    k = len(x)
    nb, dist = oracle.knn_query(k, x, c, a, q, query_assignments=qa)
    order = others[numpy.argsort(dq[:, others], axis=1, kind="stable")]
    assert (nb[:, :others.size] == order).all()
    assert (nb[:, others.size:] == 0).all() and (dist[:, others.size:] == FLT_MAX).all()
    nb3, dist3 = oracle.knn_query(k, x, c, a, q, query_assignments=numpy.full(len(q), 3, numpy.uint32))
    inside = members[numpy.argsort(dq[:, members], axis=1, kind="stable")]
    assert (nb3[:, :members.size] == inside).all() and (nb3[:, members.size:] == 0).all()


def test_half2_distances_are_the_k_smallest():
    """half2=True: sums of halves tie often, so the check is on the distances -- each the half2 distance of its pair,
    ascending, and as a multiset the k smallest over the corpus; without a tie at a slot the index is fixed too."""
    rs = numpy.random.RandomState(5)
    x = rs.randn(300, 16).astype(numpy.float16)
    c = x[rs.choice(300, 8, replace=False)].copy()
    a, _, _ = oracle.lloyd_assign(x.astype(numpy.float32), c.astype(numpy.float32))
    q = numpy.concatenate([rs.randn(30, 16), x[:10].astype(numpy.float64)]).astype(numpy.float16)
    k = 12
    nb, dist = oracle.knn_query(k, x, c, a, q, half2=True)
    L = oracle.lib()
    L.kmo_set_fp16_mode(2)
    try:
        d = _all_distances(q.astype(numpy.float32), x.astype(numpy.float32), "L2")
    finally:
        L.kmo_set_fp16_mode(0)
    plain = oracle.knn_query(k, x, c, a, q)[1]
    assert (dist != plain).any()                 # the half2 arithmetic is in effect
    assert (_bits(dist) == _bits(numpy.take_along_axis(d, nb.astype(numpy.int64), axis=1))).all()
    assert (_bits(dist) == _bits(numpy.sort(d, axis=1)[:, :k])).all()
    for i in range(len(q)):
        assert len(set(nb[i].tolist())) == k
    with pytest.raises(ValueError):
        oracle.knn_query(k, x.astype(numpy.float32), c, a, q, half2=True)


def test_arguments():
    x, c, a, qs, _ = tie_free("L2")
    with pytest.raises(ValueError):
        oracle.knn_query(3, x, c, a, qs[:, :5])
    with pytest.raises(ValueError):
        oracle.knn_query(3, x, c, a, qs, query_assignments=numpy.zeros(3, numpy.uint32))
    with pytest.raises(ValueError):
        oracle.knn_query(0, x, c, a, qs)
    assert isinstance(oracle.lib().kmo_knn_query, ctypes._CFuncPtr)
