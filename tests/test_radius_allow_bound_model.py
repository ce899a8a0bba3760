"""CPU model of the MASKED radius search's cluster prune: the lb and triangle tests of
tests/test_radius_bound_model.py with R replaced by the radii over the allowed rows -- the radii of the index the masked
call is defined by, corpus_tables(x, c, patched(a, mask, K), metric).

Both tests are lower bounds of the distance to every member that MAY BE RETURNED, so a smaller R prunes more and must
still drop no allowed hit.  Two masks: a random half, and an "inner" mask -- the rows at or below their cluster's median
member distance -- which shrinks every radius and so must prune strictly more (cluster, query) pairs than the unmasked
radii: otherwise the test would check nothing the unmasked model does not.

Pruned (cluster, query) pairs summed over radii_of(dm), the queries' computed clusters, lb where it applies (L2 up to
1024 features) and the triangle test elsewhere, as first measured:

    case             unmasked   random mask   inner mask
    L2 D = 64           17106         17111        17817
    angular D = 64      13944         13990        14090
    L2 D = 1152          9611          9632         9908

with no allowed hit in a pruned cluster in any of the six masked cases."""

import numpy
import pytest

import oracle
from _radius_inputs import truth
from test_radius_bound_model import (F, assert_no_hit_pruned, corpus_tables, lb_prunes, query_clusters, radii_of,
                                     triangle_prunes)

_MASKS = {}


def patched(a, mask, K):
    """test_gpu_knn_allow.patched (restated: that module needs torch): the denied rows lose their cluster."""
    return numpy.where(numpy.asarray(mask) != 0, a, K).astype(numpy.uint32)


def masks(d, metric):
    """name -> mask for truth(2000, d, metric): computed once."""
    if (d, metric) not in _MASKS:
        x, c, a, _, _ = truth(2000, d, metric, False)
        K = len(c)
        x32, c32, a = x.astype(F), c.astype(F), numpy.asarray(a)
        member = numpy.full(len(x), numpy.nan, F)
        for i in numpy.nonzero(a < K)[0]:
            member[i] = oracle.distance(x32[i], c32[a[i]], metric)
        inner = numpy.zeros(len(x), bool)
        for k in range(K):
            rows = a == k
            if rows.any():
                inner[rows] = member[rows] <= numpy.nanmedian(member[rows])
        _MASKS[(d, metric)] = {"random": numpy.random.RandomState(0).rand(len(x)) < 0.5, "inner": inner}
    return _MASKS[(d, metric)]


@pytest.mark.parametrize("name", ["random", "inner"])
@pytest.mark.parametrize("metric,d", [("L2", 64), ("angular", 64), ("L2", 1152)])
def test_no_allowed_hit_in_a_pruned_cluster(metric, d, name):
    x, c, a, q, dm = truth(2000, d, metric, False)
    K = len(c)
    x32, c32, q32 = x.astype(F), c.astype(F), q.astype(F)
    mask = masks(d, metric)[name]
    _, R = corpus_tables(x32, c32, a, metric)
    C, Rm = corpus_tables(x32, c32, patched(a, mask, K), metric)
    with numpy.errstate(invalid="ignore"):
        assert not (Rm > R).any()                      # (a NaN: a cluster without an allowed row)
    allowed = dm.copy()
    allowed[:, ~mask] = numpy.nan                      # the masked call's truth: the denied columns struck out
    use_lb = metric == "L2" and d <= 1024
    total = total_masked = 0
    for kind in ("computed", "one", "random"):
        qcls = query_clusters(q32, c32, metric, kind)
        md = numpy.array([oracle.distance(q32[i], c32[qcls[i]], metric) for i in range(len(q32))], F)
        for r in radii_of(dm):
            tri = triangle_prunes(C, Rm, md, qcls, r, metric, d, False)
            assert_no_hit_pruned(tri, allowed, a, r, "triangle %s %s D=%d %s mask" % (kind, metric, d, name))
            if kind != "computed":
                continue
            plain = triangle_prunes(C, R, md, qcls, r, metric, d, False)
            if use_lb:                                 # (lb does not depend on the query's cluster)
                tri, plain = lb_prunes(q32, c32, Rm, r), lb_prunes(q32, c32, R, r)
                assert_no_hit_pruned(tri, allowed, a, r, "lb D=%d %s mask" % (d, name))
            # the masked radii prune whatever the unmasked ones do (but where no row is allowed: Rm = NaN, no test
            # speaks and the search skips the cluster by its allowed count)
            assert not (plain & ~tri)[~numpy.isnan(Rm)].any()
            total += int(plain.sum())
            total_masked += int(tri.sum())
    print("pruned (cluster, query) pairs %s D=%d: unmasked %d, %s mask %d" % (metric, d, total, name, total_masked))
    assert total > 0, "the model never pruned anything: it checks nothing"
    if name == "inner":
        assert total_masked > total, "the inner mask prunes no more than no mask: the test checks nothing"
