"""CPU model of the radius search's cluster prune tests (knn_radius.hip, knn_index.cpp: KnnIndex::radius).

The result of a radius search is the brute-force set, so a prune test may only drop a cluster none of whose members is
a hit.  The two tests are restated here in numpy float32 with the constants of the host code, on the oracle's own
centroid distances C, member distances and radii R, and held against the oracle's hits:

  lb        (L2, up to 1024 features) lb[c][q] = (d * sd - R[c] * 1.00003) * 0.99997 > r, d = the fp32 sum-of-squares
            distance of the query to centroid c in any summation order: the model takes the largest value the
            (D + 3) u bound on that sum allows, which prunes most.
  triangle  (angular; L2 wider than 1024) C[c][c_q] - d(q, c_q) - R[c] - margin > r with
            margin = 1.01 * 4 * sqrt(2 dp), dp = (1e-6, or 1e-3 for half rows) + 1e-8 D     (angular, radians)
            margin = (1e-5 + 4e-9 D) * (C + d + R)                                          (L2)

No oracle hit may lie in a cluster its query prunes, at radii from 0 to above every distance, for the queries' computed
clusters and for deliberately wrong ones."""

import numpy
import pytest

import oracle
from _radius_inputs import truth

F = numpy.float32
U = 2.0 ** -24


def corpus_tables(x, c, a, metric):
    """The oracle's C (K x K) and R (K), as knn_cuda's preparation computes them."""
    x32, c32 = numpy.ascontiguousarray(x, F), numpy.ascontiguousarray(c, F)
    a = numpy.ascontiguousarray(a, numpy.uint32)
    n, d = x32.shape
    k = len(c32)
    L = oracle.lib()
    m = oracle._metric(metric)
    inv, offsets = numpy.empty(n, numpy.uint32), numpy.empty(k + 1, numpy.uint32)
    L.kmo_knn_inverse(n, k, oracle._up(a), oracle._up(inv), oracle._up(offsets))
    R, C = numpy.empty(k, F), numpy.empty((k, k), F)
    L.kmo_knn_radiuses(m, n, d, k, oracle._fp(x32), oracle._fp(c32), oracle._up(inv), oracle._up(offsets), oracle._fp(R))
    L.kmo_knn_cluster_distances(m, d, k, oracle._fp(c32), oracle._fp(C))
    return C, R


def lb_prunes(q, c, R, r):
    """K x Q: the lb test, with the fp32 centroid distance at the top of its rounding interval."""
    q64, c64 = q.astype(numpy.float64), c.astype(numpy.float64)
    d = q.shape[1]
    d2 = ((c64[:, None, :] - q64[None, :, :]) ** 2).sum(axis=2)
    dist = numpy.sqrt(d2 * (1.0 + (d + 3) * U)).astype(F)
    dist = numpy.nextafter(dist, F(numpy.inf))
    sd = F(min(0.99998, 1.0 - (d + 16.0) * 6.0e-8))
    with numpy.errstate(invalid="ignore"):
        lb = ((dist * sd).astype(F) - (R[:, None] * F(1.00003)).astype(F)).astype(F) * F(0.99997)
        return lb.astype(F) > F(r)


def triangle_prunes(C, R, md, qcls, r, metric, d, half):
    """K x Q: the triangle test with the host's margin, in float32 steps."""
    cd = C[:, qcls]                  # C[c][c_q]
    rr = numpy.broadcast_to(R[:, None], cd.shape)
    mdb = numpy.broadcast_to(md[None, :], cd.shape)
    if metric == "L2":
        absm, rel = F(0), F(1e-5 + 4e-9 * d)
    else:
        dp = (1.0e-3 if half else 1.0e-6) + 1.0e-8 * d
        absm, rel = F(4.0 * 1.01 * numpy.sqrt(2.0 * dp)), F(0)
    with numpy.errstate(invalid="ignore"):
        margin = (absm + (rel * ((cd + mdb).astype(F) + rr).astype(F)).astype(F)).astype(F)
        lim = (((cd - mdb).astype(F) - rr).astype(F) - margin).astype(F)
        return lim > F(r)


def query_clusters(q, c, metric, kind):
    finite = numpy.nonzero(numpy.isfinite(c).all(axis=1))[0]
    if kind == "computed":
        return oracle.lloyd_assign(numpy.ascontiguousarray(q, F), numpy.ascontiguousarray(c, F), metric=metric)[0].astype(numpy.int64)
    if kind == "one":
        return numpy.full(len(q), finite[0], numpy.int64)
    return finite[numpy.random.default_rng(6).integers(0, len(finite), len(q))].astype(numpy.int64)


def radii_of(dm):
    v = dm[~numpy.isnan(dm)]
    qs = numpy.quantile(v.astype(numpy.float64), [0.0005, 0.005, 0.02, 0.1, 0.5, 0.9]).astype(F)
    return [F(0)] + list(qs) + [numpy.nextafter(v.max(), F(numpy.inf)), F(2) * v.max()]


def assert_no_hit_pruned(prunes, dm, a, r, what):
    qi, idx = numpy.nonzero(dm <= F(r))
    bad = prunes[numpy.asarray(a).astype(numpy.int64)[idx], qi]
    assert not bad.any(), "%s r=%r: %d hits lie in pruned clusters (first: query %d row %d)" % (
        what, float(r), int(bad.sum()), int(qi[bad][0]), int(idx[bad][0]))


@pytest.mark.parametrize("d", [64, 256, 512, 1152])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_no_hit_in_a_pruned_cluster(metric, half, d):
    x, c, a, q, dm = truth(2000, d, metric, half)
    x32, c32, q32 = x.astype(F), c.astype(F), q.astype(F)
    C, R = corpus_tables(x32, c32, a, metric)
    pruned_some = False
    for kind in ("computed", "one", "random"):
        qcls = query_clusters(q32, c32, metric, kind)
        md = numpy.array([oracle.distance(q32[i], c32[qcls[i]], metric) for i in range(len(q32))], F)
        for r in radii_of(dm):
            tri = triangle_prunes(C, R, md, qcls, r, metric, d, half)
            assert_no_hit_pruned(tri, dm, a, r, "triangle %s %s D=%d half=%s" % (kind, metric, d, half))
            pruned_some |= bool(tri.any())
            if metric == "L2" and d <= 1024 and kind == "computed":   # (lb does not depend on the query's cluster)
                lbp = lb_prunes(q32, c32, R, r)
                assert_no_hit_pruned(lbp, dm, a, r, "lb D=%d half=%s" % (d, half))
                pruned_some |= bool(lbp.any())
    assert pruned_some, "the model never pruned anything: it checks nothing"


def test_the_host_code_has_these_constants():
    """The constants restated above are the ones KnnIndex::radius and knn_centroid_bounds_kernel compile."""
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kmcuda_amd", "csrc")
    with open(os.path.join(csrc, "knn_index.cpp")) as f:
        host = f.read()
    for text in ("prune_rel = (float)(1e-5 + 4e-9 * (double)D);", "(fp16 ? 1.0e-3 : 1.0e-6) + 1.0e-8 * (double)D;",
                 "prune_abs = (float)(4.0 * 1.01 * sqrt(2.0 * dp));", "prune_abs = INFINITY;"):
        assert text in host, text
    with open(os.path.join(csrc, "knn.hip")) as f:
        bounds = f.read()
    for text in ("fminf(0.99998f, 1.0f - ((float)D + 16.0f) * 6.0e-8f)", "(d * sd - R[c] * 1.00003f) * 0.99997f"):
        assert text in bounds, text


def test_margins_cover_their_terms():
    """The angular margin covers four angles whose cosines are each off by dp (|acos a - acos b| <= sqrt(2 |a - b|)
    at the worst place, a = 1), and the L2 margin the chunked fp32 sums of C and R ((D / 16) u relative on a squared
    distance, half of it on the distance)."""
    for d in (16, 64, 1152, 1 << 16):
        for half in (False, True):
            dp = (1.0e-3 if half else 1.0e-6) + 1.0e-8 * d
            worst = float(numpy.arccos(1.0 - dp))          # the largest angle error a product error dp can cause
            assert 4.0 * 1.01 * numpy.sqrt(2.0 * dp) >= 4.0 * worst
            # dp itself: row norms within 3 x 2^-24 (2^-11 for halves rounded from unit rows) of 1 on either side of a
            # product, plus the chunked sums of the product ((D / 16 + 2) u)
            norm = 2.0 ** -11 if half else 3 * 2.0 ** -24
            assert dp >= (1.0 + norm) ** 2 - 1.0 + (d / 16.0 + 2.0) * U
        # each of the three terms is off by at most that relative error: their sum times it covers all three
        assert 1e-5 + 4e-9 * d >= 0.5 * (d / 16.0 + 3.0) * U + 4 * U
