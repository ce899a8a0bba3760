"""The inputs of tests/test_gpu_knn_radius_edges.py are what those tests need them to be -- checked against the oracle
alone, so that an input assertion of a GPU test does not fire first on a GPU machine.

  angular radii   at least 4 float32 ulp from every oracle distance an acos produced (acos is ocml's on the device and
                  libm's in the oracle: 2 ulp, tests/_angular.py), the largest distance of the limits' corpus below 3.1
  cluster sizes   at "every" each cluster holds a hit, at "all" every clustered row is one
  data range      a median of at least 15 hits per query and some query with none; the centred values inside the half
                  range at 6e4, beyond it at 2e5; which search the fp16x2 corpora across the half range ask for"""
import numpy
import pytest

pytest.importorskip("torch")   # (the corpora are built by the GPU test modules' helpers, which import it)

import _radius_inputs as ri   # noqa: E402


def assert_clear(cs):
    for name, r in cs.r.items():
        clear = ri.angular_clearance(cs.dm, r)
        assert clear >= 4, "radius %s = %r: an oracle distance %.2f ulp away" % (name, float(r), clear)


def assert_typical(cs, r, empty=True):
    counts = cs.counts(r)
    assert numpy.median(counts) >= 15, numpy.median(counts)
    if empty:
        assert (counts == 0).any()


@pytest.mark.parametrize("d", [8] + ri.EQUAL_D + ri.PADDED_D)
@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_instantiation_inputs(metric, d):
    cs = ri.instantiation(metric, d, False)
    assert_typical(cs, cs.r["target"], empty=metric == "L2")
    if metric != "L2":
        assert_clear(cs)


@pytest.mark.parametrize("d", ri.HALF_D)
@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_instantiation_inputs_fp16x2(metric, d):
    cs = ri.instantiation(metric, d, True)
    assert cs.x.dtype == cs.q.dtype == numpy.float16
    assert_typical(cs, cs.r["target"], empty=metric == "L2")
    if metric != "L2":
        assert_clear(cs)


@pytest.mark.parametrize("d", ri.RANGE_D)
@pytest.mark.parametrize("scale", ri.SCALES)
def test_data_range_inputs(scale, d):
    cs = ri.data_range(scale, d)
    assert_typical(cs, cs.r["target"])
    top_x, top_q = ri.centred_top(cs)
    if scale == 6e4:
        assert max(top_x, top_q) < 65504
    if scale == 2e5:
        assert top_x > 65520
    if scale == 1e-6:
        assert max(top_x, top_q) < 6.1e-5       # every centred value a half subnormal


def test_other_range_inputs():
    cs = ri.subnormal_squares()
    assert_typical(cs, cs.r["target"])
    assert float(cs.r["target"]) ** 2 < 1.2e-38
    for d in (64, 512):
        cs = ri.offset_rows(d)
        assert_typical(cs, cs.r["target"])
        assert max(ri.centred_top(cs)) < 100 and cs.x.min() > 9000
    cs = ri.uniform_beyond()
    assert_typical(cs, cs.r["target"], empty=False)
    assert ri.centred_top(cs)[0] > 65520


@pytest.mark.parametrize("d", [64, 512])
def test_outlier_query_inputs(d):
    cs = ri.one_outlier_query(d)
    assert len(cs.q) == 300 and cs.q[150, 5] == 1e6
    top_x, top_q = ri.centred_top(cs)
    assert top_x < 65504 < 65520 < top_q
    rest = numpy.delete(cs.q, 150, axis=0).astype(numpy.float32)
    assert numpy.abs(rest - cs.c.mean(axis=0)).max() < 65504      # the other chunks stay inside
    assert_typical(cs, cs.r["target"])
    assert cs.counts(cs.r["target"])[150] == 0


@pytest.mark.parametrize("d,skew,xrange,qrange,want", ri.HALF_RANGE)
def test_half_range_inputs(d, skew, xrange, qrange, want):
    cs = ri.half_across(d, skew, xrange, qrange)
    assert ri.half_range_expectation(cs) == want
    assert numpy.median(cs.counts(cs.r["target"])) >= 15


@pytest.mark.parametrize("d", ri.SIZED_D)
def test_cluster_size_inputs(d):
    cs = ri.cluster_sizes(d)
    assert numpy.bincount(cs.a).tolist() == ri.SIZES
    assert ri.hit_clusters(cs, cs.r["every"]) == len(ri.SIZES)
    below = numpy.nextafter(cs.r["every"], numpy.float32(0))
    assert ri.hit_clusters(cs, below) == len(ri.SIZES) - 1        # the radius is a pair's own distance
    assert cs.r["every"] < cs.r["all"]
    assert (cs.counts(cs.r["all"]) == sum(ri.SIZES)).all()


def test_query_block_inputs():
    for d, nq in ri.BLOCKS:
        cs = ri.query_blocks(d, nq)
        assert len(cs.q) == nq and (cs.qa == ri.SIZES.index(513)).all()
        assert numpy.median(cs.counts(cs.r["target"])) >= 15


def test_angular_limit_inputs():
    cs = ri.angular_limits()
    assert numpy.nanmax(cs.dm) < 3.1
    assert_clear(cs)
    members = int((cs.a < len(cs.c)).sum())
    assert (cs.counts(cs.r["switch"]) == members).all() and (cs.counts(cs.r["below"]) == members).all()
    for name in ("2.0", "pi/2"):
        counts = cs.counts(cs.r[name])
        assert 0 < counts.sum() < members * len(cs.q)
    assert numpy.cos(numpy.float32(2.0)) < 0 and numpy.cos(numpy.float64(cs.r["pi/2"])) <= 0


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("d", [16, 256, 768])
def test_unit_row_inputs(d, half):
    cs = ri.unit_rows(d, half)
    assert_clear(cs)
    zero = cs.counts(cs.r["0"])
    assert (zero == 0).any()
    if half or d == 16:   # (fp32 unit rows of 256 and 768 features: every product, a row's with itself too, is below 1)
        assert (zero >= 1).sum() >= 20 and (zero >= 2).any()
    assert (cs.counts(cs.r["3.2"]) == len(cs.x)).all()
    assert (cs.dm >= numpy.float32(3.1415925)).any()              # antipodes: beyond the kernel's switch constant


def test_degenerate_and_prune_inputs():
    for d in (64, 1100):
        cs = ri.degenerate_corpus(d)
        assert len(cs.inf_rows) == 1 and cs.a[cs.inf_rows[0]] < len(cs.c)
        counts = cs.counts(cs.r["target"])
        assert (counts[cs.bad] == 0).all() and numpy.median(counts) >= 15
        hits = cs.dm <= cs.r["target"]
        assert hits[:, cs.a == 6].any() and not hits[:, cs.inf_rows].any() and not hits[:, cs.a >= len(cs.c)].any()
    for cs in (ri.moved_rows(), ri.skewed(), ri.half_strict()):
        assert numpy.median(cs.counts(cs.r["target"])) >= 15


@pytest.mark.parametrize("d", [50, 64, 600])
def test_wide_radius_inputs(d):
    """At the wide radius a query has hits in several clusters and not in most: partly covered clusters exist."""
    cs = ri.instantiation("L2", d, False) if d != 64 else ri.data_range(1.0, d)
    per = ri.clusters_hit(cs, cs.r["wide"])
    assert 2 <= numpy.median(per) < len(cs.c) / 2
    assert cs.r["wide"] > 2 * cs.r["target"]
