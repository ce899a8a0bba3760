"""Radius search (kmcuda_amd.KnnIndex.query_radius; knn_radius.hip, KnnIndex::radius in knn_index.cpp) on
every kernel variant, data range and tile edge: each instantiation of knn_radius_f16_kernel (DP 16 ... 1024, rows that
fill DP and rows zero-padded to it, both metrics), data from half subnormals to beyond the half range, a chunk that
leaves the half range between chunks that do not, cluster sizes and query blocks around the tiles, angular radii at the
kernel's switch to "everything" and at cos r <= 0, a degenerate corpus, and every prune path and switch the call reads.

One helper checks every case.  The result is the brute-force set, so it is compared with the oracle's distance matrix
thresholded (tests/_radius_inputs.py): counts, offsets and neighbours equal in (cluster, row) order, L2 distances equal
as bit patterns, angular ones within 2 float32 ulp at a radius 4 ulp clear of every oracle distance.  Finite fp32 L2
inputs also pass a float64 check that the oracle and the kernels cannot both get wrong the same way.  `expect` names the
search that must have run; it is read back from what verbosity = 1 prints and from the two statistics lines of
KMCUDA_AMD_KNN_STATS, so that a guard which sends everything to the exact kernel passes nothing here; on the f16 path
the statistics also satisfy what the kernel's bookkeeping implies.

The inputs' own properties (a radius' clearance, "every cluster has a hit", the half-range conditions) are asserted
here and, on the oracle alone, in tests/test_radius_edges_inputs_cpu.py."""
import contextlib
import os
import re

import numpy
import pytest

import _radius_inputs as ri
from _radius_inputs import all_distances, expected
from test_gpu_kmeans import StdoutListener

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EXACT = "every candidate is evaluated with the exact arithmetic"
INDEX_HALF_RANGE = "k-NN index: a centred row leaves the half range"
QUERY_HALF_RANGE = "k-NN query: a centred query leaves the half range"
EXPECT = ("f16", "exact", "index_half_range", "query_half_range")
SWITCHES = ("KMCUDA_AMD_FILTER", "KMCUDA_AMD_KNN_EXACT", "KMCUDA_AMD_FP16_STRICT", "KMCUDA_AMD_KNN_QUERY_CHUNK",
            "KMCUDA_AMD_KNN_ORDER", "KMCUDA_AMD_KNN_TIGHT", "KMCUDA_AMD_KNN_STATS")
STATS = re.compile(r"k-NN index radius (count|fill): (\d+) pairs in visited clusters, (\d+) scored on the matrix cores "
                   r"\((\d+) of them live query x real candidate; (\d+) by operand sets with a visiting query\), "
                   r"(\d+) exact chains")


@contextlib.contextmanager
def environment(env):
    """The switches a radius call reads: only those of `env`, and the statistics."""
    saved = {name: os.environ.get(name) for name in SWITCHES}
    try:
        for name in SWITCHES:
            os.environ.pop(name, None)
        os.environ["KMCUDA_AMD_KNN_STATS"] = "1"
        for name, value in (env or {}).items():
            os.environ[name] = str(value)
        yield
    finally:
        for name, value in saved.items():
            os.environ.pop(name, None)
            if value is not None:
                os.environ[name] = value


def run_radius(x, c, a, q, r, metric, qa, ptr):
    """(counts, (offsets, neighbors, distances), printed text) of one index: a counting call, then a full one."""
    from kmcuda_amd import KnnIndex
    out = StdoutListener()
    with out:
        if ptr == "host":
            with KnnIndex(x, c, a, metric=metric, verbosity=1) as ix:
                counts = ix.query_radius(q, r, query_assignments=qa, count_only=True)
                got = ix.query_radius(q, r, query_assignments=qa)
        else:
            dev = torch.device("cuda", 0)
            tx, tc, tq = (torch.from_numpy(numpy.array(v)).to(dev) for v in (x, c, q))
            ta = torch.from_numpy(numpy.array(a).view(numpy.int32)).to(dev)
            tqa = None if qa is None else torch.from_numpy(numpy.array(qa).view(numpy.int32)).to(dev)
            with KnnIndex(tx, tc, ta, metric=metric, verbosity=1) as ix:
                tcounts = ix.query_radius(tq, r, query_assignments=tqa, count_only=True)
                tgot = ix.query_radius(tq, r, query_assignments=tqa)
            assert tcounts.is_cuda and all(t.is_cuda for t in tgot)
            assert tcounts.dtype == torch.int32 and tgot[0].dtype == torch.int64 and tgot[1].dtype == torch.int32
            counts = tcounts.cpu().numpy().view(numpy.uint32)
            got = (tgot[0].cpu().numpy(), tgot[1].cpu().numpy().view(numpy.uint32), tgot[2].cpu().numpy())
    return counts, got, out.text


def f64_distances(x, a, K, q):
    """Q x N float64 L2 distances, NaN at the rows without a cluster.  Centred rows, |x|^2 + |q|^2 - 2 x.q in float64:
    the error of a squared distance is below (D + 8) 2^-52 (|x|^2 + |q|^2), returned per query as `err` (Q)."""
    x64, q64 = x.astype(numpy.float64), q.astype(numpy.float64)
    member = a < K
    mu = x64[member].mean(axis=0)
    x64, q64 = x64 - mu, q64 - mu
    xn, qn = (x64 ** 2).sum(axis=1), (q64 ** 2).sum(axis=1)
    d2 = xn[None, :] + qn[:, None] - 2.0 * (q64 @ x64.T)
    err = (x.shape[1] + 8) * 2.0 ** -52 * (xn[member].max() + qn)
    out = numpy.sqrt(numpy.maximum(d2, 0.0))
    out[:, ~member] = numpy.nan
    return out, err, x64, q64


def f64_check(x, a, K, q, r, offsets, nb, what):
    """Every returned pair has float64 distance <= r (1 + 1e-5); every clustered pair with float64 distance
    <= r (1 - 1e-5) is returned (1e-5: the relative bar of the k-NN tests' _f64_check helpers)."""
    d64, err, x64, q64 = f64_distances(x, a, K, q)
    # where the expansion's error is not far below the bar (a query with a huge feature): the differences themselves
    for i in numpy.nonzero(err > 1e-7 * float(r) ** 2)[0]:
        d64[i, a < K] = numpy.sqrt(((x64[a < K] - q64[i]) ** 2).sum(axis=1))
    returned = numpy.zeros(d64.shape, bool)
    qi = numpy.repeat(numpy.arange(len(q)), numpy.diff(offsets))
    returned[qi, nb.astype(numpy.int64)] = True
    r64 = float(numpy.float32(r))
    with numpy.errstate(invalid="ignore"):
        far = returned & ~(d64 <= r64 * (1 + 1e-5))
        missed = ~returned & (d64 <= r64 * (1 - 1e-5))
    assert not far.any(), "%s: %d returned pairs are beyond r in float64, first %s" % (
        what, far.sum(), numpy.argwhere(far)[0])
    assert not missed.any(), "%s: %d pairs within r in float64 are missing, first %s" % (
        what, missed.sum(), numpy.argwhere(missed)[0])


def index_has_no_filter(d, fp16, env):
    """knn_choose_path: the index prints the EXACT line when no matrix-core filter exists for it."""
    env = env or {}
    return bool(int(env.get("KMCUDA_AMD_KNN_EXACT", 0))) or (fp16 and bool(int(env.get("KMCUDA_AMD_FP16_STRICT", 0)))) or \
        d > 1024 or (d > 256 and env.get("KMCUDA_AMD_FILTER") == "f32")


def check_radius(x, c, a, q, r, metric="L2", qa=None, env=None, expect=None, half2=False, ptr="host", dm=None):
    """KnnIndex(x, c, a).query_radius(q, r) == the oracle's brute-force set: see the module's docstring.  `expect` in
    EXPECT: the search that must have run.  half2: KMCUDA_AMD_FP16_STRICT, the oracle in the reference's half2
    arithmetic.  dm: all_distances(x, c, a, q, metric, half2), if the caller holds it.  Returns (counts, (offsets,
    neighbors, distances), statistics, text); statistics: a dict of the numbers of the `k-NN index radius` lines."""
    a = numpy.ascontiguousarray(a, dtype=numpy.uint32)
    q = numpy.ascontiguousarray(q)
    qa = None if qa is None else numpy.ascontiguousarray(qa, dtype=numpy.uint32)
    assert x.dtype == c.dtype == q.dtype
    r = numpy.float32(r)
    K, d = len(c), x.shape[1]
    env = dict(env or {})
    if half2:
        env["KMCUDA_AMD_FP16_STRICT"] = 1
    what = "%s %s D=%d r=%r %s %s" % (metric, x.dtype, d, float(r), ptr, env)
    # ---- the truth, and what the radius must be for the comparison to be sound ----
    if dm is None:
        dm = all_distances(x, c, a, q, metric, half2)
    if metric != "L2":
        clear = ri.angular_clearance(dm, r)
        assert clear >= 4, "%s: an oracle distance %.2f ulp from the radius" % (what, clear)
    exp = expected(dm, a, r)
    ecounts, eoffsets, enb, edist = exp
    # ---- run ----
    with environment(env):
        counts, got, text = run_radius(x, c, a, q, r, metric, qa, ptr)
    offsets, nb, dist = got
    # ---- the oracle's brute-force set ----
    assert counts.dtype == numpy.uint32 and offsets.dtype == numpy.int64
    assert nb.dtype == numpy.uint32 and dist.dtype == numpy.float32
    bad = numpy.nonzero(counts != ecounts)[0]
    assert bad.size == 0, "%s: %d counts differ from the oracle's, first query %d: %d vs %d" % (
        what, bad.size, bad[0], counts[bad[0]], ecounts[bad[0]])
    assert (numpy.diff(offsets) == ecounts).all() and (offsets == eoffsets).all() and nb.shape == enb.shape, what
    assert (nb == enb).all(), "%s: %d of %d neighbors differ" % (what, (nb != enb).sum(), len(enb))
    if metric == "L2":
        assert (dist.view(numpy.uint32) == edist.view(numpy.uint32)).all(), what
    else:
        assert (numpy.abs(dist - edist) <= 2 * numpy.spacing(numpy.maximum(dist, edist))).all(), what
    # ---- float64 ----
    if metric == "L2" and not half2 and x.dtype == numpy.float32 and all(bool(numpy.isfinite(v).all()) for v in (x, c, q)):
        f64_check(x, a, K, q, r, offsets, nb, what)
    # ---- the search that ran ----
    lines = STATS.findall(text)
    total = int(eoffsets[-1])
    calls = 2 + (total > 0)                      # two counting calls, and a fill unless there is nothing to fill
    assert [ln[0] for ln in lines] == ["count", "count", "fill"][:calls], text
    numbers = [tuple(int(v) for v in ln[1:]) for ln in lines]
    assert all(t == numbers[0] for t in numbers), "%s: the statistics lines differ: %s" % (what, numbers)
    visited, scored, live, by_sets, chains = numbers[0]
    stats = dict(visited=visited, scored=scored, live=live, by_sets=by_sets, chains=chains, hits=total)
    print("radius statistics %s: %d hits, %d chains, %d live pairs, %d scored, %d visited; chains / live pairs = %s" % (
        what, total, chains, live, scored, visited, "%.4g" % (chains / live) if live else "-"))
    if expect is not None:
        assert expect in EXPECT
        chunk = int(env.get("KMCUDA_AMD_KNN_QUERY_CHUNK", 0))
        chunked = 0 < chunk < len(q)
        assert (INDEX_HALF_RANGE in text) == (expect == "index_half_range"), text
        # (one chunk of the batch leaves the range, in every one of the calls)
        assert text.count(QUERY_HALF_RANGE) == (calls if expect == "query_half_range" else 0), text
        assert (EXACT in text) == (expect != "f16" and index_has_no_filter(d, x.dtype == numpy.float16, env)), text
        if expect == "f16" or (expect == "query_half_range" and chunked):
            assert scored > 0, "%s: nothing was scored on the matrix cores" % what
        else:
            assert scored == 0 and live == 0 and chains == 0, "%s: the matrix-core filter ran: %s" % (what, stats)
        if expect == "f16":
            finite = int(numpy.isfinite(q.astype(numpy.float32)).all(axis=1).sum())
            members = a[a < K].astype(numpy.int64)
            sizes = numpy.bincount(members, minlength=K)
            assert total <= chains <= live <= visited <= finite * len(members), "%s: %s" % (what, stats)
            assert live <= scored and by_sets <= scored, "%s: %s" % (what, stats)
            # every cluster that holds a hit of a query was visited by that query, whole
            hq, hidx = numpy.nonzero(dm <= r)
            pairs = numpy.unique(hq * K + a[hidx].astype(numpy.int64))
            assert visited >= int(sizes[pairs % K].sum()), "%s: %s" % (what, stats)
    return counts, got, stats, text


def check_case(cs, name="target", **kw):
    return check_radius(cs.x, cs.c, cs.a, cs.q, cs.r[name], metric=cs.metric, qa=cs.qa, half2=cs.half2, dm=cs.dm, **kw)


def same(u, v):
    """Two results of check_radius: counts and CSR equal, distances as bit patterns."""
    return (u[0] == v[0]).all() and (u[1][0] == v[1][0]).all() and (u[1][1] == v[1][1]).all() and \
        (u[1][2].view(numpy.uint32) == v[1][2].view(numpy.uint32)).all()


# ----------------------------------------------------------------------------------------------------------------
# 1. every instantiation of knn_radius_f16_kernel<DP, METRIC, FASTX, FILL>
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ri.EQUAL_D + ri.PADDED_D)
@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_every_instantiation(metric, d):
    """D == DP (FASTX) at the widths no other radius test runs, and D < DP (rows zero-padded) at every width."""
    check_case(ri.instantiation(metric, d, False), expect="f16")


@pytest.mark.parametrize("d", ri.HALF_D)
@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_every_instantiation_fp16x2(metric, d):
    check_case(ri.instantiation(metric, d, True), expect="f16")


@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_eight_features_take_the_exact_kernel(metric):
    """filter_dp_for(8) = 8: below the f16 filter's 16, and radius search has no f32-filtered kernel."""
    check_case(ri.instantiation(metric, 8, False), expect="exact")


# ----------------------------------------------------------------------------------------------------------------
# 2. data range, L2 fp32
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ri.RANGE_D)
@pytest.mark.parametrize("scale", ri.SCALES)
def test_data_range(scale, d):
    """1e-6: half subnormals (amin's 6e-8 sqrt(DP) (qn + nmx) term); 6e4: the last binade of the half range; 2e5:
    beyond it, the exact kernel."""
    cs = ri.data_range(scale, d)
    top = max(ri.centred_top(cs))
    if scale == 6e4:
        assert top < 65504
    if scale == 2e5:
        assert ri.centred_top(cs)[0] > 65520
    check_case(cs, expect="index_half_range" if scale == 2e5 else "f16")


def test_fp32_subnormal_squared_distances():
    """Rows and queries at 1e-19: every squared difference is an fp32 subnormal, and so is r * r."""
    cs = ri.subnormal_squares()
    assert float(cs.r["target"]) ** 2 < 1.2e-38
    check_case(cs, expect="f16")


@pytest.mark.parametrize("d", [64, 512])
def test_offset_rows(d):
    check_case(ri.offset_rows(d), expect="f16")


def test_uniform_beyond_the_half_range():
    cs = ri.uniform_beyond()
    assert ri.centred_top(cs)[0] > 65520
    check_case(cs, expect="index_half_range")


# ----------------------------------------------------------------------------------------------------------------
# 3. one chunk leaves the half range
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 512])
def test_one_chunk_leaves_the_half_range(d):
    """Query 150 of 300 has a 1e6 feature.  Whole: the one chunk takes the exact kernel.  In chunks of 64 only
    [128, 192) does, the others stay on the filter; the answer is the same."""
    cs = ri.one_outlier_query(d)
    whole = check_case(cs, expect="query_half_range")
    chunked = check_case(cs, env={"KMCUDA_AMD_KNN_QUERY_CHUNK": 64}, expect="query_half_range")
    assert same(whole, chunked)
    assert whole[2]["scored"] == 0 and chunked[2]["scored"] > 0
    assert whole[0][150] == 0


@pytest.mark.parametrize("d,skew,xrange,qrange,want", ri.HALF_RANGE)
def test_fp16x2_across_the_half_range(d, skew, xrange, qrange, want):
    cs = ri.half_across(d, skew, xrange, qrange)
    assert ri.half_range_expectation(cs) == want
    check_case(cs, expect=want)


# ----------------------------------------------------------------------------------------------------------------
# 4. cluster and query-block sizes
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", ["every", "all"])
@pytest.mark.parametrize("d", ri.SIZED_D)
def test_cluster_sizes_around_the_tiles(d, radius):
    """Clusters of 1 ... 513 rows.  "every": each cluster holds a hit (and the radius is a pair's own distance: `<=`).
    "all": every clustered row is a hit of every query, so a padding row counted or a real row dropped at any tile
    end shows in the counts."""
    cs = ri.cluster_sizes(d)
    r = cs.r[radius]
    assert ri.hit_clusters(cs, r) == len(ri.SIZES)
    if radius == "all":
        assert (cs.counts(r) == len(cs.x)).all()
    counts, _, _, _ = check_case(cs, radius, expect="f16")
    if radius == "all":
        assert (counts == sum(ri.SIZES)).all()


@pytest.mark.parametrize("d,nq", ri.BLOCKS)
def test_query_blocks(d, nq):
    """All queries planned into one cluster: blocks of 128 queries (D = 512, 768) and of 512 (D = 16, 256), full, one
    short and one over."""
    cs = ri.query_blocks(d, nq)
    check_case(cs, expect="f16")


# ----------------------------------------------------------------------------------------------------------------
# 5. angular limits
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", ["switch", "below", "2.0", "pi/2"])
def test_angular_limits(radius):
    """r >= 3.1415925: amin = -inf; below it cosf(r), negative from pi / 2 on."""
    cs = ri.angular_limits()
    assert numpy.nanmax(cs.dm) < 3.1
    counts, _, _, _ = check_case(cs, radius, expect="f16")
    if radius in ("switch", "below"):
        assert (counts == (cs.a < len(cs.c)).sum()).all()


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16x2"])
@pytest.mark.parametrize("d", [16, 256, 768])
def test_angular_zero_and_everything(d, half):
    """Duplicates, near-duplicates whose product clamps to distance 0, antipodal rows: r = 0 returns exactly the
    oracle's zero-distance rows (fp32 rows of 256 and 768 features have none: the round-down chain leaves every product
    of two such unit rows below 1), r = 3.2 every clustered row."""
    cs = ri.unit_rows(d, half)
    zero = cs.counts(cs.r["0"])
    assert (zero == 0).any()
    if half or d == 16:
        assert (zero >= 1).sum() >= 20 and (zero >= 2).any()    # copies of rows, some of them duplicated rows
    counts, got, _, _ = check_case(cs, "0", expect="f16")
    assert (got[2] == 0).all() and (counts == zero).all()
    counts, _, _, _ = check_case(cs, "3.2", expect="f16")
    assert (counts == len(cs.x)).all()


# ----------------------------------------------------------------------------------------------------------------
# 6. degenerate corpus
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ptr", ["host", "device"])
@pytest.mark.parametrize("path", ["default", "exact"])
@pytest.mark.parametrize("d", [64, 1100])
def test_degenerate_corpus(d, path, ptr):
    """NaN rows, an inf feature, NaN and empty centroids, a one-row cluster, duplicates across clusters; NaN and inf
    queries."""
    cs = ri.degenerate_corpus(d)
    env = {"KMCUDA_AMD_KNN_EXACT": 1} if path == "exact" else {}
    counts, got, _, _ = check_case(cs, env=env, ptr=ptr, expect="f16" if (d, path) == (64, "default") else "exact")
    assert (counts[cs.bad] == 0).all() and counts.sum() > 0
    assert (cs.a[got[1].astype(numpy.int64)] < len(cs.c)).all()      # no row without a cluster
    assert (cs.a[got[1].astype(numpy.int64)] == 6).any()             # members of the cluster whose centroid is NaN
    assert len(cs.inf_rows) == 1 and not numpy.isin(got[1], cs.inf_rows).any()


# ----------------------------------------------------------------------------------------------------------------
# 7. prune paths
# ----------------------------------------------------------------------------------------------------------------
def test_assignments_not_the_nearest_centroid():
    """30 % of the rows in a random other cluster: radii that reach across the corpus, hits in clusters far from the
    query's own."""
    cs = ri.moved_rows()
    for radius in ("target", "wide"):
        check_case(cs, radius, expect="f16")


@pytest.mark.parametrize("radius", ["target", "wide"])
@pytest.mark.parametrize("d", [50, 64])
def test_exact_path_prunes(d, radius):
    """KMCUDA_AMD_KNN_EXACT: DP = D.  D = 64: the lb table; D = 50 (DP & 3 != 0): the triangle test with its relative
    margin.  "wide": hits in parts of the neighbouring blobs, clusters at every lower bound up to r."""
    cs = ri.instantiation("L2", d, False) if d == 50 else ri.data_range(1.0, d)
    assert radius == "target" or 2 <= numpy.median(ri.clusters_hit(cs, cs.r["wide"])) < len(cs.c) / 2
    check_case(cs, radius, env={"KMCUDA_AMD_KNN_EXACT": 1}, expect="exact")


@pytest.mark.parametrize("d", [50, 64, 600])
def test_lb_prune_at_a_wide_radius(d):
    """The default path's lb test (padded rows, D == DP, a wide instantiation) where partly covered clusters exist."""
    cs = ri.instantiation("L2", d, False) if d != 64 else ri.data_range(1.0, d)
    assert 2 <= numpy.median(ri.clusters_hit(cs, cs.r["wide"])) < len(cs.c) / 2
    check_case(cs, "wide", expect="f16")   # (how much lb prunes there is printed, not asserted: at D = 600 nothing)


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_query_order(order):
    """KMCUDA_AMD_KNN_ORDER (qperm): every order gives the oracle's CSR bit for bit, hence the same one."""
    check_case(ri.skewed(), env={"KMCUDA_AMD_KNN_ORDER": order}, expect="f16")


def test_tight_changes_nothing():
    """KMCUDA_AMD_KNN_TIGHT does not apply to a fixed radius -- the same result and the same work."""
    cs = ri.skewed()
    base = check_case(cs, expect="f16")
    loose = check_case(cs, env={"KMCUDA_AMD_KNN_TIGHT": 0}, expect="f16")
    assert same(base, loose) and base[2] == loose[2]


def test_half2_arithmetic_prunes_nothing():
    """KMCUDA_AMD_FP16_STRICT: the exact kernel in the reference's half2 arithmetic, prune_abs = inf."""
    cs = ri.half_strict()
    _, _, stats, _ = check_case(cs, expect="exact")
    finite = int(numpy.isfinite(cs.q.astype(numpy.float32)).all(axis=1).sum())
    assert stats["visited"] == finite * int((cs.a < len(cs.c)).sum())
