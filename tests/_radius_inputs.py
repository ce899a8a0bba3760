"""Inputs and ground truth of the radius-search tests (tests/test_gpu_knn_radius.py, tests/test_radius_bound_model.py;
the edge cases of tests/test_gpu_knn_radius_edges.py and their input checks, tests/test_radius_edges_inputs_cpu.py, at
the end of the file).

The corpus is the Gaussian mixture under an oracle k-means of tests/test_gpu_knn_query.py (rebuilt here; at N = 2000,
K = 16, seed 0 it leaves empty clusters and, in one case, a NaN centroid -- wanted).  The truth is the oracle's:
oracle.knn_query(k = N) returns, for every query, the exact distance to every clustered corpus row; a query's expected
hits are the rows with distance <= r in ascending (cluster id, row index) order.  Everything is computed once per
key."""
import numpy

import oracle

FLT_MAX = numpy.float32(3.402823466e+38)


def mixture(n, d, centres=12, seed=0, spread=10.0):
    rng = numpy.random.default_rng(seed)
    mu = rng.uniform(0, spread, (centres, d)).astype(numpy.float32)
    lab = rng.integers(0, centres, n)
    return (mu[lab] + rng.standard_normal((n, d)).astype(numpy.float32)).astype(numpy.float32), mu


def unit(x):
    return (x / numpy.linalg.norm(x, axis=1, keepdims=True)).astype(numpy.float32)


_CORPUS, _QUERIES, _DIST = {}, {}, {}


def clustered(n, d, metric="L2", half=False, clusters=16, seed=0):
    """(samples, centroids, assignments), read-only."""
    key = (n, d, metric, half, clusters, seed)
    if key not in _CORPUS:
        x, _ = mixture(n, d, seed=seed)
        if metric != "L2":
            x = unit(x - x.mean(axis=0))
        if half:
            x = x.astype(numpy.float16)
        c, a, _ = oracle.kmeans(x, clusters, seed=seed, metric=metric, init="random")
        for v in (x, c, a):
            v.setflags(write=False)
        _CORPUS[key] = (x, c, a)
    return _CORPUS[key]


def fresh_queries(q, n, d, metric="L2", half=False, seed=0):
    """q rows near the corpus of clustered(n, d, metric, half): corpus rows plus noise, some exact copies."""
    key = (q, n, d, metric, half, seed)
    if key not in _QUERIES:
        x = clustered(n, d, metric, half, seed=seed)[0].astype(numpy.float32)
        rng = numpy.random.default_rng(100 + seed)
        rows = x[rng.choice(len(x), q)]
        noise = rng.standard_normal((q, d)).astype(numpy.float32)
        out = rows + (0.7 if metric == "L2" else 0.03) * noise
        out[::17] = rows[::17]
        # a few rows far from every corpus row: no hits at the radii of the tests
        far = rng.uniform(-60, 80, (5, d)) if metric == "L2" else -x.mean(axis=0) + 0.05 * rng.standard_normal((5, d))
        out[-5:] = far.astype(numpy.float32)
        if metric != "L2":
            out = unit(out)
        out = numpy.ascontiguousarray(out.astype(numpy.float16 if half else numpy.float32))
        out.setflags(write=False)
        _QUERIES[key] = out
    return _QUERIES[key]


def all_distances(x, c, a, q, metric="L2", half2=False):
    """Q x N float32: the oracle's exact distance of every query to every corpus row that has a cluster, NaN elsewhere
    (rows without a cluster; every entry of a query with a NaN or inf feature).  half2: a distance that overflows the
    half range is inf in the reference's half2 arithmetic, never pushed by its search and within no radius: NaN here.

    With k = N the heap never fills and nothing is pruned, so the distances do not depend on the centroids -- but for
    one thing: the reference's procedure never visits a cluster whose centroid is not finite (its C entries are NaN),
    and the brute-force set holds that cluster's members too.  The oracle therefore gets the first finite centroid in
    the place of every non-finite one.  A pair that is still missing must be one whose distance oracle.distance gives
    as NaN or inf (a row with an inf feature): no hit at any radius."""
    n, clusters = len(x), len(c)
    a = numpy.asarray(a)
    broken = ~numpy.isfinite(c.astype(numpy.float32)).all(axis=1)
    if broken.any():
        c = c.copy()
        c[broken] = c[numpy.nonzero(~broken)[0][0]]
    nb, dist = oracle.knn_query(n, x, c, a, q, metric=metric, half2=half2)
    members = int((a < clusters).sum())
    out = numpy.full((len(q), n), numpy.nan, numpy.float32)
    ok = nb[:, 0] != 0xFFFFFFFF
    # (the lists come out sorted: the filled slots first, then index 0 and FLT_MAX)
    rows, slots = numpy.nonzero(ok[:, None] & (dist[:, :members] != FLT_MAX))
    out[rows, nb[rows, slots].astype(numpy.int64)] = dist[rows, slots]
    assert numpy.isnan(out[:, a >= clusters]).all()
    if not half2:
        gaps = numpy.argwhere(numpy.isnan(out) & ok[:, None] & (a < clusters)[None, :])
        assert len(gaps) <= 0.01 * out.size, "the oracle's lists are not complete"
        x32, q32 = x.astype(numpy.float32), q.astype(numpy.float32)
        for i, j in gaps:
            assert not numpy.isfinite(oracle.distance(q32[i], x32[j], metric)), "the oracle's lists are not complete"
    return out


def truth(n, d, metric="L2", half=False, q=300):
    """(x, c, a, queries, distances Q x N) of the standard case, cached."""
    key = (n, d, metric, half, q)
    if key not in _DIST:
        x, c, a = clustered(n, d, metric, half)
        qs = fresh_queries(q, n, d, metric, half)
        dm = all_distances(x, c, a, qs, metric)
        dm.setflags(write=False)
        _DIST[key] = (x, c, a, qs, dm)
    return _DIST[key]


def expected(dm, a, r):
    """(counts, offsets, neighbors, distances) of the brute-force radius search over the distance matrix dm."""
    a = numpy.asarray(a).astype(numpy.int64)
    qi, idx = numpy.nonzero(dm <= numpy.float32(r))   # (NaN compares false; row-major: ascending idx per query)
    order = numpy.lexsort((idx, a[idx], qi))
    qi, idx = qi[order], idx[order]
    counts = numpy.bincount(qi, minlength=dm.shape[0]).astype(numpy.uint32)
    offsets = numpy.zeros(dm.shape[0] + 1, numpy.int64)
    numpy.cumsum(counts, out=offsets[1:])
    return counts, offsets, idx.astype(numpy.uint32), dm[qi, idx]


def target_radius(dm, kth=21):
    """The median distance to the kth nearest clustered row."""
    finite = dm[~numpy.isnan(dm).all(axis=1)]
    return numpy.float32(numpy.median(numpy.sort(numpy.nan_to_num(finite, nan=numpy.inf), axis=1)[:, kth - 1]))


def gap_radius(dm, target, around=200):
    """The midpoint of the widest gap between consecutive distinct distances among the `around` values nearest `target`."""
    v = numpy.unique(dm[~numpy.isnan(dm)])
    near = numpy.sort(v[numpy.argsort(numpy.abs(v - target), kind="stable")[:around]])
    i = int(numpy.argmax(numpy.diff(near)))
    return numpy.float32((numpy.float64(near[i]) + numpy.float64(near[i + 1])) / 2)


def ulps_from(dm, r):
    """The smallest distance, in float32 ulps of r, between r and an entry of dm."""
    v = dm[~numpy.isnan(dm)].astype(numpy.float64)
    return float(numpy.abs(v - numpy.float64(r)).min() / numpy.spacing(numpy.float32(r)))


# ----------------------------------------------------------------------------------------------------------------
# The edge cases (tests/test_gpu_knn_radius_edges.py).  Every builder returns a Case, computed once per key; the corpora
# and query batches are those of tests/test_gpu_knn_edges.py and tests/test_gpu_knn_query_edges.py (imported when a
# case is built: those modules need torch, this one's first half does not).
# ----------------------------------------------------------------------------------------------------------------
ANGULAR_SWITCH = numpy.float32(3.1415925)   # knn_radius.hip: amin = -inf from this radius on


class Case:
    """A corpus (x, c, a), a query batch q (with its clusters qa, or None: the index computes them), the oracle's
    distance matrix dm and the radii r (a dict: name -> float32) of one edge case."""

    def __init__(self, x, c, a, q, metric="L2", qa=None, half2=False, radii=None, **more):
        self.x, self.c, self.q = x, c, numpy.ascontiguousarray(q)
        self.a = numpy.ascontiguousarray(a, dtype=numpy.uint32)
        self.qa = None if qa is None else numpy.ascontiguousarray(qa, dtype=numpy.uint32)
        self.metric, self.half2 = metric, half2
        self.dm = all_distances(x, c, self.a, self.q, metric, half2)
        self.r = dict(radii(self) if radii else {"target": target_radius(self.dm), "wide": wide_radius(self.dm)})
        self.__dict__.update(more)
        for v in (self.x, self.c, self.a, self.q, self.dm):
            v.setflags(write=False)

    def counts(self, r):
        return expected(self.dm, self.a, r)[0]


def wide_radius(dm):
    """The tenth percentile of all distances: a query's hits are its own blob and PARTS of the blobs next to it, so
    the clusters that matter sit at every lower bound between 0 and r -- where a prune test that is too eager shows."""
    return numpy.float32(numpy.quantile(dm[~numpy.isnan(dm)].astype(numpy.float64), 0.10))


def clusters_hit(cs, r):
    """Per query: in how many clusters it has a hit."""
    hits = cs.dm <= numpy.float32(r)
    a = cs.a.astype(numpy.int64)
    per = numpy.zeros((len(cs.q), len(cs.c)), bool)
    qi, idx = numpy.nonzero(hits)
    per[qi, a[idx]] = True
    return per.sum(axis=1)


_CASES = {}


def case(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


def _edges():
    import test_gpu_knn_edges
    import test_gpu_knn_query_edges
    return test_gpu_knn_edges, test_gpu_knn_query_edges


def _unit64(v):
    return v / numpy.linalg.norm(v, axis=1, keepdims=True)


def angular_clearance(dm, r):
    """ulps_from over the distances an acos produced: a distance of exactly 0 is the clamp's (`p >= 1 ? 0 : acos(p)`,
    no acos on either side, tests/_angular.py) and equal on the device and in the oracle."""
    return ulps_from(numpy.where(dm == 0, numpy.float32(numpy.nan), dm), r)


def angular_radius(cs):
    """target_radius moved into the widest gap nearby (the tests assert its clearance)."""
    return {"target": gap_radius(cs.dm, target_radius(cs.dm))}


def rows_of(d):
    return 2500 if d <= 256 else 1200


# ---- 1. every instantiation -------------------------------------------------------------------------------------
EQUAL_D = [16, 32, 128, 768, 1024]                       # D == DP
PADDED_D = [9, 12, 24, 50, 100, 200, 300, 600, 900]      # D < DP: rows zero-padded, FASTX = false
HALF_D = [50, 200, 600]


def instantiation(metric, d, half):
    """24 blobs of spread 0.05 in the unit cube and the standard query batch; angular: centred and normalised."""
    def make():
        e, qe = _edges()
        x, c, a = e.blobs(rows_of(d), d, 24, 1.0, seed=300 + d, spread=0.05)
        if metric != "L2":
            mean = x.mean(axis=0)
            x, c = _unit64(x - mean).astype(numpy.float32), _unit64(c - mean).astype(numpy.float32)
        if half:
            x, c = x.astype(numpy.float16), c.astype(numpy.float16)
        if half or metric != "L2":
            a = oracle.lloyd_assign(x.astype(numpy.float32), c.astype(numpy.float32), metric=metric)[0]
        # angular: the blobs' angular spread is 0.05 sqrt(D) / sqrt(D / 12) = 0.17 rad, sigma per feature of a unit row
        sigma = 0.05 if metric == "L2" else 0.17 / numpy.sqrt(d)
        q = qe.batch(x, c, sigma, seed=d, unit=metric != "L2")
        return Case(x, c, a, q, metric, radii=None if metric == "L2" else angular_radius)
    return case(("inst", metric, d, half), make)


# ---- 2. data range ----------------------------------------------------------------------------------------------
SCALES = [1e-6, 1.0, 6e4, 2e5]
RANGE_D = [16, 64, 256, 512, 1024]


def data_range(scale, d):
    """The corpus and queries of test_gpu_knn_query_edges.test_data_range."""
    def make():
        e, qe = _edges()
        x, c, a = e.blobs(rows_of(d), d, 24, scale, seed=d + int(numpy.log10(scale) * 7) + 100, spread=0.05)
        q = qe.batch(x, c, 0.05 * scale, seed=d, far=(0.0, 1.0) if scale == 6e4 else (-3.0, 4.0))
        return Case(x, c, a, q)
    return case(("range", scale, d), make)


def centred_top(cs):
    """The largest |centred value| of the corpus rows and of the queries (centre: the mean of the finite centroids)."""
    c32 = cs.c.astype(numpy.float32)
    mu = c32[numpy.isfinite(c32).all(axis=1)].mean(axis=0)
    return (float(numpy.abs(cs.x.astype(numpy.float32) - mu).max()), float(numpy.abs(cs.q.astype(numpy.float32) - mu).max()))


def subnormal_squares():
    def make():
        e, qe = _edges()
        x, c, a = e.blobs(2500, 16, 24, 1e-19, seed=51)
        return Case(x, c, a, qe.batch(x, c, 0.15e-19, seed=52, far=(0.0, 1.0)))
    return case(("1e-19",), make)


def offset_rows(d):
    def make():
        e, qe = _edges()
        x, c, a = e.blobs(rows_of(d), d, 24, 1.0, seed=41, offset=1e4)
        return Case(x, c, a, qe.batch(x, c, 0.15, seed=d))
    return case(("offset", d), make)


def uniform_beyond():
    """test_gpu_knn_edges.test_uniform_beyond_the_half_range's rows (2500 of them), uniform queries and 20 copies."""
    def make():
        rs = numpy.random.RandomState(16)
        x = (rs.rand(2500, 16) * 2e5).astype(numpy.float32)
        c = x[rs.choice(2500, 20, replace=False)].copy()
        a = oracle.lloyd_assign(x, c)[0]
        q = (rs.rand(280, 16) * 2e5).astype(numpy.float32)
        q[:20] = x[rs.choice(2500, 20, replace=False)]
        return Case(x, c, a, q)
    return case(("uniform",), make)


# ---- 3. one chunk leaves the half range ---------------------------------------------------------------------------
def one_outlier_query(d):
    """test_gpu_knn_query_edges.test_one_chunk_leaves_the_half_range: 300 queries, number 150 with a 1e6 feature."""
    def make():
        e, qe = _edges()
        x, c, a = e.blobs(2500 if d == 64 else 1200, d, 24, 1.0, seed=71 + d, spread=0.05)
        q = qe.batch(x, c, 0.05, seed=72, fresh=250)
        assert len(q) == 300
        q[150, 5] = 1e6
        return Case(x, c, a, q)
    return case(("outlier", d), make)


HALF_RANGE = [(64, False, 3e4, 6e4, "query_half_range"), (512, False, 3e4, 6e4, "query_half_range"),
              (64, True, 6e4, 6e4, "index_half_range"), (512, True, 6e4, 6e4, "index_half_range"),
              (64, False, 3e4, 3e4, "f16")]


def half_across(d, skew, xrange, qrange):
    """test_gpu_knn_query_edges.test_fp16x2_across_the_half_range's half corpus and queries."""
    def make():
        rs = numpy.random.RandomState(d + skew)
        n, K = 2400 if d == 64 else 1200, 20
        x = rs.uniform(-xrange, xrange, (n, d))
        if skew:
            x[: int(0.9 * n)] = rs.uniform(xrange / 2, xrange, (int(0.9 * n), d))
        x16 = x.astype(numpy.float16)
        c16 = x16[rs.choice(int(0.9 * n) if skew else n, K, replace=False)].copy()
        a = oracle.lloyd_assign(x16.astype(numpy.float32), c16.astype(numpy.float32))[0]
        q16 = rs.uniform(-qrange, qrange, (300, d)).astype(numpy.float16)
        q16[:20] = x16[rs.choice(n, 20, replace=False)]
        q16[20:30] = q16[30:40]
        return Case(x16, c16, a, q16)
    return case(("half-across", d, skew, xrange, qrange), make)


def half_range_expectation(cs):
    """Which search the centred values ask for, with no borderline rounding deciding (asserted)."""
    top_x, top_q = centred_top(cs)
    assert abs(top_x - 65520) > 16 and abs(top_q - 65520) > 16
    return "index_half_range" if top_x >= 65520 else ("query_half_range" if top_q >= 65520 else "f16")


# ---- 4. cluster and query-block sizes -----------------------------------------------------------------------------
SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 129, 511, 513]
SIZED_D = [16, 64, 256, 512, 768]
BLOCKS = [(512, n) for n in (127, 128, 129, 300)] + [(768, n) for n in (127, 128, 129, 300)] + \
         [(16, n) for n in (511, 512, 513)] + [(256, n) for n in (511, 512, 513)]


def _sized(d):
    e, _ = _edges()
    return case(("sized-corpus", d), lambda: e.sized(SIZES, d, seed=71 + d))


def sized_radii(cs):
    """"every": the smallest radius at which every cluster holds a hit of some query -- the distance of a pair itself,
    which `<=` includes; "all": just above the largest distance, every clustered row a hit of every query."""
    per_cluster = [numpy.nanmin(cs.dm[:, cs.a == k]) for k in range(len(cs.c))]
    return {"every": numpy.float32(max(per_cluster)),
            "all": numpy.nextafter(numpy.nanmax(cs.dm), numpy.float32(numpy.inf))}


def cluster_sizes(d):
    def make():
        _, qe = _edges()
        x, c, a = _sized(d)
        return Case(x, c, a, qe.batch(x, c, 0.12, seed=d), radii=sized_radii)
    return case(("sized", d), make)


def hit_clusters(cs, r):
    """How many clusters hold at least one hit of some query."""
    a = cs.a.astype(numpy.int64)
    _, idx = numpy.nonzero(cs.dm <= numpy.float32(r))
    return len(numpy.unique(a[idx]))


def query_blocks(d, nq):
    """nq queries around the centre of the 513-row cluster, all planned into it (query_assignments)."""
    def make():
        x, c, a = _sized(d)
        rs = numpy.random.RandomState(nq)
        big = SIZES.index(513)
        q = (c[big] + rs.randn(nq, d) * 0.12).astype(numpy.float32)
        q[:20] = x[rs.choice(len(x), 20, replace=False)]
        q[20:30] = q[30:40]
        return Case(x, c, a, q, qa=numpy.full(nq, big, numpy.uint32))
    return case(("blocks", d, nq), make)


# ---- 5. angular limits ---------------------------------------------------------------------------------------------
def angular_limits():
    """The standard angular D = 64 corpus at the kernel's switch constant, the float below it, 2.0 and pi / 2."""
    def make():
        x, c, a = clustered(2000, 64, "angular")
        q = fresh_queries(300, 2000, 64, "angular")
        below = numpy.nextafter(ANGULAR_SWITCH, numpy.float32(0))
        return Case(x, c, a, q, "angular", radii=lambda cs: {
            "switch": ANGULAR_SWITCH, "below": below, "2.0": numpy.float32(2.0), "pi/2": numpy.float32(1.5707964)})
    return case(("angular-limits",), make)


def unit_rows(d, half):
    """test_gpu_knn_query_edges.test_angular_outside_queries: duplicates, near-duplicates that clamp to distance 0 and
    antipodal rows, with queries around rows, random directions, near-copies, copies and negations."""
    def make():
        e, _ = _edges()
        n, K = 2000, 20
        dtype = numpy.float16 if half else numpy.float32
        x = e.unit_corpus(n, d, seed=d + half).astype(dtype)
        rs = numpy.random.RandomState(d)
        c = x[rs.choice(n, K, replace=False)].copy()
        x32 = x.astype(numpy.float32)
        a = oracle.lloyd_assign(x32, c.astype(numpy.float32), metric=oracle.COS)[0]
        pick = lambda m: x32[rs.choice(n, m, replace=False)].astype(numpy.float64)   # noqa: E731
        fresh = _unit64(pick(200) * 4 + rs.randn(200, d))
        far = _unit64(rs.randn(20, d))
        near = _unit64(pick(20) + rs.randn(20, d) * 1e-7)
        q = numpy.concatenate([fresh, far, near]).astype(dtype)
        q = numpy.concatenate([q, x[rs.choice(n, 20, replace=False)], (-pick(20)).astype(dtype)])
        q = numpy.concatenate([q, q[rs.choice(len(q), 10, replace=False)]])
        q = numpy.ascontiguousarray(q[rs.permutation(len(q))])
        return Case(x, c, a, q, "angular", radii=lambda cs: {"0": numpy.float32(0), "3.2": numpy.float32(3.2)})
    return case(("unit", d, half), make)


# ---- 6. degenerate corpus ------------------------------------------------------------------------------------------
def degenerate_corpus(d):
    def make():
        _, qe = _edges()
        x, c, a, q, bad = qe.degenerate_queries(d)
        return Case(x, c, a, q, bad=bad, inf_rows=numpy.nonzero(numpy.isinf(x).any(axis=1))[0])
    return case(("degenerate", d), make)


# ---- 7. prune paths --------------------------------------------------------------------------------------------------
def moved_rows():
    """30 % of the rows in a random other cluster: the radii grow, the prune stays sound."""
    def make():
        e, qe = _edges()
        x, c, a = e.blobs(2500, 64, 24, 1.0, seed=91)
        rs = numpy.random.RandomState(91)
        moved = rs.choice(2500, 750, replace=False)
        a = a.copy()
        a[moved] = (a[moved] + rs.randint(1, 24, 750)) % 24
        return Case(x, c, a, qe.batch(x, c, 0.15, seed=92))
    return case(("moved",), make)


def skewed():
    """The corpus of test_order_and_tight."""
    def make():
        e, qe = _edges()
        x, c, a = e.sized([3000, 1200, 600] + [40] * 40 + [1, 2, 3], 64, seed=131)
        return Case(x, c, a, qe.batch(x, c, 0.12, seed=132))
    return case(("skewed",), make)


def half_strict():
    """Half blobs for KMCUDA_AMD_FP16_STRICT: the oracle in the reference's half2 arithmetic."""
    def make():
        _, qe = _edges()
        x, c, a = qe.half_case(64, "L2")
        return Case(x, c, a, qe.half_batch(x, c, "L2", seed=92), half2=True)
    return case(("half2",), make)
