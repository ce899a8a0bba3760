"""The k-NN index (kmcuda_amd.KnnIndex, knn_index.cpp, the search kernels' SELF = false mode) against its bit-exact
CPU oracle, oracle.knn_query -- DESIGN.md 4.8 point 2 in plain C -- at the edges where a filtered search goes wrong, for
queries that are NOT corpus rows: data far from unit scale, a chunk that leaves the half range between chunks that do
not, fp16x2 queries whose clusters the index computes, angular queries, non-finite queries and whole chunks of them,
cluster sizes and query batches around the kernels' tiles, k around the heap sizes and beyond the candidates, every
query-mode switch, and cluster ids that are legal but wrong.

One helper checks every case.  L2 (and the half2 arithmetic of KMCUDA_AMD_FP16_STRICT): indices equal the oracle's bit
for bit and distances equal as bit patterns, NaN rows and FLT_MAX filler slots included (a NaN slot must be NaN on both
sides; its payload is nobody's contract).  Angular: an entry may differ only under the rule of tests/_angular.py, every
returned distance is within 2 float32 ulp of oracle.distance.  Clusters the index computed equal oracle.lloyd_assign.
Finite L2 inputs also pass a float64 order check that the oracle and the kernels cannot both get wrong the same way.
`expect` names the search that must have run, read from what verbosity=1 prints (the index prints no f16 statistics
line: f16 against f32 is set by the environment and confirmed by the absence of the other lines)."""
import numpy
import pytest

import oracle
from _angular import assert_knn_only_acos_matters, assert_only_acos_matters
from test_gpu_kmeans import StdoutListener
from test_gpu_knn_edges import blobs, degenerate, sized, unit_corpus

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NONE = 0xFFFFFFFF
FLT_MAX = numpy.finfo(numpy.float32).max
EXACT = "every candidate is evaluated with the exact arithmetic"
INDEX_HALF_RANGE = "k-NN index: a centred row leaves the half range"
QUERY_HALF_RANGE = "k-NN query: a centred query leaves the half range"
PATHS = {"f16": {}, "f32": {"KMCUDA_AMD_FILTER": "f32"}, "exact": {"KMCUDA_AMD_KNN_EXACT": 1}}
EXPECT = ("f16", "f32", "exact", "index_half_range_f32", "index_half_range_exact", "query_half_range_f32",
          "query_half_range_exact")


def _bits(d):
    """float32 bit patterns, every NaN mapped to one pattern."""
    d = numpy.ascontiguousarray(d, dtype=numpy.float32)
    return numpy.where(numpy.isnan(d), numpy.uint32(0x7FC00000), d.view(numpy.uint32))


def _f64_query_check(x, a, K, q, k, nb, rows):
    """test_gpu_knn_edges._f64_check, query against corpus: the float64 distances of a returned list are the k
    smallest float64 distances to the rows that have a cluster, in order."""
    x64 = x.astype(numpy.float64)
    cand = numpy.nonzero(a < K)[0]
    for i in rows:
        qi = q[i].astype(numpy.float64)
        d = numpy.sqrt(((x64[cand] - qi) ** 2).sum(axis=1))
        m = min(k, d.size)
        want = numpy.sort(numpy.partition(d, m - 1)[:m] if m < d.size else d)[:m]
        got = numpy.sqrt(((x64[nb[i, :m].astype(numpy.int64)] - qi) ** 2).sum(axis=1))
        assert numpy.allclose(got, want, rtol=1e-5, atol=0), (int(i), got, want)


def run_query(k, x, c, a, q, qa, metric, ptr, **kw):
    """One KnnIndex build + query with verbosity 1; numpy results (uint32 views) and what the library printed."""
    from kmcuda_amd import KnnIndex
    out = StdoutListener()
    with out:
        if ptr == "host":
            with KnnIndex(x, c, a, metric=metric, verbosity=1) as ix:
                res = ix.query(q, k, query_assignments=qa, **kw)
        else:
            dev = torch.device("cuda", 0)
            tx, tc, tq = (torch.from_numpy(v).to(dev) for v in (x, c, q))
            ta = torch.from_numpy(a.view(numpy.int32)).to(dev)
            tqa = None if qa is None else torch.from_numpy(qa.view(numpy.int32)).to(dev)
            with KnnIndex(tx, tc, ta, metric=metric, verbosity=1) as ix:
                res = ix.query(tq, k, query_assignments=tqa, **kw)
            res = res if isinstance(res, tuple) else (res,)
            res = tuple(r.cpu().numpy().view(numpy.uint32) if r.dtype == torch.int32 else r.cpu().numpy() for r in res)
            res = res if len(res) > 1 else res[0]
    return res, out.text


def check_query(k, x, c, a, q, qa=None, metric="L2", env=None, ptr="host", expect=None, monkeypatch=None, half2=False,
                rows=60, seed=0):
    """KnnIndex(x, c, a).query(q, k) == oracle.knn_query(k, x, c, a, q): see the module's docstring.  `expect` in EXPECT:
    the search that must have run (a `query_half_range_*` line exactly once).  half2: KMCUDA_AMD_FP16_STRICT is set and
    the oracle runs the reference's half2 arithmetic.  Returns (neighbors, distances, printed text)."""
    for key, v in (env or {}).items():
        monkeypatch.setenv(key, str(v))
    a = numpy.ascontiguousarray(a, dtype=numpy.uint32)
    q = numpy.ascontiguousarray(q)
    qa = None if qa is None else numpy.ascontiguousarray(qa, dtype=numpy.uint32)
    assert x.dtype == c.dtype == q.dtype
    res, text = run_query(k, x, c, a, q, qa, metric, ptr, return_assignments=qa is None)
    nb, dist = res[0], res[1]
    x32, c32, q32 = x.astype(numpy.float32), c.astype(numpy.float32), q.astype(numpy.float32)
    K = len(c)
    finite = numpy.isfinite(q32).all(axis=1)
    what = "%s D=%d k=%d %s %s" % (metric, x.shape[1], k, ptr, env)
    # ---- the clusters the index computed (4.8 point 1; a non-finite query has none, whatever the pass wrote) ----
    if qa is None:
        got_qa = res[2]
        ref_qa, _, _ = oracle.lloyd_assign(q32, c32, metric=metric)
        if metric == "L2":
            bad = numpy.nonzero(got_qa[finite] != ref_qa[finite])[0]
            assert bad.size == 0, "%s: %d query clusters differ from the oracle's" % (what, bad.size)
        else:
            assert_only_acos_matters(q32[finite], c32, got_qa[finite], ref_qa[finite], what)
    # ---- the lists ----
    ref_nb, ref_dist = oracle.knn_query(k, x if half2 else x32, c if half2 else c32, a, q if half2 else q32,
                                        query_assignments=qa, metric=metric, half2=half2)
    assert (nb[~finite] == NONE).all() and numpy.isnan(dist[~finite]).all(), what
    if metric == "L2":
        bad = numpy.nonzero((nb != ref_nb).any(axis=1))[0]
        assert bad.size == 0, "%s: %d lists differ from the oracle, first %d: %s vs %s" % (
            what, bad.size, bad[0], nb[bad[0]], ref_nb[bad[0]])
        bad = numpy.nonzero((_bits(dist) != _bits(ref_dist)).any(axis=1))[0]
        assert bad.size == 0, "%s: %d distance rows differ from the oracle, first %d: %s vs %s" % (
            what, bad.size, bad[0], dist[bad[0]], ref_dist[bad[0]])
    else:
        allowed = assert_knn_only_acos_matters(x32, nb, ref_nb, what, queries=q32)
        print("angular allowance: %d of %d rows (%s)" % (allowed, len(q), what))
        filler = ref_dist == FLT_MAX             # slots no candidate filled, and the rows without a cluster: exact
        assert (filler == (dist == FLT_MAX)).all() and (nb[filler] == 0).all(), what
        assert (numpy.isnan(dist) == numpy.isnan(ref_dist)).all(), what
        for i, j in zip(*numpy.nonzero(~filler & ~numpy.isnan(ref_dist))):
            want = numpy.float32(oracle.distance(q32[i], x32[nb[i, j]], metric=oracle.COS))
            assert abs(dist[i, j] - want) <= 2 * numpy.spacing(max(dist[i, j], want)), (what, i, j, dist[i, j], want)
    # ---- float64 order (not under the half2 arithmetic, whose distances are sums of halves) ----
    if metric == "L2" and not half2 and all(bool(numpy.isfinite(v).all()) for v in (x32, c32, q32)):
        rs = numpy.random.RandomState(seed)
        sel = numpy.arange(len(q)) if len(q) <= rows else rs.choice(len(q), rows, replace=False)
        _f64_query_check(x32, a, K, q32, k, nb, sel)
    # ---- the search that ran ----
    if expect is not None:
        assert expect in EXPECT
        assert (EXACT in text) == (expect == "exact"), text
        assert (INDEX_HALF_RANGE in text) == expect.startswith("index_half_range"), text
        assert text.count(QUERY_HALF_RANGE) == (1 if expect.startswith("query_half_range") else 0), text
        if expect == "index_half_range_f32":
            assert INDEX_HALF_RANGE + ", the f32 matrix-core filter" in text, text
        if expect == "index_half_range_exact":
            assert INDEX_HALF_RANGE + ", every candidate is evaluated exactly" in text, text
        if expect == "query_half_range_f32":
            assert QUERY_HALF_RANGE + ", the f32 matrix-core filter" in text, text
        if expect == "query_half_range_exact":
            assert QUERY_HALF_RANGE + ", the exact search" in text, text
    return nb, dist, text


def batch(x, c, sigma, seed, fresh=200, far=(-3.0, 4.0), a=None, unit=False):
    """The standard query batch: `fresh` new draws from the corpus's blobs (centres c, spread sigma), 20 rows far
    outside every cluster (uniform over the centres' box stretched by `far`; unit: random directions), 20 exact copies
    of corpus rows, 10 duplicated queries; shuffled.  unit: the new rows are normalised (the copies stay copies)."""
    rs = numpy.random.RandomState(seed)
    x32, c32 = x.astype(numpy.float32), c.astype(numpy.float32)
    fin = c32[numpy.isfinite(c32).all(axis=1)]
    lo, span = float(fin.min()), float(fin.max() - fin.min())
    new = fin[rs.randint(0, len(fin), fresh)] + rs.randn(fresh, x.shape[1]) * sigma
    outside = rs.uniform(lo + far[0] * span, lo + far[1] * span, (20, x.shape[1]))
    if unit:
        new, outside = _unit(new), _unit(rs.randn(20, x.shape[1]))
    ok = numpy.nonzero(numpy.isfinite(x32).all(axis=1) & (True if a is None else a < len(c)))[0]
    copies = x[rs.choice(ok, 20, replace=False)]
    q = numpy.concatenate([new.astype(x.dtype), outside.astype(x.dtype), copies])
    q = numpy.concatenate([q, q[rs.choice(len(q), 10, replace=False)]])
    return numpy.ascontiguousarray(q[rs.permutation(len(q))])


def _unit(v):
    return v / numpy.linalg.norm(v, axis=1, keepdims=True)


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ----------------------------------------------------------------------------------------------------------------
# 1. data range, fp32 L2
# ----------------------------------------------------------------------------------------------------------------
RANGE = [(s, d, f) for s in (1e-6, 1.0, 6e4, 2e5) for d in (16, 64, 256, 512, 1024) for f in ("f16", "f32")
         if not (f == "f32" and d > 256)]


@pytest.mark.parametrize("scale,d,filt", RANGE)
def test_data_range(scale, d, filt, monkeypatch):
    n = 2500 if d <= 256 else 1200
    x, c, a = cached(("range", scale, d), lambda: blobs(n, d, 24, scale, seed=d + int(numpy.log10(scale) * 7) + 100,
                                                        spread=0.05))
    # (at 6e4 the far rows stay in the centres' box: a query outside it would leave the half range on its own)
    q = batch(x, c, 0.05 * scale, seed=d, far=(0.0, 1.0) if scale == 6e4 else (-3.0, 4.0))
    if scale == 6e4:
        assert max(numpy.abs(x - c.mean(axis=0)).max(), numpy.abs(q - c.mean(axis=0)).max()) < 65504   # just inside
    if scale == 2e5:
        assert numpy.abs(x - c.mean(axis=0)).max() > 65520                                             # beyond it
    expect = filt if scale < 1e5 or filt == "f32" else ("index_half_range_f32" if d <= 256 else "index_half_range_exact")
    check_query(10, x, c, a, q, env={"KMCUDA_AMD_FILTER": filt}, monkeypatch=monkeypatch, expect=expect, seed=d)


@pytest.mark.parametrize("d", [64, 512])
def test_offset_rows(d, monkeypatch):
    """Unit spread at offset 1e4: the centred rows and queries are unit-scale, the f16 filter stays on."""
    x, c, a = blobs(2500 if d == 64 else 1200, d, 24, 1.0, seed=41, offset=1e4)
    check_query(10, x, c, a, batch(x, c, 0.15, seed=d), monkeypatch=monkeypatch, expect="f16")


@pytest.mark.parametrize("filt", ["f16", "f32"])
def test_fp32_subnormal_squared_distances(filt, monkeypatch):
    """Rows and queries at 1e-19: every squared difference is an fp32 subnormal."""
    x, c, a = blobs(2500, 16, 24, 1e-19, seed=51)
    q = batch(x, c, 0.15e-19, seed=52, far=(0.0, 1.0))
    qa, _, _ = oracle.lloyd_assign(q, c)
    assert max((x - c[a]).max(), (q - c[qa]).max()) ** 2 < 1.2e-38
    check_query(10, x, c, a, q, env={"KMCUDA_AMD_FILTER": filt}, monkeypatch=monkeypatch, expect=filt)


def test_beyond_the_filters_widths(monkeypatch):
    x, c, a = blobs(1200, 1152, 24, 1.0, seed=61, spread=0.05)
    check_query(10, x, c, a, batch(x, c, 0.05, seed=62), monkeypatch=monkeypatch, expect="exact")


# ----------------------------------------------------------------------------------------------------------------
# 2. the per-chunk fallback: `cp` belongs to the chunk, `path` to the index
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 512])
def test_one_chunk_leaves_the_half_range(d, monkeypatch):
    x, c, a = blobs(2500 if d == 64 else 1200, d, 24, 1.0, seed=71 + d, spread=0.05)
    q = batch(x, c, 0.05, seed=72, fresh=250)
    assert len(q) == 300
    q[150, 5] = 1e6                                     # chunk 2 of [0,64) [64,128) [128,192) [192,256) [256,300)
    expect = "query_half_range_f32" if d == 64 else "query_half_range_exact"
    whole = check_query(10, x, c, a, q, monkeypatch=monkeypatch, expect=expect)
    chunked = check_query(10, x, c, a, q, env={"KMCUDA_AMD_KNN_QUERY_CHUNK": 64}, monkeypatch=monkeypatch, expect=expect)
    assert (whole[0] == chunked[0]).all() and (_bits(whole[1]) == _bits(chunked[1])).all()


# ----------------------------------------------------------------------------------------------------------------
# 3. fp16x2
# ----------------------------------------------------------------------------------------------------------------
def half_case(d, metric):
    """Half-valued blobs (unit rows for the angular metric), K = 24 half centroids, the oracle's assignments."""
    def make():
        x, c, _ = blobs(2000 if d <= 64 else 1200, d, 24, 1.0, seed=81 + d)
        if metric != "L2":
            mean = x.mean(axis=0)
            x, c = _unit(x - mean), _unit(c - mean)
        x16, c16 = x.astype(numpy.float16), c.astype(numpy.float16)
        a, _, _ = oracle.lloyd_assign(x16.astype(numpy.float32), c16.astype(numpy.float32), metric=metric)
        return x16, c16, a
    return cached(("half", d, metric), make)


def half_batch(x16, c16, metric, seed):
    return batch(x16, c16, 0.15 if metric == "L2" else 0.05, seed, unit=metric != "L2")


@pytest.mark.parametrize("metric", ["L2", "angular"])
@pytest.mark.parametrize("d,path", [(64, "f16"), (64, "f32"), (64, "exact"), (512, "f16"), (512, "exact")])
def test_fp16x2_outside_queries_computed_clusters(metric, d, path, monkeypatch):
    """launch_half_to_float -> the engine's lloyd_assign on half-valued rows -> the search."""
    x, c, a = half_case(d, metric)
    q = half_batch(x, c, metric, seed=82)
    check_query(10, x, c, a, q, metric=metric, env=PATHS[path], monkeypatch=monkeypatch, expect=path)


@pytest.mark.parametrize("d,skew,xrange,qrange,want", [
    (64, False, 6e4, 6e4, "index_half_range_f32"), (64, True, 6e4, 6e4, "index_half_range_f32"),
    (512, True, 6e4, 6e4, "index_half_range_exact"), (64, False, 3e4, 6e4, "query_half_range_f32"),
    (512, False, 3e4, 6e4, "query_half_range_exact"), (64, False, 3e4, 3e4, "f16")])
def test_fp16x2_across_the_half_range(d, skew, xrange, qrange, want, monkeypatch):
    """The +-6e4 half corpus of test_gpu_knn_edges.test_fp16x2_across_the_half_range, skewed and not, with outside half
    queries: centred by the mean of the centroids a value can reach twice 65504 and the INDEX leaves the half range.
    The same at +-3e4 stays inside; then queries over +-6e4 leave it on their own, queries over +-3e4 do not."""
    rs = numpy.random.RandomState(d + skew)
    n, K = 2400 if d == 64 else 1200, 20
    x = rs.uniform(-xrange, xrange, (n, d))
    if skew:
        x[: int(0.9 * n)] = rs.uniform(xrange / 2, xrange, (int(0.9 * n), d))
    x16 = x.astype(numpy.float16)
    c16 = x16[rs.choice(int(0.9 * n) if skew else n, K, replace=False)].copy()
    a, _, _ = oracle.lloyd_assign(x16.astype(numpy.float32), c16.astype(numpy.float32))
    q16 = rs.uniform(-qrange, qrange, (300, d)).astype(numpy.float16)
    q16[:20] = x16[rs.choice(n, 20, replace=False)]
    q16[20:30] = q16[30:40]
    mu = c16.astype(numpy.float32).mean(axis=0)
    top_x, top_q = numpy.abs(x16.astype(numpy.float32) - mu).max(), numpy.abs(q16.astype(numpy.float32) - mu).max()
    assert abs(top_x - 65520) > 16 and abs(top_q - 65520) > 16          # no borderline rounding decides the path
    tail = "f32" if d <= 256 else "exact"
    expect = "index_half_range_" + tail if top_x >= 65520 else ("query_half_range_" + tail if top_q >= 65520 else "f16")
    assert expect == want
    check_query(10, x16, c16, a, q16, monkeypatch=monkeypatch, expect=expect)


@pytest.mark.parametrize("d", [32, 64])
def test_fp16_strict_is_the_half2_oracle(d, monkeypatch):
    """KMCUDA_AMD_FP16_STRICT: radii, centroid distances, mydist and every candidate distance in the reference's half2
    arithmetic.  Sums of halves tie often; the oracle, given the same clusters, supplies the ties."""
    x, c, a = half_case(d, "L2")
    q = half_batch(x, c, "L2", seed=92)
    qa, _, _ = oracle.lloyd_assign(q.astype(numpy.float32), c.astype(numpy.float32))
    nb, dist, _ = check_query(10, x, c, a, q, qa=qa, env={"KMCUDA_AMD_FP16_STRICT": 1}, monkeypatch=monkeypatch,
                              expect="exact", half2=True)
    plain = oracle.knn_query(10, x, c, a, q, query_assignments=qa)[1]
    assert (dist != plain).any()                        # the half2 arithmetic is in effect
    assert (numpy.diff(dist, axis=1) == 0).any()        # and the case does hold ties


def test_fp16x2_device_pointers(monkeypatch):
    x, c, a = half_case(64, "L2")
    check_query(10, x, c, a, half_batch(x, c, "L2", seed=93), ptr="device", monkeypatch=monkeypatch, expect="f16")


# ----------------------------------------------------------------------------------------------------------------
# 4. angular, outside queries
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("d,path", [(16, "f16"), (256, "f16"), (768, "f16"), (16, "f32"), (16, "exact")])
def test_angular_outside_queries(d, path, half, monkeypatch):
    n, K = 2000, 20
    dtype = numpy.float16 if half else numpy.float32
    x = unit_corpus(n, d, seed=d + half).astype(dtype)
    rs = numpy.random.RandomState(d)
    c = x[rs.choice(n, K, replace=False)].copy()
    x32 = x.astype(numpy.float32)
    a, _, _ = oracle.lloyd_assign(x32, c.astype(numpy.float32), metric=oracle.COS)
    pick = lambda m: x32[rs.choice(n, m, replace=False)].astype(numpy.float64)   # noqa: E731
    fresh = _unit(pick(200) * 4 + rs.randn(200, d))                    # around corpus rows
    far = _unit(rs.randn(20, d))                                       # random directions: near nothing
    near = _unit(pick(20) + rs.randn(20, d) * 1e-7)                    # products >= 1 clamp to distance 0
    q = numpy.concatenate([fresh, far, near]).astype(dtype)
    q = numpy.concatenate([q, x[rs.choice(n, 20, replace=False)], (-pick(20)).astype(dtype)])   # copies, negations
    q = numpy.concatenate([q, q[rs.choice(len(q), 10, replace=False)]])
    q = numpy.ascontiguousarray(q[rs.permutation(len(q))])
    check_query(10, x, c, a, q, metric="angular", env=PATHS[path], monkeypatch=monkeypatch, expect=path)


# ----------------------------------------------------------------------------------------------------------------
# 5. degenerate corpus, non-finite queries
# ----------------------------------------------------------------------------------------------------------------
def degenerate_queries(d):
    x, c, a = degenerate(d)
    _, c0, _ = blobs(2000, d, 30, 1.0, seed=61 + d)           # the centres before degenerate() broke two of them
    rs = numpy.random.RandomState(d)
    noise = lambda m: (rs.randn(m, d) * 0.05).astype(numpy.float32)   # noqa: E731
    rest = numpy.setdiff1d(numpy.arange(2000), numpy.nonzero(numpy.isnan(x).any(axis=1))[0])
    dup = rest[100:110]
    assert (x[dup] == x[rest[200:210]]).all()
    finite = numpy.isfinite(x).all(axis=1)
    q = numpy.concatenate([
        c0[4] + noise(15), c0[5] + noise(15),                # near the empty clusters' (former) centroids
        numpy.repeat(x[a == 7], 3, axis=0),                  # the one-row cluster's row, three times
        x[numpy.nonzero((a == 6) & finite)[0][:8]],          # rows of the cluster whose centroid is NaN
        x[dup],                                              # rows that exist twice, in different clusters
        batch(x, c, 0.15, seed=d, fresh=120, a=a),
    ]).astype(numpy.float32)
    q = q[rs.permutation(len(q))]
    bad = rs.choice(len(q), 8, replace=False)
    q[bad[:6], rs.randint(0, d, 6)] = numpy.nan              # 6 NaN queries (not always feature 0)
    q[bad[0], 0] = numpy.nan
    q[bad[6], 1], q[bad[7], d - 1] = numpy.inf, -numpy.inf   # 2 inf queries
    return x, c, a, numpy.ascontiguousarray(q), numpy.sort(bad)


@pytest.mark.parametrize("ptr", ["host", "device"])
@pytest.mark.parametrize("path", ["f16", "f32", "exact", "exact_wide"])
def test_degenerate_corpus(path, ptr, monkeypatch):
    x, c, a, q, bad = cached(("degenerate", path == "exact_wide"),
                             lambda: degenerate_queries(1100 if path == "exact_wide" else 64))
    nb, dist, _ = check_query(10, x, c, a, q, ptr=ptr, env=PATHS.get(path, {}), monkeypatch=monkeypatch,
                              expect="exact" if path == "exact_wide" else path)
    assert (nb[bad] == NONE).all() and numpy.isnan(dist[bad]).all()
    none = numpy.nonzero(a >= 30)[0]
    assert not numpy.isin(nb, none).any()                    # corpus rows without a cluster are never returned


@pytest.mark.parametrize("path", ["f16", "f32", "exact"])
def test_every_query_non_finite(path, monkeypatch):
    """An empty block plan: nblocks == 0, p_end == p_base, the preparation kernels with zero assigned rows."""
    x, c, a = degenerate(64)
    q = numpy.ones((40, 64), numpy.float32)
    q[numpy.arange(40), numpy.arange(40)] = numpy.where(numpy.arange(40) % 3 == 0, numpy.inf, numpy.nan)
    for qa in (None, numpy.zeros(40, numpy.uint32)):
        nb, dist, _ = check_query(3, x, c, a, q, qa=qa, env=PATHS[path], monkeypatch=monkeypatch, expect=path)
        assert (nb == NONE).all() and numpy.isnan(dist).all()


@pytest.mark.parametrize("path", ["f16", "f32", "exact"])
def test_a_chunk_of_nan_queries_between_two_others(path, monkeypatch):
    x, c, a = degenerate(64)
    q = batch(x, c, 0.15, seed=5, fresh=50, a=a)[:96].copy()
    q[32:64, 7] = numpy.nan
    env = dict(PATHS[path], KMCUDA_AMD_KNN_QUERY_CHUNK=32)
    nb, dist, _ = check_query(10, x, c, a, q, env=env, monkeypatch=monkeypatch, expect=path)
    assert (nb[32:64] == NONE).all() and numpy.isnan(dist[32:64]).all()
    assert (nb[:32] != NONE).all() and (nb[64:] != NONE).all()


# ----------------------------------------------------------------------------------------------------------------
# 6. shapes
# ----------------------------------------------------------------------------------------------------------------
SIZES = [1, 31, 32, 33, 511, 512, 513, 1023, 1025, 2, 64, 96]


@pytest.mark.parametrize("d", [16, 64, 512])
def test_cluster_sizes_around_the_tiles(d, monkeypatch):
    x, c, a = cached(("sized", d), lambda: sized(SIZES, d, seed=71 + d))
    check_query(10, x, c, a, batch(x, c, 0.12, seed=d), monkeypatch=monkeypatch, expect="f16")


def test_one_cluster_holds_ninety_percent(monkeypatch):
    x, c, a = sized([2700] + [15] * 20, 64, seed=81)
    check_query(10, x, c, a, batch(x, c, 0.12, seed=81), monkeypatch=monkeypatch, expect="f16")


@pytest.mark.parametrize("filt", ["f16", "f32"])
def test_assignments_not_the_nearest_centroid(filt, monkeypatch):
    """Legal inputs: 30 % of the corpus rows in a random other cluster (the radii grow, the prune stays sound)."""
    x, c, a = blobs(3000, 64, 30, 1.0, seed=91)
    rs = numpy.random.RandomState(91)
    moved = rs.choice(3000, 900, replace=False)
    a = a.copy()
    a[moved] = (a[moved] + rs.randint(1, 30, 900)) % 30
    check_query(10, x, c, a, batch(x, c, 0.15, seed=92), env={"KMCUDA_AMD_FILTER": filt}, monkeypatch=monkeypatch,
                expect=filt)


@pytest.mark.parametrize("nq", [513, 1025])
def test_batch_concentrated_in_one_cluster(nq, monkeypatch):
    """Every query in cluster 8 (1025 rows): the block plan of one cluster around 512 and 1024 queries."""
    x, c, a = cached(("sized", 64), lambda: sized(SIZES, 64, seed=71 + 64))
    rs = numpy.random.RandomState(nq)
    q = (c[8] + rs.randn(nq, 64) * 0.12).astype(numpy.float32)
    q[:20] = x[rs.choice(len(x), 20, replace=False)]
    q[20:30] = q[30:40]
    check_query(10, x, c, a, q, qa=numpy.full(nq, 8, numpy.uint32), monkeypatch=monkeypatch, expect="f16")


@pytest.mark.parametrize("nq", [1, 31, 33])
def test_small_batches(nq, monkeypatch):
    x, c, a = cached(("sized", 64), lambda: sized(SIZES, 64, seed=71 + 64))
    check_query(10, x, c, a, batch(x, c, 0.12, seed=nq)[:nq], monkeypatch=monkeypatch, expect="f16")


# ----------------------------------------------------------------------------------------------------------------
# 7. k
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 32, 64, 65, 200])
def test_k(k, monkeypatch):
    x, c, a = cached(("k",), lambda: blobs(3000, 64, 30, 1.0, seed=101))
    check_query(k, x, c, a, batch(x, c, 0.15, seed=102), monkeypatch=monkeypatch, expect="f16", rows=30)


@pytest.mark.parametrize("k", [39, 40])
def test_k_at_n(k, monkeypatch):
    x, c, a = blobs(40, 64, 4, 1.0, seed=111)
    nb, _, _ = check_query(k, x, c, a, batch(x, c, 0.15, seed=112), monkeypatch=monkeypatch)
    assert (numpy.sort(nb[:, :39], axis=1) < 40).all()
    if k == 40:
        assert (numpy.sort(nb, axis=1) == numpy.arange(40)).all()     # every corpus row, once


def test_filler_tail(monkeypatch):
    """k = N on a corpus where 5 rows have no cluster: the last 5 slots hold index 0 at FLT_MAX (row 0 has no cluster,
    so a 0 there is the filler and nothing else)."""
    x, c, a = blobs(200, 64, 6, 1.0, seed=121)
    a = a.astype(numpy.uint32)
    a[[0, 50, 51, 120, 199]] = [NONE, 6, NONE, 6, 9]
    nb, dist, _ = check_query(200, x, c, a, batch(x, c, 0.15, seed=122, a=a), monkeypatch=monkeypatch)
    assert (nb[:, 195:] == 0).all() and (dist[:, 195:] == FLT_MAX).all()
    assert (nb[:, :195] != 0).all() and (dist[:, :195] < FLT_MAX).all()


@pytest.mark.parametrize("k", [1, 65])
@pytest.mark.parametrize("ptr", ["host", "device"])
def test_without_distances(k, ptr, monkeypatch):
    """distances == nullptr inside SELF = false: the lists are those of the call that returns distances."""
    x, c, a = cached(("k",), lambda: blobs(3000, 64, 30, 1.0, seed=101))
    q = batch(x, c, 0.15, seed=131)
    nb, _, _ = check_query(k, x, c, a, q, ptr=ptr, monkeypatch=monkeypatch, expect="f16")
    only, _ = run_query(k, x, c, numpy.ascontiguousarray(a, dtype=numpy.uint32), q, None, "L2", ptr,
                        return_distances=False)
    assert only.shape == nb.shape and (only == nb).all()


# ----------------------------------------------------------------------------------------------------------------
# 8. switches of the query mode
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1, 2, 3])
@pytest.mark.parametrize("tight", [0, 1])
def test_order_and_tight(order, tight, monkeypatch):
    """launch_knn_centroid_bounds reads a.qxs, launch_knn_query_order a.qoffsets and a.qmydist."""
    x, c, a = cached(("skewed",), lambda: sized([3000, 1200, 600] + [40] * 40 + [1, 2, 3], 64, seed=131))
    check_query(10, x, c, a, batch(x, c, 0.12, seed=132), env={"KMCUDA_AMD_KNN_ORDER": order, "KMCUDA_AMD_KNN_TIGHT": tight},
                monkeypatch=monkeypatch, expect="f16")


@pytest.mark.parametrize("K", [8000, 8200])
def test_many_clusters(K, monkeypatch):
    """Above 8192 clusters the query-order key has no 32 bits left: identity order."""
    x, c, a = blobs(3 * K, 16, K, 1.0, seed=121, spread=0.02)
    check_query(5, x, c, a, batch(x, c, 0.02, seed=K, fresh=250), monkeypatch=monkeypatch, expect="f16", rows=40)


# ----------------------------------------------------------------------------------------------------------------
# 9. wrong but legal clusters
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["f16", "f32", "exact"])
def test_wrong_but_legal_clusters(path, monkeypatch):
    """A random cluster per query on a corpus with duplicate rows (in the same and in different clusters).  Under ties
    the visiting order is the cluster's, so the oracle gets the same ids."""
    def make():
        x, c, a = blobs(3000, 64, 30, 1.0, seed=141)
        x[1000:1100] = x[:100]
        a = a.copy()
        a[1000:1100] = a[:100]
        a[1050:1100] = (a[1050:1100] + 7) % 30
        return x, c, a
    x, c, a = cached(("dups",), make)
    q = batch(x, c, 0.15, seed=142)
    q[:40] = x[:40]                                     # queries AT the duplicated rows
    qa = numpy.random.RandomState(143).randint(0, 30, len(q)).astype(numpy.uint32)
    check_query(10, x, c, a, q, qa=qa, env=PATHS[path], monkeypatch=monkeypatch, expect=path)
