"""Masked radius search (KnnIndex.query_radius_allow; kmamd_knn_index_radius_count_allow / _fill_allow; the MASK
instantiations of knn_radius.hip).

A radius result is a brute-force set, so the masked result is defined three ways that must agree bit for bit; one helper
(check_masked) holds every masked call -- the counting form and the full one -- against all of them:
  (a) the oracle's distance matrix with the denied columns struck out, thresholded (L2 and the half2 arithmetic on bit
      patterns; angular within 2 float32 ulp at a radius 4 ulp clear of every oracle distance, as the unmasked tests);
  (b) the unmasked call on the SAME index with the denied rows deleted from its CSR;
  (c) the unmasked call on a FRESH index built from the assignments with every denied row's set to K;
  (d) and the unmasked call after the masked ones returns what it returned before.
Which search ran is read from the statistics lines (scored > 0: the f16 kernel, scored == 0: the exact one)."""
import ctypes

import numpy
import pytest

import _radius_inputs as ri
from _radius_inputs import all_distances, expected
from test_gpu_knn_allow import patched, sorted_order
from test_gpu_knn_radius_edges import STATS, environment
from test_gpu_kmeans import StdoutListener

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EXPECT = ("f16", "exact", "mixed")


def host(v):
    if isinstance(v, numpy.ndarray):
        return v
    v = v.cpu().numpy()
    return v.view(numpy.uint32) if v.dtype == numpy.int32 else v


def run(ix, q, r, mask=None, qa=None):
    """(counts, offsets, neighbors, distances) on the host, and the numbers of the statistics lines the two calls
    (counting, then full) printed."""
    out = StdoutListener()
    with out:
        if mask is None:
            counts = ix.query_radius(q, r, query_assignments=qa, count_only=True)
            full = ix.query_radius(q, r, query_assignments=qa)
        else:
            counts = ix.query_radius_allow(q, r, mask, query_assignments=qa, count_only=True)
            full = ix.query_radius_allow(q, r, mask, query_assignments=qa)
    res = tuple(host(v) for v in (counts,) + tuple(full))
    lines = STATS.findall(out.text)
    assert [ln[0] for ln in lines] == ["count", "count", "fill"][:2 + (int(res[1][-1]) > 0)], out.text
    numbers = [tuple(int(v) for v in ln[1:]) for ln in lines]
    assert all(t == numbers[0] for t in numbers), "the statistics lines differ: %s" % numbers
    visited, scored, live, by_sets, chains = numbers[0]
    assert res[0].dtype == numpy.uint32 and res[1].dtype == numpy.int64 and res[2].dtype == numpy.uint32
    assert (numpy.diff(res[1]) == res[0]).all()
    return res, dict(visited=visited, scored=scored, live=live, by_sets=by_sets, chains=chains)


def same(u, v, what):
    """Two tuples of arrays: equal, float32 ones as bit patterns."""
    assert len(u) == len(v)
    for i, (g, w) in enumerate(zip(u, v)):
        assert g.shape == w.shape, "%s: array %d has another shape (%s against %s)" % (what, i, g.shape, w.shape)
        if g.dtype == numpy.float32:
            g, w = g.view(numpy.uint32), w.view(numpy.uint32)
        bad = numpy.nonzero(g != w)[0]
        assert bad.size == 0, "%s: array %d differs in %d places, first at %d: %s against %s" % (
            what, i, bad.size, bad[0], g[bad[0]], w[bad[0]])


def struck(res, mask):
    """An unmasked result with the denied rows deleted."""
    counts, offsets, nb, dist = res
    keep = numpy.asarray(mask)[nb.astype(numpy.int64)] != 0
    qi = numpy.repeat(numpy.arange(len(counts)), numpy.diff(offsets))
    c2 = numpy.bincount(qi[keep], minlength=len(counts)).astype(numpy.uint32)
    o2 = numpy.zeros(len(counts) + 1, numpy.int64)
    numpy.cumsum(c2, out=o2[1:])
    return c2, o2, nb[keep], dist[keep]


def check_masked(x, c, a, q, radii, masks, metric="L2", qa=None, env=None, expect="f16", half2=False, dm=None,
                 ptr="host", fresh=True):
    """Every mask of `masks` (name -> flags per row) at every radius of `radii` on ONE KnnIndex(x, c, a): see the
    module's docstring.  expect: the search the calls must have run, in EXPECT ("mixed": some chunks on either).
    ptr = "device": the index, the queries and the masks as tensors.  Returns {(name, r): (result, statistics)} with
    the unmasked calls under the name None."""
    from kmcuda_amd import KnnIndex
    assert expect in EXPECT
    a = numpy.ascontiguousarray(a, dtype=numpy.uint32)
    q = numpy.ascontiguousarray(q)
    K = len(c)
    env = dict(env or {})
    if half2:
        env["KMCUDA_AMD_FP16_STRICT"] = 1
    if dm is None:
        dm = all_distances(x, c, a, q, metric, half2)
    dev = torch.device("cuda", 0)

    def give(v, labels=False):
        if v is None or ptr == "host":
            return v
        v = numpy.array(v)
        return torch.from_numpy(v.view(numpy.int32) if labels else v).to(dev)

    def ran(stats, hits, what):
        if expect == "exact":
            assert stats["scored"] == 0 and stats["live"] == 0 and stats["chains"] == 0, "%s: the f16 kernel ran: %s" % (what, stats)
        elif hits:   # (a hit of the f16 kernel has been scored; "mixed": most chunks stay on it)
            assert stats["scored"] > 0 and stats["chains"] >= (hits if expect == "f16" else 1), "%s: %s" % (what, stats)

    out = {}
    with environment(env):
        with KnnIndex(give(x), give(c), give(a, True), metric=metric) as ix:
            gq, gqa = give(q), give(qa, True)
            for r in radii:
                r = numpy.float32(r)
                if metric != "L2":
                    clear = ri.angular_clearance(dm, r)
                    assert clear >= 4, "an oracle distance %.2f ulp from the radius %r" % (clear, float(r))
                base, bstats = run(ix, gq, r, None, gqa)
                assert expect != "f16" or bstats["scored"] > 0
                ran(bstats, int(base[1][-1]), "unmasked")
                out[(None, float(r))] = (base, bstats)
                for name, mask in masks.items():
                    mask = numpy.asarray(mask)
                    what = "%s: %s %s D=%d r=%r %s %s, %d of %d rows allowed" % (
                        name, metric, x.dtype, x.shape[1], float(r), ptr, env, int((mask != 0).sum()), len(x))
                    got, stats = run(ix, gq, r, give(mask), gqa)
                    # (a) the oracle
                    allowed = dm.copy()
                    allowed[:, mask == 0] = numpy.nan
                    ecounts, eoffsets, enb, edist = expected(allowed, a, r)
                    same(got[:3], (ecounts, eoffsets, enb), what + " against the oracle")
                    if metric == "L2":
                        same(got[3:], (edist,), what + " against the oracle's distances")
                    else:
                        assert (numpy.abs(got[3] - edist) <= 2 * numpy.spacing(numpy.maximum(got[3], edist))).all(), what
                    # (b) the unmasked call of this index, the denied rows struck out
                    same(got, struck(base, mask), what + " against the unmasked call, filtered")
                    # (c) the unmasked call of the index the masked call is defined by
                    ap = patched(a, mask, K)
                    if fresh and (ap < K).any():
                        with KnnIndex(give(x), give(c), give(ap, True), metric=metric) as fx:
                            want, _ = run(fx, gq, r, None, gqa)
                        same(got, want, what + " against the fresh index")
                    ran(stats, int(got[1][-1]), what)
                    assert stats["visited"] <= bstats["visited"], what   # (radii over fewer rows prune no less)
                    out[(name, float(r))] = (got, stats)
                # (d) the index is what it was
                again, astats = run(ix, gq, r, None, gqa)
                same(again, base, "the unmasked call after the masked ones, r=%r" % float(r))
                assert astats == bstats
    return out


def check_case(cs, names, masks, **kw):
    return check_masked(cs.x, cs.c, cs.a, cs.q, [cs.r[n] for n in names], masks, metric=cs.metric, qa=cs.qa,
                        half2=cs.half2, dm=cs.dm, **kw)


def half_mask(n, seed=0, p=0.5):
    return numpy.random.RandomState(seed).rand(n) < p


# ----------------------------------------------------------------------------------------------------------------
# 1. every masked f16 instantiation
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ri.EQUAL_D + ri.PADDED_D)
@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_every_masked_f16_instantiation(metric, d):
    cs = ri.instantiation(metric, d, False)
    check_case(cs, ["target", "wide"] if metric == "L2" else ["target"], {"half": half_mask(len(cs.x), d)}, expect="f16")


@pytest.mark.parametrize("d", ri.HALF_D)
@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_every_masked_f16_instantiation_fp16x2(metric, d):
    cs = ri.instantiation(metric, d, True)
    check_case(cs, ["target", "wide"] if metric == "L2" else ["target"], {"half": half_mask(len(cs.x), d)}, expect="f16",
               ptr="device")


# ----------------------------------------------------------------------------------------------------------------
# 2. every route to the masked exact kernel
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"KMCUDA_AMD_KNN_EXACT": 1}, {"KMCUDA_AMD_FILTER": "f32"}])
@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_switches_take_the_masked_exact_kernel(metric, env):
    cs = ri.instantiation(metric, 128, False)
    check_case(cs, ["target", "wide"] if metric == "L2" else ["target"], {"half": half_mask(len(cs.x), 1)}, env=env,
               expect="exact")


def test_half2_arithmetic_prunes_nothing():
    cs = ri.half_strict()
    out = check_case(cs, ["target"], {"half": half_mask(len(cs.x), 2)}, expect="exact")
    finite = int(numpy.isfinite(cs.q.astype(numpy.float32)).all(axis=1).sum())
    r = float(cs.r["target"])
    # every cluster keeps an allowed row here, and nothing is pruned: every finite query visits every member
    assert out[("half", r)][1]["visited"] == out[(None, r)][1]["visited"] == finite * int((cs.a < len(cs.c)).sum())


@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_wide_rows(metric):
    x, c, a, q, dm = ri.truth(2000, 1152, metric)
    r = ri.target_radius(dm) if metric == "L2" else ri.gap_radius(dm, ri.target_radius(dm))
    check_masked(x, c, a, q, [r], {"half": half_mask(2000, 3)}, metric=metric, dm=dm, expect="exact")


def test_an_index_beyond_the_half_range():
    cs = ri.uniform_beyond()
    assert ri.centred_top(cs)[0] > 65520
    check_case(cs, ["target", "wide"], {"half": half_mask(len(cs.x), 4)}, expect="exact")


def test_one_chunk_leaves_the_half_range():
    """Query 150 has a 1e6 feature.  One chunk: all of it on the exact kernel.  Chunks of 64: only [128, 192)."""
    cs = ri.one_outlier_query(64)
    masks = {"half": half_mask(len(cs.x), 5)}
    r = float(cs.r["target"])
    whole = check_case(cs, ["target"], masks, expect="exact")
    chunked = check_case(cs, ["target"], masks, env={"KMCUDA_AMD_KNN_QUERY_CHUNK": 64}, expect="mixed")
    same(whole[("half", r)][0], chunked[("half", r)][0], "one chunk against chunks of 64")
    assert whole[("half", r)][1]["scored"] == 0 and chunked[("half", r)][1]["scored"] > 0
    assert whole[("half", r)][0][0][150] == 0


# ----------------------------------------------------------------------------------------------------------------
# 3. bit, sub-tile and ring edges
# ----------------------------------------------------------------------------------------------------------------
def layout(a, K):
    """(order: sorted position -> row, offsets of the clusters in it)."""
    return sorted_order(a, K), numpy.concatenate([[0], numpy.cumsum(numpy.bincount(a[a < K], minlength=K))])


def sub_tile_of(a, K):
    """Per row: (its cluster, the 32-row sub-tile of the cluster it lies in) -- tiles start at a cluster's first row."""
    order, offsets = layout(a, K)
    sub = numpy.zeros(len(a), numpy.int64)
    for cl in range(K):
        rows = order[offsets[cl]:offsets[cl + 1]]
        sub[rows] = numpy.arange(len(rows)) // 32
    return sub


def edge_masks(a, K, d):
    """name -> mask, built through the sorted order of the corpus.  d: the tiles of the f16 kernel hold two sub-tiles
    up to 256 features (DP), one beyond."""
    n = len(a)
    order, offsets = layout(a, K)
    sizes = numpy.diff(offsets)
    sub = sub_tile_of(a, K)
    per_tile = 2 if d <= 256 else 1
    big = int(numpy.argmax(sizes))
    masks = {}
    for p in (31, 32, 33, 63, 64, 65):
        m = numpy.zeros(n, bool)
        m[order[p]] = True
        masks["position %d alone" % p] = m
    first, last, tail = numpy.zeros(n, bool), numpy.zeros(n, bool), numpy.zeros(n, bool)
    for cl in range(K):
        if sizes[cl]:
            first[order[offsets[cl]]] = True
            last[order[offsets[cl + 1] - 1]] = True
            tail[order[offsets[cl] + 32 * ((sizes[cl] - 1) // 32):offsets[cl + 1]]] = True
    masks["the first row of every cluster"] = first
    masks["the last row of every cluster"] = last
    masks["the last sub-tile of every cluster"] = tail
    second = numpy.zeros(n, bool)
    second[order[::2]] = True
    masks["every second position"] = second
    but_one = numpy.ones(n, bool)
    but_one[order[64]] = False
    masks["everything but one row"] = but_one
    for j in range((sizes[big] + 31) // 32):
        masks["sub-tile %d of the largest cluster" % j] = (a == big) & (sub == j)
    masks["even sub-tiles"] = sub % 2 == 0          # (two per tile: sub-tile 0 of every tile)
    masks["odd sub-tiles"] = sub % 2 == 1           # (sub-tile 1 of every tile; the clusters up to 32 rows denied)
    masks["even tiles"] = (sub // per_tile) % 2 == 0
    masks["odd tiles"] = (sub // per_tile) % 2 == 1
    masks["the largest cluster denied"] = a != big
    masks["only the largest cluster"] = a == big
    return masks


@pytest.mark.parametrize("env,expect", [({}, "f16"), ({"KMCUDA_AMD_KNN_EXACT": 1}, "exact")])
@pytest.mark.parametrize("radius", ["all", "every"])
@pytest.mark.parametrize("d", [16, 64, 512])
def test_bit_sub_tile_and_ring_edges(d, radius, env, expect):
    """Clusters of 1 ... 513 rows; d = 16, 64: two sub-tiles per tile and the deeper ring, d = 512: one and two
    buffers.  "all": every allowed clustered row is a hit of every query, so one row dropped or one too many shows."""
    cs = ri.cluster_sizes(d)
    K = len(cs.c)
    masks = edge_masks(cs.a, K, d)
    own = oracle_clusters(cs)
    assert (own == int(numpy.argmax(numpy.bincount(cs.a)))).sum() > 5     # "denied": some queries' own cluster
    out = check_case(cs, [radius], masks, env=env, expect=expect)
    if radius == "all":
        for name, mask in masks.items():
            counts = out[(name, float(cs.r["all"]))][0][0]
            assert (counts == int(mask.sum())).all(), name


def oracle_clusters(cs):
    import oracle
    return oracle.lloyd_assign(cs.q.astype(numpy.float32), cs.c.astype(numpy.float32))[0]


@pytest.mark.parametrize("env,expect", [({}, "f16"), ({"KMCUDA_AMD_KNN_EXACT": 1}, "exact")])
def test_one_cluster(env, expect):
    from test_gpu_knn_edges import sized
    from test_gpu_knn_query_edges import batch
    x, c, a = sized([300], 64, seed=7)
    q = batch(x, c, 0.12, seed=8, fresh=60)
    dm = all_distances(x, c, a, q)
    masks = {"half": half_mask(300, 6), "position 0 alone": numpy.arange(300) == sorted_order(a, 1)[0],
             "odd sub-tiles": sub_tile_of(a, 1) % 2 == 1}
    check_masked(x, c, a, q, [ri.target_radius(dm), numpy.nextafter(numpy.nanmax(dm), numpy.float32(numpy.inf))], masks,
                 dm=dm, env=env, expect=expect)


# ----------------------------------------------------------------------------------------------------------------
# 4. the skip is real and exact
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 64, 512])
def test_a_clear_sub_tile_is_not_scored(d):
    """At "all" nothing is pruned and every cluster keeps an allowed row under "even sub-tiles", so every wave that
    scores at all walks every cluster, and `scored` grows by the same amount per scored sub-tile of a wave -- 1024 per
    operand set with a live query, the same in every cluster.  An unmasked wave scores ceil(size / 32) sub-tiles of a
    cluster; a masked one those with an allowed row.  Hence scored(mask) * (all sub-tiles) == scored(all-true) * (the
    sub-tiles that are not clear), exactly."""
    cs = ri.cluster_sizes(d)
    K = len(cs.c)
    sub = sub_tile_of(cs.a, K)
    even = sub % 2 == 0
    out = check_case(cs, ["all"], {"all-true": numpy.ones(len(cs.x), bool), "even sub-tiles": even}, expect="f16", fresh=False)
    r = float(cs.r["all"])
    plain, full, masked = (out[(name, r)][1] for name in (None, "all-true", "even sub-tiles"))
    assert full == plain                                   # every number of the statistics line
    assert 0 < masked["scored"] < full["scored"]
    sizes = numpy.bincount(cs.a, minlength=K)
    every = int(((sizes + 31) // 32).sum())
    kept = len({(int(cl), int(j)) for cl, j in zip(cs.a[even], sub[even])})
    assert kept == int((((sizes + 31) // 32 + 1) // 2).sum()) and kept < every
    assert masked["scored"] * every == full["scored"] * kept, (masked, full, every, kept)
    assert masked["visited"] == full["visited"]            # (the clusters visited, whole: the reference's count)


# ----------------------------------------------------------------------------------------------------------------
# 5. degenerate masks and rows
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,expect", [({}, "f16"), ({"KMCUDA_AMD_KNN_EXACT": 1}, "exact")])
def test_degenerate_masks_and_rows(env, expect):
    """The D = 64 corpus of test_gpu_knn_radius.py with duplicates and rows without a cluster (their flags are
    ignored), NaN and inf queries."""
    from test_gpu_knn_radius import edge_corpus
    x, c, a = edge_corpus()
    K, n = len(c), len(x)
    q = numpy.ascontiguousarray(ri.fresh_queries(300, n, 64)[:120]).copy()
    q[1, 3] = numpy.nan
    q[3, 0] = numpy.inf
    q[5, 63] = -numpy.inf
    dm = all_distances(x, c, a, q)
    r = ri.target_radius(dm)
    half = half_mask(n, 7)
    flipped = half.copy()
    flipped[a >= K] = ~flipped[a >= K]
    masks = {"all-true bool": numpy.ones(n, bool), "all-true 255": numpy.full(n, 255, numpy.uint8), "clustered": a < K,
             "all-false": numpy.zeros(n, bool), "unclustered": a >= K, "half": half, "half, other flags on the rest": flipped,
             "half as 7s": half.astype(numpy.uint8) * 7}
    out = check_masked(x, c, a, q, [r, numpy.float32(0)], masks, dm=dm, env=env, expect=expect)
    for rr in (float(r), 0.0):
        base = out[(None, rr)][0]
        for name in ("all-true bool", "all-true 255", "clustered"):
            same(out[(name, rr)][0], base, name)
        for name in ("all-false", "unclustered"):
            got, stats = out[(name, rr)]
            assert (got[0] == 0).all() and got[1][-1] == 0 and stats["visited"] == 0 and stats["scored"] == 0
        for name in ("half, other flags on the rest", "half as 7s"):
            same(out[(name, rr)][0], out[("half", rr)][0], name)
        assert (out[("half", rr)][0][0][[1, 3, 5]] == 0).all()
    assert out[("half", float(r))][0][0].sum() > 0


# ----------------------------------------------------------------------------------------------------------------
# 6. prune soundness
# ----------------------------------------------------------------------------------------------------------------
_INNER = {}


def inner_mask(cs):
    """The rows at or below their cluster's median member distance: every radius shrinks."""
    if id(cs) not in _INNER:
        _INNER[id(cs)] = _inner_mask(cs)
    return _INNER[id(cs)]


def _inner_mask(cs):
    import oracle
    x32, c32 = cs.x.astype(numpy.float32), cs.c.astype(numpy.float32)
    member = numpy.array([oracle.distance(x32[i], c32[cs.a[i]], cs.metric) for i in range(len(x32))], numpy.float32)
    mask = numpy.zeros(len(x32), bool)
    for cl in range(len(c32)):
        rows = cs.a == cl
        if rows.any():
            mask[rows] = member[rows] <= numpy.median(member[rows])
    return mask


@pytest.mark.parametrize("env,expect", [({}, "f16"), ({"KMCUDA_AMD_KNN_EXACT": 1}, "exact")])
@pytest.mark.parametrize("corpus", ["moved_rows", "skewed"])
def test_the_prune_stays_sound(corpus, env, expect):
    cs = getattr(ri, corpus)()
    masks = {"inner": inner_mask(cs), "a third of the clusters denied": cs.a % 3 != 1}
    out = check_case(cs, ["wide"], masks, env=env, expect=expect)
    r = float(cs.r["wide"])
    from kmcuda_amd import KnnIndex
    with KnnIndex(cs.x, cs.c, cs.a) as ix:
        shrunk = ix.radii_allow(masks["inner"]) < ix.radii()
    assert shrunk.sum() >= len(cs.c) // 2              # the masked radii differ: the prune reads other numbers
    assert out[("inner", r)][1]["visited"] <= out[(None, r)][1]["visited"]


# ----------------------------------------------------------------------------------------------------------------
# 7. the index is left alone
# ----------------------------------------------------------------------------------------------------------------
def plain(ix, q, r, mask=None):
    res = ix.query_radius(q, r) if mask is None else ix.query_radius_allow(q, r, mask)
    counts = ix.query_radius(q, r, count_only=True) if mask is None else ix.query_radius_allow(q, r, mask, count_only=True)
    return (counts,) + tuple(res)


def test_after_add_and_after_remove():
    from kmcuda_amd import KnnIndex
    cs = ri.data_range(1.0, 64)
    x, c, a, q = cs.x, cs.c, cs.a, cs.q
    K, n, n0 = len(c), len(x), 1800
    r = cs.r["target"]
    removed = numpy.arange(0, n, 9)
    a_now = a.copy()
    with KnnIndex(x[:n0], c, a[:n0]) as ix:
        with pytest.raises(ValueError):
            ix.query_radius_allow(q, r, numpy.ones(n, bool))          # the mask follows n_rows
        ix.add(x[n0:], a[n0:])
        with pytest.raises(ValueError):
            ix.query_radius_allow(q, r, numpy.ones(n0, bool))
        mask = half_mask(n, 12)
        got = plain(ix, q, r, mask)
        with KnnIndex(x, c, patched(a_now, mask, K)) as fx:
            same(got, plain(fx, q, r), "after add")
        same(got, struck(plain(ix, q, r), mask), "after add, against the unmasked call")
        ix.remove(removed)
        a_now[removed] = K
        flipped = mask.copy()
        flipped[removed] = ~flipped[removed]                           # flags of removed rows are ignored
        with KnnIndex(x, c, patched(a_now, mask, K)) as fx:
            want = plain(fx, q, r)
        for m in (mask, flipped):
            got = plain(ix, q, r, m)
            same(got, want, "after remove")
            assert not numpy.isin(got[2], removed).any()
    allowed = cs.dm.copy()
    allowed[:, patched(a_now, mask, K) >= K] = numpy.nan
    same(want, expected(allowed, a_now, r), "after remove, against the oracle")


def test_two_masks_in_a_row_leave_the_index_untouched():
    from kmcuda_amd import KnnIndex
    cs = ri.data_range(1.0, 64)
    q, r, n = cs.q, cs.r["wide"], len(cs.x)
    m1, m2 = half_mask(n, 13), half_mask(n, 14, 0.1)
    with KnnIndex(cs.x, cs.c, cs.a) as ix:
        before = plain(ix, q, r) + (ix.radii(), numpy.array(ix.info()))
        r1 = plain(ix, q, r, m1)
        r2 = plain(ix, q, r, m2)
        r1_again = plain(ix, q, r, m1)
        after = plain(ix, q, r) + (ix.radii(), numpy.array(ix.info()))
    for u, v in zip(after, before):
        assert (u.view(numpy.uint32) == v.view(numpy.uint32)).all() if u.dtype == numpy.float32 else (u == v).all()
    same(r1_again, r1, "the first mask again")
    same(r1, struck(before[:4], m1), "the first mask")
    same(r2, struck(before[:4], m2), "the second mask")
    assert r1[1][-1] != r2[1][-1]


# ----------------------------------------------------------------------------------------------------------------
# 8. chunking, 9. device masks
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"KMCUDA_AMD_KNN_EXACT": "1"}])
def test_chunking(env, monkeypatch):
    from kmcuda_amd import KnnIndex
    cs = ri.data_range(1.0, 64)
    q = cs.q[:130].copy()
    q[100, 3] = numpy.nan
    r, mask = cs.r["wide"], half_mask(len(cs.x), 15)
    dev = torch.device("cuda", 0)
    tq, tm = torch.from_numpy(q).to(dev), torch.from_numpy(mask).to(dev)
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    with KnnIndex(cs.x, cs.c, cs.a) as ix:
        want = plain(ix, q, r, mask)
        same(want, struck(plain(ix, q, r), mask), "one chunk")
        for chunk in ("1", "37", "1000"):
            monkeypatch.setenv("KMCUDA_AMD_KNN_QUERY_CHUNK", chunk)
            same(plain(ix, q, r, mask), want, "chunks of %s, host buffers" % chunk)
            same(tuple(host(v) for v in plain(ix, tq, r, tm)), want, "chunks of %s, device buffers" % chunk)
    assert want[0][100] == 0 and want[1][-1] > 0


def test_device_resident_masks():
    from kmcuda_amd import KnnIndex
    cs = ri.data_range(1.0, 64)
    q, r, n = cs.q, cs.r["target"], len(cs.x)
    mask = half_mask(n, 16)
    dev = torch.device("cuda", 0)
    tq = torch.from_numpy(q.copy()).to(dev)
    with KnnIndex(cs.x, cs.c, cs.a) as ix:
        want = plain(ix, q, r, mask)
        for tm in (torch.from_numpy(mask).to(dev), torch.from_numpy(mask.astype(numpy.uint8) * 200).to(dev),
                   torch.from_numpy(numpy.repeat(mask, 2)).to(dev)[::2]):
            for _ in range(2):
                got = plain(ix, tq, r, tm)
                assert all(t.is_cuda for t in got)
                same(tuple(host(v) for v in got), want, "device-resident %s mask" % tm.dtype)
        with pytest.raises(TypeError):
            ix.query_radius_allow(tq, r, mask)
        with pytest.raises(TypeError):
            ix.query_radius_allow(q, r, torch.from_numpy(mask).to(dev))
        with pytest.raises(ValueError):
            ix.query_radius_allow(tq, r, torch.from_numpy(mask))       # a tensor in host memory
    from kmcuda_amd import knn_query_radius
    same((want[0],), (knn_query_radius(r, cs.x, cs.c, cs.a, q, allow=mask, count_only=True),), "knn_query_radius")
    same(want[1:], knn_query_radius(r, cs.x, cs.c, cs.a, q, allow=mask), "knn_query_radius")


# ----------------------------------------------------------------------------------------------------------------
# 10. wrong query clusters
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,d", [("L2", 64), ("angular", 64), ("L2", 1152)])
def test_query_assignments_do_not_matter(metric, d):
    from kmcuda_amd import KnnIndex
    x, c, a, q, dm = ri.truth(2000, d, metric)
    r = ri.target_radius(dm) if metric == "L2" else ri.gap_radius(dm, ri.target_radius(dm))
    mask = half_mask(2000, 17)
    finite = numpy.nonzero(numpy.isfinite(c).all(axis=1))[0]
    rng = numpy.random.default_rng(2)
    with KnnIndex(x, c, a, metric=metric) as ix:
        base = plain(ix, q, r, mask)
        same(base, struck(plain(ix, q, r), mask), "computed clusters")
        for qa in (numpy.full(len(q), finite[0], numpy.uint32), finite[rng.integers(0, len(finite), len(q))].astype(numpy.uint32)):
            got = (ix.query_radius_allow(q, r, mask, query_assignments=qa, count_only=True),) + \
                ix.query_radius_allow(q, r, mask, query_assignments=qa)
            same(got, base, "wrong query clusters")
    assert base[1][-1] > 0


# ----------------------------------------------------------------------------------------------------------------
# 11. the C contract
# ----------------------------------------------------------------------------------------------------------------
def test_c_contract():
    from kmcuda_amd import KnnIndex
    cs = ri.data_range(1.0, 64)
    x, c, a, q, dm = cs.x, cs.c, cs.a, cs.q, cs.dm
    r, n, nq = cs.r["wide"], len(cs.x), len(cs.q)
    A = half_mask(n, 18)
    B = A & half_mask(n, 19)                                        # a strict subset
    ua, ub = A.astype(numpy.uint8), B.astype(numpy.uint8)

    def truth_of(mask):
        allowed = dm.copy()
        allowed[:, ~mask] = numpy.nan
        return expected(allowed, a, r)
    counts_a, off_a, nb_a, dist_a = truth_of(A)
    counts_b, _, nb_b, dist_b = truth_of(B)
    assert (counts_b < counts_a).any()
    total = int(off_a[-1])
    vp = lambda v: ctypes.c_void_p(v.ctypes.data) if v is not None else None   # noqa: E731
    f32 = ctypes.c_float
    SENT_I, SENT_F = 0xABCD1234, numpy.float32(-77.5)
    lead = 7
    offs = (off_a + lead).astype(numpy.uint64)

    def buffers():
        return numpy.full(total + lead + 16, SENT_I, numpy.uint32), numpy.full(total + lead + 16, SENT_F, numpy.float32)

    with KnnIndex(x, c, a) as ix:
        L = ix.lib
        counts = numpy.full(nq, 77, numpy.uint32)
        assert L.kmamd_knn_index_radius_count_allow(ix.h, f32(r), nq, vp(q), None, vp(counts), None, -1, vp(ua)) == 0
        assert (counts == counts_a).all()
        nb, dist = buffers()
        assert L.kmamd_knn_index_radius_fill_allow(ix.h, f32(r), nq, vp(q), None, vp(offs), vp(nb), vp(dist), -1, vp(ua)) == 0
        assert (nb[lead:lead + total] == nb_a).all() and (dist[lead:lead + total].view(numpy.uint32) == dist_a.view(numpy.uint32)).all()
        assert (nb[:lead] == SENT_I).all() and (nb[lead + total:] == SENT_I).all()
        assert (dist[:lead] == SENT_F).all() and (dist[lead + total:] == SENT_F).all()
        # a count under A, a fill under B: refused after the search, every range holds the head of ITS query's hits
        nb, dist = buffers()
        assert L.kmamd_knn_index_radius_fill_allow(ix.h, f32(r), nq, vp(q), None, vp(offs), vp(nb), vp(dist), -1, vp(ub)) == 1
        assert (nb[:lead] == SENT_I).all() and (nb[lead + total:] == SENT_I).all()
        assert (dist[:lead] == SENT_F).all() and (dist[lead + total:] == SENT_F).all()
        ob = numpy.concatenate([[0], numpy.cumsum(counts_b)]).astype(numpy.int64)
        for i in range(nq):
            lo, m = int(offs[i]), int(counts_b[i])
            assert (nb[lo:lo + m] == nb_b[ob[i]:ob[i + 1]]).all() and (dist[lo:lo + m] == dist_b[ob[i]:ob[i + 1]]).all(), i
        # ... and the other way round (more hits than the range): nothing behind a query's own range
        offs_b = (ob + lead).astype(numpy.uint64)
        nb, dist = buffers()
        assert L.kmamd_knn_index_radius_fill_allow(ix.h, f32(r), nq, vp(q), None, vp(offs_b), vp(nb), vp(dist), -1, vp(ua)) == 1
        assert (nb[:lead] == SENT_I).all() and (nb[int(offs_b[-1]):] == SENT_I).all() and (dist[int(offs_b[-1]):] == SENT_F).all()
        for i in range(nq):
            lo, m = int(offs_b[i]), int(counts_b[i])
            assert (nb[lo:lo + m] == nb_a[off_a[i]:off_a[i] + m]).all(), i
        # decreasing offsets: refused before any write (and before the mask is looked at)
        bad = offs.copy()
        i = int(numpy.nonzero(counts_a)[0][0])
        bad[i], bad[i + 1] = bad[i + 1], bad[i]
        assert bad[i] > bad[i + 1]
        nb, dist = buffers()
        assert L.kmamd_knn_index_radius_fill_allow(ix.h, f32(r), nq, vp(q), None, vp(bad), vp(nb), vp(dist), -1, vp(ua)) == 1
        assert (nb == SENT_I).all() and (dist == SENT_F).all()
        # no row allowed: all-equal offsets succeed and write nothing
        zeros = numpy.zeros(n, numpy.uint8)
        flat = numpy.full(nq + 1, lead, numpy.uint64)
        assert L.kmamd_knn_index_radius_count_allow(ix.h, f32(r), nq, vp(q), None, vp(counts), None, -1, vp(zeros)) == 0
        assert (counts == 0).all()
        assert L.kmamd_knn_index_radius_fill_allow(ix.h, f32(r), nq, vp(q), None, vp(flat), vp(nb), vp(dist), -1, vp(zeros)) == 0
        assert (nb == SENT_I).all() and (dist == SENT_F).all()
        # the unmasked call's refusals, in its order; another device; no queries
        other = ix.device + 1
        counts[:] = 77
        assert L.kmamd_knn_index_radius_count_allow(ix.h, f32(r), nq, vp(q), None, vp(counts), None, other, vp(ua)) == 1
        assert L.kmamd_knn_index_radius_fill_allow(ix.h, f32(r), nq, vp(q), None, vp(offs), vp(nb), vp(dist), other, vp(ua)) == 1
        for radius in (-1.0, float("nan"), float("inf")):
            assert L.kmamd_knn_index_radius_count_allow(ix.h, f32(radius), nq, vp(q), None, vp(counts), None, -1, vp(ua)) == 1
            assert L.kmamd_knn_index_radius_fill_allow(ix.h, f32(radius), nq, vp(q), None, vp(offs), vp(nb), vp(dist), -1, vp(ua)) == 1
        assert L.kmamd_knn_index_radius_count_allow(ix.h, f32(r), nq, None, None, vp(counts), None, -1, vp(ua)) == 1
        assert L.kmamd_knn_index_radius_count_allow(ix.h, f32(r), nq, vp(q), None, None, None, -1, vp(ua)) == 1
        assert L.kmamd_knn_index_radius_fill_allow(ix.h, f32(r), nq, vp(q), None, None, vp(nb), vp(dist), -1, vp(ua)) == 1
        assert L.kmamd_knn_index_radius_fill_allow(ix.h, f32(r), nq, vp(q), None, vp(offs), None, None, -1, vp(ua)) == 1
        assert L.kmamd_knn_index_radius_count_allow(ix.h, f32(r), 0, None, None, None, None, -1, vp(ua)) == 0
        assert L.kmamd_knn_index_radius_fill_allow(ix.h, f32(r), 0, None, None, None, None, None, -1, vp(ua)) == 0
        assert (counts == 77).all() and (nb == SENT_I).all() and (dist == SENT_F).all()
        # allow == NULL is the unmasked call
        ecounts, eoff, enb, edist = expected(dm, a, r)
        assert L.kmamd_knn_index_radius_count_allow(ix.h, f32(r), nq, vp(q), None, vp(counts), None, -1, None) == 0
        assert (counts == ecounts).all()
        nb = numpy.full(int(eoff[-1]) + 16, SENT_I, numpy.uint32)
        dist = numpy.full(int(eoff[-1]) + 16, SENT_F, numpy.float32)
        u64 = eoff.astype(numpy.uint64)
        assert L.kmamd_knn_index_radius_fill_allow(ix.h, f32(r), nq, vp(q), None, vp(u64), vp(nb), vp(dist), -1, None) == 0
        same((nb[:int(eoff[-1])], dist[:int(eoff[-1])]), (enb, edist), "allow == NULL")
        assert (nb[int(eoff[-1]):] == SENT_I).all()
        # device buffers and a device mask: the subset fill again, where the caller's slots really lie next to the ranges
        dev = torch.device("cuda", 0)
        tq, tb = torch.from_numpy(q.copy()).to(dev), torch.from_numpy(ub).to(dev)
        toff = torch.from_numpy(offs.astype(numpy.int64)).to(dev)
        tnb = torch.full((total + lead + 16,), 0x2BCD1234, dtype=torch.int32, device=dev)
        tdist = torch.full((total + lead + 16,), float(SENT_F), dtype=torch.float32, device=dev)
        dp = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
        assert L.kmamd_knn_index_radius_fill_allow(ix.h, f32(r), nq, dp(tq), None, dp(toff), dp(tnb), dp(tdist), 0, dp(tb)) == 1
        hnb, hdist = tnb.cpu().numpy().view(numpy.uint32), tdist.cpu().numpy()
        assert (hnb[:lead] == 0x2BCD1234).all() and (hnb[lead + total:] == 0x2BCD1234).all()
        assert (hdist[:lead] == SENT_F).all() and (hdist[lead + total:] == SENT_F).all()
        for i in range(nq):
            lo, m = int(offs[i]), int(counts_b[i])
            assert (hnb[lo:lo + m] == nb_b[ob[i]:ob[i + 1]]).all(), i
