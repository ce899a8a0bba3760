"""The allow-mask of the k-NN index queries (KnnIndex.query(allow=); knn_mask.hip and the MASK
instantiations of knn_f16.hip / knn.hip) on the device.

A masked call must return what the same call returns on the index KnnIndex builds from the same rows and centroids with
the assignments of every denied row set to K.  "Equal" below means identical neighbour arrays and identical distance BIT
PATTERNS (NaN equals NaN), for query(k=7) and query(k=7, nprobe=3) -- against that fresh index under both metrics, and
under L2 also against the CPU oracle (oracle.knn_query / tests/_probe_ref.probe_reference on the patched assignments);
under the angular metric the oracle comparison has the allowance of tests/_angular.py and nothing wider.

1. every masked f16 instantiation  2. every route to the masked exact kernel  3. bit and tile edges, built through the
sorted order  4. all-true, all-false, non-finite queries  5. the masked radii  6. add / remove / two masks in a row
7. chunking  8. device-resident masks  9. a refusal that needs a device."""
import ctypes

import numpy
import pytest

import oracle
from _angular import assert_knn_only_acos_matters
from _probe_ref import EXACT, FLT_MAX, NONE, probe_reference
from test_gpu_knn_edges import sized
from test_gpu_knn_probe import cached, corpus, fresh, nearest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K7, P3 = 7, 3


def bits(d):
    d = numpy.ascontiguousarray(d)
    if d.dtype != numpy.float32:
        return d
    return numpy.where(numpy.isnan(d), numpy.uint32(0x7FC00000), d.view(numpy.uint32))


def same(got, want, what):
    for g, w in zip(got, want):
        g, w = bits(g), bits(w)
        assert g.shape == w.shape, what
        bad = numpy.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
        assert bad.size == 0, "%s: %d rows differ, first %d: %s against %s" % (what, bad.size, bad[0], g[bad[0]], w[bad[0]])


def patched(a, mask, K):
    return numpy.where(numpy.asarray(mask) != 0, a, K).astype(numpy.uint32)


def half_mask(n, seed=0, p=0.5):
    return numpy.random.RandomState(seed).rand(n) < p


def sorted_order(a, K):
    """Sorted position -> row id, as the index orders a fresh corpus."""
    return numpy.argsort(numpy.minimum(a, K), kind="stable")


def listen():
    from test_gpu_kmeans import StdoutListener
    return StdoutListener()


def against_oracle(metric, x, q, got, ref, what):
    """L2 / half2: the oracle's bits.  Angular: the allowance of tests/_angular.py for the lists, fillers and NaN rows in
    the same places, every real distance within 2 ulp of the oracle's distance to the row returned."""
    nb, dist = got
    ref_nb, ref_dist = ref
    if metric == "L2":
        same(got, ref, what + " against the oracle")
        return
    x32, q32 = x.astype(numpy.float32), q.astype(numpy.float32)
    has = ~numpy.isnan(ref_dist).all(axis=1)
    assert (nb[~has] == NONE).all() and numpy.isnan(dist[~has]).all(), what
    allowed = assert_knn_only_acos_matters(x32, nb[has], ref_nb[has], what, queries=q32[has])
    print("angular allowance: %d of %d rows (%s)" % (allowed, len(q), what))
    filler = ref_dist == FLT_MAX
    assert (filler == (dist == FLT_MAX)).all() and (nb[filler] == 0).all(), what
    assert (numpy.isnan(dist) == numpy.isnan(ref_dist)).all(), what
    for i, j in zip(*numpy.nonzero(~filler & ~numpy.isnan(ref_dist))):
        want = numpy.float32(oracle.distance(q32[i], x32[nb[i, j]], metric=oracle.COS))
        assert abs(dist[i, j] - want) <= 2 * numpy.spacing(max(dist[i, j], want)), (what, i, j, dist[i, j], want)


def check_allow(x, c, a, q, mask, metric="L2", env=None, expect=None, monkeypatch=None, half2=False, k=K7, p=P3,
                given=False, with_oracle=True, what=""):
    """query(k, allow=mask) and query(k, nprobe=p, allow=mask) on KnnIndex(x, c, a) equal the unmasked calls on
    KnnIndex(x, c, patched a), and the oracle on the patched assignments.  expect: "f16" or "exact", the search that
    must have run, read from what verbosity 1 prints.  given: the caller passes the queries' clusters and probe lists
    (the half2 arithmetic has no pass that computes them).  Returns the masked call's (neighbors, distances)."""
    from kmcuda_amd import KnnIndex
    for key, v in (env or {}).items():
        monkeypatch.setenv(key, str(v))
    K = len(c)
    a = numpy.ascontiguousarray(a, dtype=numpy.uint32)
    mask = numpy.asarray(mask)
    ap = patched(a, mask, K)
    p = min(p, K)
    qa_in = probes_in = None
    if given:
        probes_in = nearest(q.astype(numpy.float32), c.astype(numpy.float32), p)
        qa_in = numpy.ascontiguousarray(probes_in[:, 0])
    what = "%s %s D=%d K=%d %s allowed %d of %d" % (what, metric, x.shape[1], K, env, int((mask != 0).sum()), len(x))
    out = listen()
    with out:
        with KnnIndex(x, c, a, metric=metric, verbosity=1) as ix:
            plain = ix.query(q, k, query_assignments=qa_in)
            nb, dist, qa = ix.query(q, k, query_assignments=qa_in, return_assignments=True, allow=mask)
            pnb, pdist, used = ix.query(q, k, nprobe=None if given else p, probes=probes_in, return_probes=True, allow=mask)
            again = ix.query(q, k, query_assignments=qa_in)
    text = out.text
    same(again, plain, what + ": the unmasked call after the masked ones")
    with KnnIndex(x, c, ap, metric=metric) as fx:
        want = fx.query(q, k, query_assignments=qa_in, return_assignments=True)
        pwant = fx.query(q, k, nprobe=None if given else p, probes=probes_in, return_probes=True)
    same((nb, dist, qa), want, what + " query against the fresh index")
    same((pnb, pdist, used), pwant, what + " probed query against the fresh index")
    denied = numpy.nonzero(ap >= K)[0]
    for found, d in ((nb, dist), (pnb, pdist)):
        real = d < FLT_MAX
        assert not numpy.isin(found[real], denied).any(), what + ": a denied row was returned"
    if with_oracle:
        xo, co, qo = (x, c, q) if half2 else (v.astype(numpy.float32) for v in (x, c, q))
        against_oracle(metric, x, q, (nb, dist),
                       oracle.knn_query(k, xo, co, ap, qo, query_assignments=qa, metric=metric, half2=half2), what)
        against_oracle(metric, x, q, (pnb, pdist), probe_reference(k, xo, co, ap, qo, used, metric=metric, half2=half2),
                       what + " probed")
    if expect is not None:
        assert expect in ("f16", "exact")
        assert (EXACT in text) == (expect == "exact"), text
    return nb, dist


# ----------------------------------------------------------------------------------------------------------------
# 1. every masked f16 instantiation
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "cos"])
@pytest.mark.parametrize("d", [10, 32, 64, 100, 256, 300, 768, 1000])
def test_every_masked_f16_instantiation(d, metric, monkeypatch):
    n, nq = (2000, 150) if d <= 256 else (1200, 90)
    x, c, a = cached(("inst", d, metric), lambda: corpus(n, d, 24, 300 + d, metric))
    q = fresh(c, nq, d, metric=metric)
    check_allow(x, c, a, q, half_mask(n, d), metric=metric, expect="f16", monkeypatch=monkeypatch)


@pytest.mark.parametrize("metric", ["L2", "cos"])
@pytest.mark.parametrize("d", [64, 256])
def test_half_rows(d, metric, monkeypatch):
    x, c, a = cached(("half", d, metric), lambda: corpus(2000, d, 24, 400 + d, metric, half=True))
    q = fresh(c, 150, d + 1, metric=metric)
    check_allow(x, c, a, q, half_mask(2000, d + 1), metric=metric, expect="f16", monkeypatch=monkeypatch)


# ----------------------------------------------------------------------------------------------------------------
# 2. the routes to the masked exact kernel
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "cos"])
@pytest.mark.parametrize("env", [{"KMCUDA_AMD_KNN_EXACT": 1}, {"KMCUDA_AMD_FILTER": "f32"}])
def test_exact_paths(env, metric, monkeypatch):
    x, c, a = cached(("paths", metric), lambda: corpus(2000, 64, 24, 1400, metric))
    q = fresh(c, 120, 11, metric=metric)
    check_allow(x, c, a, q, half_mask(2000, 2), metric=metric, env=env, expect="exact", monkeypatch=monkeypatch)


def test_half2_arithmetic(monkeypatch):
    x, c, a = cached(("half", 64, "L2"), lambda: corpus(2000, 64, 24, 464, "L2", half=True))
    q = fresh(c, 100, 14)
    check_allow(x, c, a, q, half_mask(2000, 3), env={"KMCUDA_AMD_FP16_STRICT": 1}, expect="exact", half2=True, given=True,
                monkeypatch=monkeypatch)


def test_wide_rows(monkeypatch):
    x, c, a = cached(("wide",), lambda: corpus(800, 1100, 12, 1500))
    q = fresh(c, 60, 12)
    check_allow(x, c, a, q, half_mask(800, 4), expect="exact", monkeypatch=monkeypatch)


@pytest.mark.parametrize("d", [64, 512])
def test_an_index_beyond_the_half_range(d, monkeypatch):
    x, c, a = cached(("range", d), lambda: corpus(1500, d, 24, 1600 + d))
    q = fresh(c, 100, 13)
    x2 = x.copy()
    x2[11] += 2e5                                   # (it keeps its cluster: legal, the radius grows)
    for allowed_11 in (True, False):
        mask = half_mask(1500, 5)
        mask[11] = allowed_11
        check_allow(x2, c, a, q, mask, expect="exact", monkeypatch=monkeypatch)


# ----------------------------------------------------------------------------------------------------------------
# 3. bit and tile edges
# ----------------------------------------------------------------------------------------------------------------
SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 200, 0, 130, 5]


def edge_masks(a, K):
    """name -> mask, built through the sorted order of the corpus."""
    n = len(a)
    order = sorted_order(a, K)
    offsets = numpy.concatenate([[0], numpy.cumsum(numpy.bincount(a, minlength=K)[:K])])
    masks = {}
    for p in (31, 32, 33, 63, 64, 65):
        m = numpy.zeros(n, bool)
        m[order[p]] = True
        masks["position %d alone" % p] = m
    first, last = numpy.zeros(n, bool), numpy.zeros(n, bool)
    for cl in range(K):
        if offsets[cl + 1] > offsets[cl]:
            first[order[offsets[cl]]] = True
            last[order[offsets[cl + 1] - 1]] = True
    masks["the first row of every cluster"] = first
    masks["the last row of every cluster"] = last
    second = numpy.zeros(n, bool)
    second[order[::2]] = True
    masks["every second position"] = second
    but_one = numpy.ones(n, bool)
    but_one[order[64]] = False
    masks["everything but one row"] = but_one
    return masks


@pytest.mark.parametrize("env,expect", [({}, "f16"), ({"KMCUDA_AMD_KNN_EXACT": 1}, "exact")])
@pytest.mark.parametrize("d", [16, 64, 300])
def test_bit_and_tile_edges(d, env, expect, monkeypatch):
    x, c, a = cached(("sizes", d), lambda: sized(SIZES, d, seed=500 + d))
    q = fresh(c, 200, d + 2, sigma=0.12)
    K = len(SIZES)
    for name, mask in edge_masks(a, K).items():
        nb, dist = check_allow(x, c, a, q, mask, env=env, expect=expect, monkeypatch=monkeypatch, what=name)
        if name.endswith("alone"):   # exactly one row of the corpus: slot 0 holds it, the rest the filler
            row = numpy.nonzero(mask)[0][0]
            assert (nb[:, 0] == row).all() and (nb[:, 1:] == 0).all() and (dist[:, 1:] == FLT_MAX).all()


@pytest.mark.parametrize("env,expect", [({}, "f16"), ({"KMCUDA_AMD_KNN_EXACT": 1}, "exact")])
def test_a_cluster_denied_the_own_cluster_of_some_queries_included(env, expect, monkeypatch):
    x, c, a = cached(("sizes", 64), lambda: sized(SIZES, 64, seed=564))
    K = len(SIZES)
    q = fresh(c, 200, 66, sigma=0.12)
    own, _, _ = oracle.lloyd_assign(q, c)
    for cl in (8, 10):                               # the two largest: many queries live there
        assert (own == cl).sum() > 5
        mask = a != cl
        nb, dist = check_allow(x, c, a, q, mask, env=env, expect=expect, monkeypatch=monkeypatch, what="cluster %d denied" % cl)
        assert not (a[nb[dist < FLT_MAX]] == cl).any()


@pytest.mark.parametrize("env,expect", [({}, "f16"), ({"KMCUDA_AMD_KNN_EXACT": 1}, "exact")])
def test_fewer_allowed_rows_than_k(env, expect, monkeypatch):
    x, c, a = cached(("sizes", 64), lambda: sized(SIZES, 64, seed=564))
    q = fresh(c, 200, 67, sigma=0.12)
    order = sorted_order(a, len(SIZES))
    mask = numpy.zeros(len(a), bool)
    mask[order[[2, 40, 300, 500]]] = True
    nb, dist = check_allow(x, c, a, q, mask, env=env, expect=expect, monkeypatch=monkeypatch, p=len(SIZES))
    assert (dist[:, :4] < FLT_MAX).all() and (dist[:, 4:] == FLT_MAX).all() and (nb[:, 4:] == 0).all()
    assert (numpy.sort(nb[:, :4], axis=1) == numpy.sort(order[[2, 40, 300, 500]])).all()


@pytest.mark.parametrize("env,expect", [({}, "f16"), ({"KMCUDA_AMD_KNN_EXACT": 1}, "exact")])
def test_k_equal_to_n_rows(env, expect, monkeypatch):
    x, c, a = cached(("kn",), lambda: corpus(300, 32, 6, 2100))
    q = fresh(c, 40, 21)
    mask = half_mask(300, 6)
    nb, dist = check_allow(x, c, a, q, mask, env=env, expect=expect, monkeypatch=monkeypatch, k=300, p=6)
    n_allowed = int(mask.sum())
    assert (dist[:, :n_allowed] < FLT_MAX).all() and (dist[:, n_allowed:] == FLT_MAX).all()
    assert (numpy.sort(nb[:, :n_allowed], axis=1) == numpy.nonzero(mask)[0]).all()


@pytest.mark.parametrize("env,expect", [({}, "f16"), ({"KMCUDA_AMD_KNN_EXACT": 1}, "exact")])
def test_one_cluster(env, expect, monkeypatch):
    x, c, a = cached(("small", 1), lambda: corpus(600, 32, 1, 901))
    q = fresh(c, 100, 5)
    check_allow(x, c, a, q, half_mask(600, 7), env=env, expect=expect, monkeypatch=monkeypatch)
    one = numpy.zeros(600, bool)
    one[417] = True
    nb, dist = check_allow(x, c, a, q, one, env=env, expect=expect, monkeypatch=monkeypatch)
    assert (nb[:, 0] == 417).all() and (dist[:, 1:] == FLT_MAX).all()


# ----------------------------------------------------------------------------------------------------------------
# 4. all-true, all-false, non-finite queries
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,expect", [({}, "f16"), ({"KMCUDA_AMD_KNN_EXACT": 1}, "exact")])
def test_all_true_all_false_and_non_finite_queries(env, expect, monkeypatch):
    from kmcuda_amd import KnnIndex
    x, c, a = cached(("nonfinite",), lambda: corpus(2000, 64, 24, 1300))
    a = a.copy()
    a[::97] = 24                                    # rows without a cluster: their flags are ignored
    q = fresh(c, 120, 10)
    q[3, 0] = numpy.nan
    q[77, 5] = numpy.inf
    q[78, 63] = -numpy.inf
    bad = numpy.array([3, 77, 78])
    fin = numpy.setdiff1d(numpy.arange(len(q)), bad)
    for key, v in env.items():
        monkeypatch.setenv(key, str(v))
    with KnnIndex(x, c, a) as ix:
        plain = ix.query(q, K7)
        pplain = ix.query(q, K7, nprobe=P3)
        for ones in (numpy.ones(2000, bool), numpy.full(2000, 255, numpy.uint8), (a < 24)):
            same(ix.query(q, K7, allow=ones), plain, "every flag set")
            same(ix.query(q, K7, nprobe=P3, allow=ones), pplain, "every flag set, probed")
        for zeros in (numpy.zeros(2000, bool), (a >= 24)):
            for nb, dist in (ix.query(q, K7, allow=zeros), ix.query(q, K7, nprobe=P3, allow=zeros)):
                assert (nb[fin] == 0).all() and (dist[fin] == FLT_MAX).all()
                assert (nb[bad] == NONE).all() and numpy.isnan(dist[bad]).all()
    nb, dist = check_allow(x, c, a, q, half_mask(2000, 8), env=env, expect=expect, monkeypatch=monkeypatch)
    assert (nb[bad] == NONE).all() and numpy.isnan(dist[bad]).all()


# ----------------------------------------------------------------------------------------------------------------
# 5. the masked radii
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,d,half", [("L2", 64, False), ("L2", 100, False), ("cos", 64, False), ("L2", 64, True)])
def test_masked_radii(metric, d, half):
    from kmcuda_amd import KnnIndex
    x, c, a = cached(("radii", metric, d, half), lambda: corpus(2000, d, 24, 2200 + d, metric, half=half))
    masks = [half_mask(2000, 9), half_mask(2000, 10, 0.02), numpy.ones(2000, bool)]
    emptied = half_mask(2000, 11)
    emptied[a == 5] = False
    masks.append(emptied)
    with KnnIndex(x, c, a, metric=metric) as ix:
        own = ix.radii()
        assert numpy.isnan(ix.radii_allow(numpy.zeros(2000, bool))).all()
        for mask in masks:
            got = ix.radii_allow(mask)
            got_u8 = ix.radii_allow(mask.astype(numpy.uint8) * 3)
            got_dev = ix.radii_allow(torch.from_numpy(mask).to(torch.device("cuda", 0)))
            with KnnIndex(x, c, patched(a, mask, 24), metric=metric) as fx:
                want = fx.radii()
            same((got, got_u8, got_dev), (want, want, want), "radii %s d=%d allowed %d" % (metric, d, mask.sum()))
            # over fewer rows a radius can only shrink (NaN: the cluster has no allowed row)
            assert ((got <= own) | numpy.isnan(got)).all()
        assert numpy.isnan(ix.radii_allow(emptied)[5]) and not numpy.isnan(own[5])
        same((ix.radii(),), (own,), "the index's own radii afterwards")


# ----------------------------------------------------------------------------------------------------------------
# 6. composition
# ----------------------------------------------------------------------------------------------------------------
def test_after_add_and_after_remove():
    from kmcuda_amd import KnnIndex
    x, c, a = cached(("compose",), lambda: corpus(2000, 64, 24, 2300))
    q = fresh(c, 150, 23)
    n0 = 1500
    removed = numpy.arange(0, 2000, 9)
    a_now = a.copy()
    with KnnIndex(x[:n0], c, a[:n0]) as ix:
        with pytest.raises(ValueError):
            ix.query(q, K7, allow=numpy.ones(2000, bool))          # the mask follows n_rows
        ix.add(x[n0:], a[n0:])
        with pytest.raises(ValueError):
            ix.query(q, K7, allow=numpy.ones(n0, bool))
        mask = half_mask(2000, 12)
        got = ix.query(q, K7, allow=mask), ix.query(q, K7, nprobe=P3, allow=mask)
        with KnnIndex(x, c, patched(a_now, mask, 24)) as fx:
            want = fx.query(q, K7), fx.query(q, K7, nprobe=P3)
        same(got[0] + got[1], want[0] + want[1], "after add")
        ix.remove(removed)
        a_now[removed] = 24
        flipped = mask.copy()
        flipped[removed] = ~flipped[removed]                       # flags of removed rows are ignored
        with KnnIndex(x, c, patched(a_now, mask, 24)) as fx:
            want = fx.query(q, K7), fx.query(q, K7, nprobe=P3)
            want_r = fx.radii()
        for m in (mask, flipped):
            got = ix.query(q, K7, allow=m), ix.query(q, K7, nprobe=P3, allow=m)
            same(got[0] + got[1], want[0] + want[1], "after remove")
            same((ix.radii_allow(m),), (want_r,), "masked radii after remove")
            assert not numpy.isin(got[0][0][got[0][1] < FLT_MAX], removed).any()


def test_two_masks_in_a_row_leave_the_index_untouched():
    from kmcuda_amd import KnnIndex
    x, c, a = cached(("compose",), lambda: corpus(2000, 64, 24, 2300))
    q = fresh(c, 150, 24)
    m1, m2 = half_mask(2000, 13), half_mask(2000, 14, 0.1)
    with KnnIndex(x, c, a) as ix:
        before = ix.query(q, K7) + ix.query(q, K7, nprobe=P3) + (ix.radii(), numpy.array(ix.info()))
        r1 = ix.query(q, K7, allow=m1) + ix.query(q, K7, nprobe=P3, allow=m1)
        r2 = ix.query(q, K7, allow=m2) + ix.query(q, K7, nprobe=P3, allow=m2)
        r1_again = ix.query(q, K7, allow=m1) + ix.query(q, K7, nprobe=P3, allow=m1)
        after = ix.query(q, K7) + ix.query(q, K7, nprobe=P3) + (ix.radii(), numpy.array(ix.info()))
    same(after, before, "the unmasked calls after two masks")
    same(r1_again, r1, "the first mask again")
    for m, r in ((m1, r1), (m2, r2)):
        with KnnIndex(x, c, patched(a, m, 24)) as fx:
            same(r, fx.query(q, K7) + fx.query(q, K7, nprobe=P3), "one mask after the other")
    assert (r1[0] != r2[0]).any()


# ----------------------------------------------------------------------------------------------------------------
# 7. chunking
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"KMCUDA_AMD_KNN_EXACT": "1"}])
def test_chunking(env, monkeypatch):
    from kmcuda_amd import KnnIndex
    x, c, a = cached(("chunks",), lambda: corpus(2500, 64, 24, 1700))
    q = fresh(c, 300, 15)
    q[100, 3] = numpy.nan
    mask = half_mask(2500, 15)
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    with KnnIndex(x, c, a) as ix:
        want = ix.query(q, K7, allow=mask) + ix.query(q, K7, nprobe=P3, allow=mask)
        for chunk in ("1", "37", "1000"):
            monkeypatch.setenv("KMCUDA_AMD_KNN_QUERY_CHUNK", chunk)
            same(ix.query(q, K7, allow=mask) + ix.query(q, K7, nprobe=P3, allow=mask), want, "chunks of " + chunk)
        monkeypatch.delenv("KMCUDA_AMD_KNN_QUERY_CHUNK")
    with KnnIndex(x, c, patched(a, mask, 24)) as fx:
        same(want, fx.query(q, K7) + fx.query(q, K7, nprobe=P3), "chunked against the fresh index")


# ----------------------------------------------------------------------------------------------------------------
# 8. device-resident mask and queries
# ----------------------------------------------------------------------------------------------------------------
def test_device_resident_mask_and_queries():
    from kmcuda_amd import KnnIndex
    x, c, a = cached(("chunks",), lambda: corpus(2500, 64, 24, 1700))
    q = fresh(c, 300, 16)
    mask = half_mask(2500, 16)
    dev = torch.device("cuda", 0)
    tq = torch.from_numpy(q).to(dev)

    def host(res):
        return tuple(r.cpu().numpy().view(numpy.uint32) if r.dtype == torch.int32 else r.cpu().numpy() for r in res)

    with KnnIndex(x, c, a) as ix:
        want = ix.query(q, K7, return_assignments=True, allow=mask) + ix.query(q, K7, nprobe=P3, return_probes=True, allow=mask)
        for tm in (torch.from_numpy(mask).to(dev), torch.from_numpy(mask.astype(numpy.uint8) * 200).to(dev),
                   torch.from_numpy(numpy.repeat(mask, 2)).to(dev)[::2]):
            for _ in range(2):   # two identical calls, identical bits
                got = host(ix.query(tq, K7, return_assignments=True, allow=tm) +
                           ix.query(tq, K7, nprobe=P3, return_probes=True, allow=tm))
                same(got, want, "device-resident %s mask" % tm.dtype)
        # the other side, either way round
        with pytest.raises(TypeError):
            ix.query(tq, K7, allow=mask)
        with pytest.raises(TypeError):
            ix.query(q, K7, allow=torch.from_numpy(mask).to(dev))
        with pytest.raises(ValueError):
            ix.query(tq, K7, allow=torch.from_numpy(mask))         # a tensor in host memory
        with pytest.raises(TypeError):
            ix.query(tq, K7, allow=torch.ones(2500, dtype=torch.float32, device=dev))


# ----------------------------------------------------------------------------------------------------------------
# 9. a refusal that needs a device
# ----------------------------------------------------------------------------------------------------------------
def test_another_device_is_refused_with_the_outputs_untouched():
    from kmcuda_amd import KnnIndex
    x, c, a = cached(("chunks",), lambda: corpus(2500, 64, 24, 1700))
    q = fresh(c, 50, 17)
    mask = half_mask(2500, 17).astype(numpy.uint8)
    vp = lambda v: ctypes.c_void_p(v.ctypes.data)   # noqa: E731
    with KnnIndex(x, c, a) as ix:
        nb = numpy.full((50, K7), 12345, numpy.uint32)
        dist = numpy.full((50, K7), -1.0, numpy.float32)
        radii = numpy.full(24, -2.0, numpy.float32)
        other = ix.device + 1
        assert ix.lib.kmamd_knn_index_query_allow(ix.h, K7, 50, vp(q), None, vp(nb), vp(dist), None, other, vp(mask)) == 1
        assert ix.lib.kmamd_knn_index_query_probe_allow(ix.h, K7, P3, 50, vp(q), None, vp(nb), vp(dist), None, other,
                                                        vp(mask)) == 1
        assert ix.lib.kmamd_knn_index_radii_allow(ix.h, vp(mask), other, vp(radii)) == 1
        assert (nb == 12345).all() and (dist == -1.0).all() and (radii == -2.0).all()
        # k and nprobe as in the calls mirrored; no queries: success, nothing written
        assert ix.lib.kmamd_knn_index_query_allow(ix.h, 0, 50, vp(q), None, vp(nb), vp(dist), None, -1, vp(mask)) == 1
        assert ix.lib.kmamd_knn_index_query_probe_allow(ix.h, K7, 25, 50, vp(q), None, vp(nb), vp(dist), None, -1,
                                                        vp(mask)) == 1
        assert ix.lib.kmamd_knn_index_query_allow(ix.h, K7, 0, None, None, None, None, None, -1, vp(mask)) == 0
        assert (nb == 12345).all() and (dist == -1.0).all()
        # a null mask is the unmasked call
        assert ix.lib.kmamd_knn_index_query_allow(ix.h, K7, 50, vp(q), None, vp(nb), vp(dist), None, -1, None) == 0
        same((nb, dist), ix.query(q, K7), "allow == NULL")
