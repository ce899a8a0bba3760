"""Rows added to a k-NN index in place (KnnIndex.add; knn_index.cpp, knn_merge.hip).

After add the index must be the index KnnIndex builds from the concatenation: "equal" below always means identical
neighbour arrays and identical distance BIT PATTERNS (uint32 views), for query, query(nprobe=3), query_radius(sort=False)
and query_radius(count_only=True).

1. Against the CPU oracle (L2) on every search path and feature counts on both sides of every padded width.
2. Against a fresh index: both metrics, fp32 and fp16x2, the half2 arithmetic with the caller's assignments.
3. Computed assignments are kmeans_predict's.
4. The edges of the merge: empty clusters, rows without a cluster, n = 1, a large batch, repeated adds, small chunks,
   the f16 tile padding, K = 1, k up to the new row count.
5. A batch row beyond the half range: the index leaves the f16 filter as the fresh one does.
6. A refused call leaves the index as it was.  7. The torch surface.  8. Repeatability."""
import ctypes

import numpy
import pytest

import oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PATHS = {"f16": {}, "f32": {"KMCUDA_AMD_FILTER": "f32"}, "exact": {"KMCUDA_AMD_KNN_EXACT": "1"}}
NA, NB, NQ, K = 900, 600, 200, 16


def mixture(n, d, centres=12, seed=0, spread=10.0):
    rng = numpy.random.default_rng(seed)
    mu = rng.uniform(0, spread, (centres, d)).astype(numpy.float32)
    lab = rng.integers(0, centres, n)
    return (mu[lab] + rng.standard_normal((n, d)).astype(numpy.float32)).astype(numpy.float32), mu


def unit(x):
    return (x / numpy.linalg.norm(x, axis=1, keepdims=True)).astype(numpy.float32)


_CACHE = {}


def clustered(d, metric="L2", half=False, n=NA + NB, clusters=K, seed=0):
    """(rows, centroids, assignments, outside queries): n rows and NQ further draws of one mixture."""
    key = (d, metric, half, n, clusters, seed)
    if key not in _CACHE:
        x, _ = mixture(n + NQ, d, seed=seed)
        if metric != "L2":
            x = unit(x - x.mean(axis=0))
        if half:
            x = x.astype(numpy.float16)
        x, q = numpy.ascontiguousarray(x[:n]), numpy.ascontiguousarray(x[n:])
        c, a, _ = oracle.kmeans(x, clusters, seed=seed, metric=metric, init="random")
        _CACHE[key] = (x, c, a.astype(numpy.uint32), q)
    return _CACHE[key]


def set_env(monkeypatch, env):
    for name in ("KMCUDA_AMD_FILTER", "KMCUDA_AMD_KNN_EXACT", "KMCUDA_AMD_FP16_STRICT", "KMCUDA_AMD_KNN_ADD_CHUNK"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def bits(x):
    x = numpy.ascontiguousarray(x)
    return x.view(numpy.uint32) if x.dtype == numpy.float32 else x


def snapshot(ix, q, k=7, radius=None, probe=3):
    """Everything the four searches return for the queries q."""
    out = {}
    out["nb"], out["dist"] = ix.query(q, k)
    if probe:
        out["probe_nb"], out["probe_dist"] = ix.query(q, k, nprobe=min(probe, ix.clusters))
    if radius is None:   # a radius with a few hits per query
        kth = out["dist"][:, min(k, 3) - 1]
        kth = kth[numpy.isfinite(kth) & (kth < 1e30)]
        radius = float(numpy.median(kth)) if len(kth) else 1.0
    out["radius"] = numpy.float32(radius)
    out["r_off"], out["r_nb"], out["r_dist"] = ix.query_radius(q, radius, sort=False)
    out["r_count"] = ix.query_radius(q, radius, count_only=True)
    return out


def assert_equal(got, want, what=""):
    assert set(got) == set(want)
    for name in want:
        g, w = bits(got[name]), bits(want[name])
        assert g.shape == w.shape, "%s %s: shape %s against %s" % (what, name, g.shape, w.shape)
        assert (g == w).all(), "%s %s: %d of %d entries differ" % (what, name, (g != w).sum(), g.size)


def fresh_snapshot(x, c, a, q, metric="L2", k=7, probe=3):
    from kmcuda_amd import KnnIndex
    with KnnIndex(x, c, a, metric=metric) as ix:
        return snapshot(ix, q, k=k, probe=probe)


def added_snapshot(x, c, a, q, na, metric="L2", k=7, probe=3, radius=None, assignments=True, pieces=1):
    """The index of the first na rows after the others have been added (in `pieces` calls)."""
    from kmcuda_amd import KnnIndex
    with KnnIndex(x[:na], c, a[:na], metric=metric) as ix:
        cuts = numpy.linspace(na, len(x), pieces + 1).astype(int)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            first = ix.add(x[lo:hi], a[lo:hi] if assignments else None)
            assert first == lo
        assert ix.n_rows == len(x) and ix.info()[0] == len(x)
        return snapshot(ix, q, k=k, probe=probe, radius=radius)


# ---- 1. against the oracle ------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_lists(d):
    if d not in _ORACLE:
        x, c, a, q = clustered(d)
        _ORACLE[d] = oracle.knn_query(7, x, c, a, q)
    return _ORACLE[d]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("d", [20, 64, 256, 320, 1152])
def test_add_against_the_oracle(monkeypatch, path, d):
    from kmcuda_amd import KnnIndex
    x, c, a, q = clustered(d)
    ref_nb, ref_dist = oracle_lists(d)
    set_env(monkeypatch, PATHS[path])
    with KnnIndex(x[:NA], c, a[:NA]) as ix:
        assert ix.add(x[NA:], a[NA:]) == NA
        nb, dist = ix.query(q, 7)
    assert (nb >= NA).any() and (nb[nb != 0xFFFFFFFF] < NA + NB).all()   # (it cannot pass on the first rows alone)
    assert (nb == ref_nb).all(), "%d lists differ" % (nb != ref_nb).any(axis=1).sum()
    assert (bits(dist) == bits(ref_dist)).all()


# ---- 2. against a fresh index -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_add_equals_a_fresh_index(monkeypatch, metric, half):
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64, metric, half)
    want = fresh_snapshot(x, c, a, q, metric)
    assert (want["nb"] >= NA).any() and want["r_off"][-1] > 0
    got = added_snapshot(x, c, a, q, NA, metric, radius=want["radius"])
    assert_equal(got, want, "%s half=%s" % (metric, half))


def test_add_under_the_half2_arithmetic(monkeypatch):
    """KMCUDA_AMD_FP16_STRICT: the caller's assignments work, computed ones are refused (there is no assignment pass)."""
    from kmcuda_amd import KnnIndex
    x, c, a, q = clustered(32, "L2", True)
    set_env(monkeypatch, {"KMCUDA_AMD_FP16_STRICT": "1"})
    want = fresh_snapshot(x, c, a, q, probe=0)
    got = added_snapshot(x, c, a, q, NA, probe=0, radius=want["radius"])
    assert_equal(got, want, "half2")
    with KnnIndex(x[:NA], c, a[:NA]) as ix:
        before = snapshot(ix, q, probe=0, radius=want["radius"])
        with pytest.raises(ValueError):
            ix.add(x[NA:])
        # the library refuses on its own too
        rc = ix.lib.kmamd_knn_index_add(ix.h, NB, x[NA:].ctypes.data_as(ctypes.c_void_p), None, None, None, -1)
        assert rc == 1   # kmcudaInvalidArguments
        assert ix.n_rows == NA and ix.info()[0] == NA
        assert_equal(snapshot(ix, q, probe=0, radius=want["radius"]), before, "after the refusal")


# ---- 3. computed assignments ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,half", [("L2", False), ("angular", False), ("L2", True)])
def test_computed_assignments_are_kmeans_predict(monkeypatch, metric, half):
    from kmcuda_amd import KnnIndex, kmeans_predict
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64, metric, half)
    pred = kmeans_predict(x[NA:], c, metric=metric)
    with KnnIndex(x[:NA], c, a[:NA], metric=metric) as ix:
        first, used = ix.add(x[NA:], return_assignments=True)
        assert first == NA
        assert used.dtype == numpy.uint32 and (used == pred).all()
        got = snapshot(ix, q)
    a2 = numpy.concatenate([a[:NA], pred]).astype(numpy.uint32)
    want = fresh_snapshot(x, c, a2, q, metric)
    assert_equal(got, want, "computed")


# ---- 4. the edges of the merge ----------------------------------------------------------------------------------------
def test_cluster_empty_before_filled_by_the_batch(monkeypatch):
    """Cluster 5 has no row in the index (radius NaN) and gets all its rows from the batch; cluster K (one more, far away)
    stays empty in both."""
    from kmcuda_amd import KnnIndex
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    order = numpy.argsort(a == 5, kind="stable")   # cluster 5's rows last
    x, a = numpy.ascontiguousarray(x[order]), numpy.ascontiguousarray(a[order])
    n5 = int((a == 5).sum())
    assert 0 < n5 <= NB and not (a[:NA] == 5).any()
    c = numpy.concatenate([c, c[:1] + 100.0]).astype(numpy.float32)   # an empty cluster for good
    near5 = (x[a == 5][:20] + 0.01).astype(numpy.float32)   # queries whose cluster is 5
    qq = numpy.concatenate([q, near5])
    want = fresh_snapshot(x, c, a, qq)
    with KnnIndex(x[:NA], c, a[:NA]) as ix:
        ix.add(x[NA:], a[NA:])
        got = snapshot(ix, qq, radius=want["radius"])
        nb, _, qa = ix.query(near5, 3, return_assignments=True)
    assert_equal(got, want, "filled cluster")
    assert (qa == 5).all()
    assert (a[nb[:, 0]] == 5).all() and (nb[:, 0] >= NA).all()   # their nearest rows are cluster 5's, all new


def test_batch_inside_one_cluster(monkeypatch):
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    order = numpy.argsort(a == 3, kind="stable")
    x, a = numpy.ascontiguousarray(x[order]), numpy.ascontiguousarray(a[order])
    na = len(x) - int((a == 3).sum()) // 2   # the batch: half of cluster 3, nothing else
    assert (a[na:] == 3).all() and (a[:na] == 3).any()
    want = fresh_snapshot(x, c, a, q)
    assert_equal(added_snapshot(x, c, a, q, na, radius=want["radius"]), want, "one cluster")


@pytest.mark.parametrize("where", ["index", "batch", "both"])
def test_rows_without_a_cluster(monkeypatch, where):
    """assignment = K (the caller's) and a NaN first feature (computed): never returned, counted in n_rows only, and
    the ids of later rows still count them."""
    from kmcuda_amd import KnnIndex
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    x, a = x.copy(), a.copy()
    if where in ("index", "both"):
        a[[0, 17, NA - 1]] = K
    with KnnIndex(x[:NA], c, a[:NA]) as ix:
        assert ix.info()[:2] == (NA, NA - int((a[:NA] == K).sum()))
        if where == "index":
            assert ix.add(x[NA:], a[NA:]) == NA
        else:
            a[[NA + 30, NA + NB - 2]] = K
            x[NA + 11, 0] = numpy.nan
            first, used = ix.add(x[NA:NA + 20], return_assignments=True)   # the NaN row: no cluster by the pass
            assert first == NA and used[11] == K and (used != K).sum() == 19
            a[NA:NA + 20] = used
            assert ix.add(x[NA + 20:], a[NA + 20:]) == NA + 20
        lost = numpy.nonzero(a == K)[0]
        assert len(lost) == {"index": 3, "batch": 3, "both": 6}[where]
        assert ix.info()[:2] == (NA + NB, NA + NB - len(lost))
        got = snapshot(ix, q)
    for name in ("nb", "probe_nb", "r_nb"):
        assert not numpy.isin(got[name], lost).any()
    assert (got["nb"] >= NA).any()
    assert_equal(got, fresh_snapshot(x, c, a, q), where)


def test_one_row(monkeypatch):
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    n = NA + 1
    want = fresh_snapshot(x[:n], c, a[:n], q)
    assert_equal(added_snapshot(x[:n], c, a[:n], q, NA, radius=want["radius"]), want, "n = 1")


def test_batch_three_times_the_index(monkeypatch):
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    want = fresh_snapshot(x, c, a, q)
    assert_equal(added_snapshot(x, c, a, q, (NA + NB) // 4, radius=want["radius"]), want, "3 x")


def test_three_adds_equal_one(monkeypatch):
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    want = fresh_snapshot(x, c, a, q)
    assert_equal(added_snapshot(x, c, a, q, NA, radius=want["radius"], pieces=3), want, "three adds")


@pytest.mark.parametrize("computed", [False, True])
def test_small_chunks_equal_the_default(monkeypatch, computed):
    """KMCUDA_AMD_KNN_ADD_CHUNK=5: 21 merges, the last of 3 rows, for 103 rows."""
    from kmcuda_amd import KnnIndex
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    n = NA + 103
    with KnnIndex(x[:NA], c, a[:NA]) as ix:
        first, used = ix.add(x[NA:n], None if computed else a[NA:n], return_assignments=True)
        want = snapshot(ix, q)
    monkeypatch.setenv("KMCUDA_AMD_KNN_ADD_CHUNK", "5")
    with KnnIndex(x[:NA], c, a[:NA]) as ix:
        first5, used5 = ix.add(x[NA:n], None if computed else a[NA:n], return_assignments=True)
        got = snapshot(ix, q, radius=want["radius"])
    assert first5 == first == NA and (used5 == used).all()
    assert_equal(got, want, "chunks of 5")
    monkeypatch.delenv("KMCUDA_AMD_KNN_ADD_CHUNK")
    a2 = numpy.concatenate([a[:NA], used]).astype(numpy.uint32)
    assert_equal(want, fresh_snapshot(x[:n], c, a2, q), "default chunk")


@pytest.mark.parametrize("computed", [False, True])
def test_small_chunks_leave_the_same_index(monkeypatch, computed):
    """70 rows onto 30 in chunks of 5 on the f16 path -- 14 merges, each from the state the one before made, the row
    count passing the 64 rows of the f16 tile padding --: info(), radii() and the lists of every row of the index are
    those of the add in one chunk, bit for bit.  Two of the given assignments name no cluster."""
    from kmcuda_amd import KnnIndex
    x, c, a, _ = clustered(64, n=100, clusters=4)
    given = a[30:].copy()
    given[[11, 52]] = 4
    seen = []
    for chunk in ({}, {"KMCUDA_AMD_KNN_ADD_CHUNK": "5"}):
        set_env(monkeypatch, chunk)
        with KnnIndex(x[:30], c, a[:30]) as ix:
            assert ix.info() == (30, 30, 2)
            first, used = ix.add(x[30:], None if computed else given, return_assignments=True)
            assert first == 30 and (computed or (used == given).all())
            seen.append((ix.info(), ix.radii(), used) + tuple(ix.query(x, 7)))
    (info1, radii1, used1, nb1, dist1), (info5, radii5, used5, nb5, dist5) = seen
    assert info5 == info1 == (100, 100 if computed else 98, 2)
    assert (bits(radii5) == bits(radii1)).all() and (used5 == used1).all()
    assert (nb5 == nb1).all() and (bits(dist5) == bits(dist1)).all()
    assert numpy.isin(numpy.arange(30, 100), nb1).sum() == (70 if computed else 68)   # (every added row is somebody's)
    if not computed:
        assert not numpy.isin(nb1, [30 + 11, 30 + 52]).any()                          # (but the two without a cluster)


def test_across_the_f16_tile_padding(monkeypatch):
    """63 rows, then 64, then 65: the zeroed rows past the last one move with every add."""
    from kmcuda_amd import KnnIndex
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64, n=100, clusters=4)
    with KnnIndex(x[:63], c, a[:63]) as ix:
        assert ix.info()[2] == 2
        for n in (64, 65):
            assert ix.add(x[n - 1:n], a[n - 1:n]) == n - 1
            want = fresh_snapshot(x[:n], c, a[:n], q)
            assert_equal(snapshot(ix, q, radius=want["radius"]), want, "%d rows" % n)


def test_one_cluster(monkeypatch):
    set_env(monkeypatch, {})
    x, _, _, q = clustered(64)
    c = x.mean(axis=0, keepdims=True).astype(numpy.float32)
    a = numpy.zeros(len(x), numpy.uint32)
    want = fresh_snapshot(x, c, a, q, probe=1)
    assert_equal(added_snapshot(x, c, a, q, NA, probe=1, radius=want["radius"]), want, "K = 1, given")
    assert_equal(added_snapshot(x, c, a, q, NA, probe=1, radius=want["radius"], assignments=False), want, "K = 1, computed")


def test_k_follows_the_row_count(monkeypatch):
    from kmcuda_amd import KnnIndex
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64, n=100, clusters=4)
    with KnnIndex(x[:30], c, a[:30]) as ix:
        with pytest.raises(ValueError):
            ix.query(q, 31)
        ix.add(x[30:40], a[30:40])
        nb, dist = ix.query(q, 40)
        with pytest.raises(ValueError):
            ix.query(q, 41)
        rc = ix.lib.kmamd_knn_index_query(ix.h, 41, 1, q.ctypes.data_as(ctypes.c_void_p), None,
                                          nb.ctypes.data_as(ctypes.c_void_p), None, None, -1)
        assert rc == 1   # kmcudaInvalidArguments
    with KnnIndex(x[:40], c, a[:40]) as ix:
        ref_nb, ref_dist = ix.query(q, 40)
    assert (nb == ref_nb).all() and (bits(dist) == bits(ref_dist)).all()
    assert (numpy.sort(nb, axis=1) == numpy.arange(40)).all()


# ---- 5. the half range ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,filter_after", [(64, 1), (320, 0)])
def test_batch_row_beyond_the_half_range(monkeypatch, d, filter_after):
    from kmcuda_amd import KnnIndex
    set_env(monkeypatch, {})
    x, c, a, q = clustered(d)
    x = x.copy()
    far = NA + 7
    x[far, 1] = 1.0e5   # centred, no finite half (|x - mu| >= 65520)
    n1 = NA + 300
    qq = numpy.concatenate([q, x[far:far + 1] + 1.0]).astype(numpy.float32)   # one query that finds the far row
    want = fresh_snapshot(x[:n1], c, a[:n1], qq)
    with KnnIndex(x[:NA], c, a[:NA]) as ix:
        assert ix.info() == (NA, NA, 2)
        ix.add(x[NA:n1], a[NA:n1])
        assert ix.info() == (n1, n1, filter_after)
        got = snapshot(ix, qq, radius=want["radius"])
        assert_equal(got, want, "beyond the half range")
        assert got["nb"][-1, 0] == far
        ref_nb, ref_dist = oracle.knn_query(7, x[:n1], c, a[:n1], qq)
        assert (got["nb"] == ref_nb).all() and (bits(got["dist"]) == bits(ref_dist)).all()
        # a later ordinary add still works
        ix.add(x[n1:], a[n1:])
        assert ix.info() == (NA + NB, NA + NB, filter_after)
        want2 = fresh_snapshot(x, c, a, qq)
        assert_equal(snapshot(ix, qq, radius=want2["radius"]), want2, "the add after")
    with KnnIndex(x[:n1], c, a[:n1]) as ix:
        assert ix.info()[2] == filter_after   # the fresh index takes the same search


# ---- 6. a refused call changes nothing ----------------------------------------------------------------------------------
def test_untouched_on_refusal(monkeypatch):
    from kmcuda_amd import KnnIndex
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    b, ab = x[NA:], a[NA:]
    with KnnIndex(x[:NA], c, a[:NA]) as ix:
        before = snapshot(ix, q)
        with pytest.raises(ValueError):
            ix.add(b[:, :32], ab)                               # a wrong feature count
        with pytest.raises(TypeError):
            ix.add(b.astype(numpy.float16), ab)                 # a wrong dtype
        with pytest.raises(TypeError):
            ix.add(b.astype(numpy.float64), ab)
        with pytest.raises(ValueError):
            ix.add(b, ab[:-1])                                  # assignments of the wrong length
        with pytest.raises(TypeError):
            ix.add(b, torch.from_numpy(ab.astype(numpy.int32)).cuda())   # buffers of two kinds
        with pytest.raises(TypeError):
            ix.add(torch.from_numpy(b).cuda(), ab)
        p = ctypes.c_void_p
        first = ctypes.c_uint32(123)
        # device_ptrs naming another device; null rows
        assert ix.lib.kmamd_knn_index_add(ix.h, NB, b.ctypes.data_as(p), ab.ctypes.data_as(p), None, first, ix.device + 1) == 1
        assert ix.lib.kmamd_knn_index_add(ix.h, NB, None, ab.ctypes.data_as(p), None, first, -1) == 1
        assert first.value == 123
        # an empty batch succeeds and changes nothing
        assert ix.add(b[:0], ab[:0]) == NA
        assert ix.n_rows == NA and ix.info() == (NA, NA, 2)
        assert_equal(snapshot(ix, q, radius=before["radius"]), before, "after the refusals")


# ---- 7. the torch surface -----------------------------------------------------------------------------------------------
def test_torch_tensors_equal_numpy(monkeypatch):
    from kmcuda_amd import KnnIndex
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    with KnnIndex(x[:NA], c, a[:NA]) as ix:
        first, used = ix.add(x[NA:], return_assignments=True)
        want = snapshot(ix, q)
    dev = torch.device("cuda", 0)
    tx, tc, tq = (torch.from_numpy(v).to(dev) for v in (x, c, q))
    ta = torch.from_numpy(a.astype(numpy.int32)).to(dev)
    with KnnIndex(tx[:NA], tc, ta[:NA]) as ix:
        tfirst, tused = ix.add(tx[NA:NA + 100], return_assignments=True)
        assert tfirst == NA and tused.is_cuda and tused.dtype == torch.int32
        assert (tused.cpu().numpy().astype(numpy.uint32) == used[:100]).all()
        assert ix.add(tx[NA + 100:], torch.from_numpy(used[100:].astype(numpy.int32)).to(dev)) == NA + 100
        nb, dist = ix.query(tq, 7)
        assert nb.is_cuda and dist.is_cuda
        counts = ix.query_radius(tq, float(want["radius"]), count_only=True)
    assert (nb.cpu().numpy().view(numpy.uint32) == want["nb"]).all()
    assert (bits(dist.cpu().numpy()) == bits(want["dist"])).all()
    assert (counts.cpu().numpy().view(numpy.uint32) == want["r_count"]).all()


# ---- 8. repeatability ---------------------------------------------------------------------------------------------------
def test_same_sequence_same_bits(monkeypatch):
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    one = added_snapshot(x, c, a, q, NA, assignments=False, pieces=2)
    two = added_snapshot(x, c, a, q, NA, assignments=False, pieces=2)
    assert_equal(two, one, "second run")
