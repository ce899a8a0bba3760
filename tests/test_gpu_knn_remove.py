"""Rows removed from a k-NN index in place (KnnIndex.remove; knn_index.cpp, knn_remove.hip).

After remove the index must be the index KnnIndex builds from the same rows and centroids with the assignments of the
removed ids set to K: "equal" below always means identical neighbour arrays and identical distance BIT PATTERNS (uint32
views) for query, query(nprobe=3), query_radius(sort=False) and query_radius(count_only=True), identical radii() bit
patterns (NaN equals NaN) and identical info()[:2].

1. Against the CPU oracle (L2) on every search path and feature counts on both sides of every padded width.
2. Against a fresh index: both metrics, fp32 and fp16x2, the half2 arithmetic.
3. The edges: a cluster emptied, a second remove, ids without a cluster, duplicates, an empty list, one id, the first and
   the last sorted position, all rows but one, K = 1, the copy's tile edge, the single-element copy, a padded width,
   k = n_rows.
4. A large index (many blocks; the kernels' grids stride only beyond 2^28 rows, which no test can hold).
5. remove and add composed.  6. A refused call leaves the index as it was.  7. The torch surface.  8. Repeatability."""
import ctypes

import numpy
import pytest

import oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PATHS = {"f16": {}, "f32": {"KMCUDA_AMD_FILTER": "f32"}, "exact": {"KMCUDA_AMD_KNN_EXACT": "1"}}
N, NQ, K = 1500, 200, 16


def mixture(n, d, centres=12, seed=0, spread=10.0):
    rng = numpy.random.default_rng(seed)
    mu = rng.uniform(0, spread, (centres, d)).astype(numpy.float32)
    lab = rng.integers(0, centres, n)
    return (mu[lab] + rng.standard_normal((n, d)).astype(numpy.float32)).astype(numpy.float32), mu


def unit(x):
    return (x / numpy.linalg.norm(x, axis=1, keepdims=True)).astype(numpy.float32)


_CACHE = {}


def clustered(d, metric="L2", half=False, n=N, clusters=K, seed=0):
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
        a = a.astype(numpy.uint32)
        for v in (x, c, a, q):
            v.setflags(write=False)
        _CACHE[key] = (x, c, a, q)
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
    """Everything the four searches return for the queries q, the radii and the row counts."""
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
    out["radii"] = ix.radii()
    out["info"] = numpy.array(ix.info()[:2], numpy.int64)
    return out


def assert_equal(got, want, what=""):
    assert set(got) == set(want)
    for name in want:
        g, w = bits(got[name]), bits(want[name])
        assert g.shape == w.shape, "%s %s: shape %s against %s" % (what, name, g.shape, w.shape)
        assert (g == w).all(), "%s %s: %d of %d entries differ" % (what, name, (g != w).sum(), g.size)


def real(dist):
    """The slots a candidate filled (the others hold row 0 at FLT_MAX, as on a fresh index)."""
    return dist < numpy.float32(3.0e38)


def patched(a, ids, clusters):
    ap = numpy.array(a, dtype=numpy.uint32, copy=True)
    ap[numpy.asarray(ids, dtype=numpy.int64)] = clusters
    return ap


def fresh_snapshot(x, c, a, q, metric="L2", k=7, probe=3):
    from kmcuda_amd import KnnIndex
    with KnnIndex(x, c, a, metric=metric) as ix:
        return snapshot(ix, q, k=k, probe=probe)


def lost_by(a, ids, clusters):
    """The distinct ids that have a cluster."""
    ids = numpy.unique(numpy.asarray(ids, dtype=numpy.int64))
    return int((numpy.asarray(a)[ids] < clusters).sum())


def check_against_fresh(x, c, a, q, lists, metric="L2", k=7, probe=3, what=""):
    """remove(ids) for every list in turn on KnnIndex(x, c, a), each return value checked; the index then equals the
    fresh one on the patched assignments.  Returns the snapshot after the last remove."""
    from kmcuda_amd import KnnIndex
    clusters = len(c)
    now = numpy.array(a, dtype=numpy.uint32, copy=True)
    with KnnIndex(x, c, a, metric=metric) as ix:
        for ids in lists:
            assert ix.remove(ids) == lost_by(now, ids, clusters), what
            now = patched(now, ids, clusters)
        assert ix.n_rows == len(x)
        want = fresh_snapshot(x, c, now, q, metric, k=k, probe=probe)
        got = snapshot(ix, q, k=k, probe=probe, radius=want["radius"])
    assert_equal(got, want, what)
    assert tuple(got["info"]) == (len(x), int((now < clusters).sum()))
    gone = numpy.nonzero(now >= clusters)[0]
    for name, dist in (("nb", "dist"), ("r_nb", "r_dist")) + ((("probe_nb", "probe_dist"),) if probe else ()):
        found = got[name][real(got[dist])]
        assert not numpy.isin(found, gone).any(), "%s %s holds a removed row" % (what, name)
    return got


def first_neighbours_and_random(nb_before, n, seed=1):
    """The first neighbour of each of the first 100 queries before the removal, and 100 random ids."""
    rng = numpy.random.default_rng(seed)
    return numpy.concatenate([nb_before[:100, 0], rng.choice(n, 100, replace=False)]).astype(numpy.uint32)


# ---- 1. against the oracle ------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_lists(d, ids):
    key = (d, ids.tobytes())
    if key not in _ORACLE:
        x, c, a, q = clustered(d)
        _ORACLE[key] = oracle.knn_query(7, x, c, patched(a, ids, K), q)
    return _ORACLE[key]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("d", [20, 64, 256, 320, 1152])
def test_remove_against_the_oracle(monkeypatch, path, d):
    from kmcuda_amd import KnnIndex
    x, c, a, q = clustered(d)
    set_env(monkeypatch, PATHS[path])
    with KnnIndex(x, c, a) as ix:
        before, _ = ix.query(q, 7)
        ids = first_neighbours_and_random(before, N)
        lost = ix.remove(ids)
        nb, dist = ix.query(q, 7)
        assert ix.n_rows == N and ix.info()[:2] == (N, N - lost)
    assert lost == lost_by(a, ids, K) and 100 <= lost <= 200
    assert numpy.isin(before, ids).any(axis=1)[:100].all()   # (doing nothing cannot pass)
    assert not numpy.isin(nb, ids).any()
    ref_nb, ref_dist = oracle_lists(d, ids)
    assert (nb == ref_nb).all(), "%d lists differ" % (nb != ref_nb).any(axis=1).sum()
    assert (bits(dist) == bits(ref_dist)).all()


# ---- 2. against a fresh index -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_remove_equals_a_fresh_index(monkeypatch, metric, half):
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64, metric, half)
    before = fresh_snapshot(x, c, a, q, metric)
    ids = first_neighbours_and_random(before["nb"], N)
    got = check_against_fresh(x, c, a, q, [ids], metric, what="%s half=%s" % (metric, half))
    assert got["r_off"][-1] > 0 and (got["nb"] != before["nb"]).any()


def test_remove_under_the_half2_arithmetic(monkeypatch):
    x, c, a, q = clustered(32, "L2", True)
    set_env(monkeypatch, {"KMCUDA_AMD_FP16_STRICT": "1"})
    before = fresh_snapshot(x, c, a, q, probe=0)
    ids = first_neighbours_and_random(before["nb"], N)
    got = check_against_fresh(x, c, a, q, [ids], probe=0, what="half2")
    assert (got["nb"] != before["nb"]).any()


# ---- 3. the edges -------------------------------------------------------------------------------------------------------
def test_every_member_of_one_cluster(monkeypatch):
    """Cluster 5 loses all its rows: its radius reads NaN (the searches then skip it) and queries that sit on its former
    members find rows of other clusters only."""
    from kmcuda_amd import KnnIndex
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    ids = numpy.nonzero(a == 5)[0]
    assert len(ids) > 7
    near5 = (x[ids[:20]] + 0.01).astype(numpy.float32)
    qq = numpy.concatenate([q, near5])
    got = check_against_fresh(x, c, a, qq, [ids], what="cluster 5 emptied")
    members = numpy.bincount(a, minlength=K)
    assert (numpy.isnan(got["radii"]) == ((members == 0) | (numpy.arange(K) == 5))).all()
    with KnnIndex(x, c, a) as ix:
        assert (numpy.isnan(ix.radii()) == (members == 0)).all()
        nb0 = ix.query(near5, 1, return_distances=False)
    assert (a[nb0[:, 0]] == 5).all() and (a[got["nb"][NQ:]] != 5).all()


def test_second_remove_of_the_same_ids(monkeypatch):
    from kmcuda_amd import KnnIndex
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    ids = numpy.random.default_rng(2).choice(N, 300, replace=False)
    with KnnIndex(x, c, a) as ix:
        assert ix.remove(ids) == 300
        once = snapshot(ix, q)
        assert ix.remove(ids) == 0 and ix.remove(ids[:5]) == 0
        assert_equal(snapshot(ix, q, radius=once["radius"]), once, "second remove")
    assert_equal(once, fresh_snapshot(x, c, patched(a, ids, K), q), "first remove")


def test_ids_without_a_cluster_duplicates_and_empty_lists(monkeypatch):
    from kmcuda_amd import KnnIndex
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    a0 = patched(a, [3, 50, N - 1], K)   # given as K at create
    a0[50] = K + 7                        # (any id >= K)
    check_against_fresh(x, c, a0, q, [[3, 50, 7]], what="ids given as K")
    check_against_fresh(x, c, a0, q, [numpy.array([9, 9, 9, 12, 12, 3, 9], numpy.int64)], what="duplicates")
    with KnnIndex(x, c, a0) as ix:
        before = snapshot(ix, q)
        assert ix.remove(numpy.zeros(0, numpy.uint32)) == 0 and ix.remove([]) == 0
        assert ix.remove([3, 50, N - 1]) == 0   # nothing listed has a cluster
        assert_equal(snapshot(ix, q, radius=before["radius"]), before, "empty lists")


def test_single_ids_and_the_ends_of_the_sorted_order(monkeypatch):
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    first = int(numpy.nonzero(a == 0)[0][0])       # sorted position 0
    last = int(numpy.nonzero(a == K - 1)[0][-1])   # the last position in front of the tail
    check_against_fresh(x, c, a, q, [[777]], what="one id")
    check_against_fresh(x, c, a, q, [[first]], what="the first position")
    check_against_fresh(x, c, a, q, [[last]], what="the last position")
    check_against_fresh(x, c, a, q, [[first, last]], what="both ends")


def test_all_rows_but_one(monkeypatch):
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    ids = numpy.delete(numpy.arange(N), 321)
    got = check_against_fresh(x, c, a, q, [ids], what="one row left")
    found = real(got["dist"])
    assert (found.sum(axis=1) == 1).all() and (got["nb"][found] == 321).all()
    assert int(numpy.isnan(got["radii"]).sum()) == K - 1


def test_one_cluster(monkeypatch):
    set_env(monkeypatch, {})
    x, _, _, q = clustered(64)
    c = x.mean(axis=0, keepdims=True).astype(numpy.float32)
    a = numpy.zeros(N, numpy.uint32)
    ids = numpy.random.default_rng(3).choice(N, 400, replace=False)
    check_against_fresh(x, c, a, q, [ids], probe=1, what="K = 1")


@pytest.mark.parametrize("n", [64, 65, 127])
def test_the_tile_edge_of_the_copy(monkeypatch, n):
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64, n=n, clusters=4)
    ids = numpy.random.default_rng(n).choice(n, n // 3, replace=False)
    check_against_fresh(x, c, a, q, [ids, [0, n - 1]], what="%d rows" % n)


def test_single_element_copy_and_padded_width(monkeypatch):
    """d = 21 on the exact search: DP = D, the copy moves single elements.  d = 36 on the f16 filter: DP is padded."""
    from kmcuda_amd import KnnIndex
    x, c, a, q = clustered(21)
    ids = numpy.random.default_rng(4).choice(N, 200, replace=False)
    set_env(monkeypatch, {"KMCUDA_AMD_KNN_EXACT": "1"})
    check_against_fresh(x, c, a, q, [ids], what="d = 21, exact")
    x, c, a, q = clustered(36)
    set_env(monkeypatch, {})
    with KnnIndex(x, c, a) as ix:
        assert ix.info()[2] == 2
    check_against_fresh(x, c, a, q, [ids], what="d = 36, f16")


def test_k_up_to_n_rows_stays_valid(monkeypatch):
    from kmcuda_amd import KnnIndex
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64, n=100, clusters=4)
    ids = numpy.arange(5, 35)
    got = check_against_fresh(x, c, a, q, [ids], k=100, what="k = n_rows")
    found = real(got["dist"])
    assert (found.sum(axis=1) == 70).all()
    assert (numpy.sort(got["nb"][found].reshape(NQ, 70), axis=1) == numpy.delete(numpy.arange(100), ids)).all()
    with KnnIndex(x, c, a) as ix:
        ix.remove(ids)
        with pytest.raises(ValueError):
            ix.query(q, 101)


# ---- 4. a large index ---------------------------------------------------------------------------------------------------
def test_many_blocks(monkeypatch):
    from kmcuda_amd import KnnIndex, kmeans_predict
    set_env(monkeypatch, {})
    n = 300000
    rng = numpy.random.default_rng(5)
    x, _ = mixture(n + 64, 16, seed=5)
    x, q = numpy.ascontiguousarray(x[:n]), numpy.ascontiguousarray(x[n:])
    c = numpy.ascontiguousarray(x[rng.choice(n, K, replace=False)])
    a = kmeans_predict(x, c).astype(numpy.uint32)
    ids = rng.choice(n, 100000, replace=False)
    with KnnIndex(x, c, a) as ix:
        assert ix.remove(ids) == 100000
        got = snapshot(ix, q)
    assert_equal(got, fresh_snapshot(x, c, patched(a, ids, K), q), "300 000 rows")
    assert not numpy.isin(got["nb"], ids).any()


# ---- 5. composition -----------------------------------------------------------------------------------------------------
def test_remove_then_add(monkeypatch):
    from kmcuda_amd import KnnIndex
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    na = 1000
    ids = numpy.random.default_rng(6).choice(na, 250, replace=False)
    with KnnIndex(x[:na], c, a[:na]) as ix:
        assert ix.remove(ids) == 250
        assert ix.add(x[na:], a[na:]) == na   # the ids go on from the unchanged n_rows
        assert ix.info()[:2] == (N, N - 250)
        got = snapshot(ix, q)
    assert (got["nb"] >= na).any()
    assert_equal(got, fresh_snapshot(x, c, patched(a, ids, K), q), "remove, add")


def test_add_then_remove(monkeypatch):
    from kmcuda_amd import KnnIndex
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    na = 1000
    ids = numpy.concatenate([numpy.arange(na, N, 3), [0, 999]])   # a third of the added rows, two of the first
    with KnnIndex(x[:na], c, a[:na]) as ix:
        assert ix.add(x[na:], a[na:]) == na
        assert ix.remove(ids) == len(ids)
        got = snapshot(ix, q)
    assert_equal(got, fresh_snapshot(x, c, patched(a, ids, K), q), "add, remove")


def test_three_removes_in_a_row(monkeypatch):
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    rng = numpy.random.default_rng(7)
    lists = [rng.choice(N, 200, replace=False) for _ in range(3)]   # (they overlap: the later ones count fewer)
    check_against_fresh(x, c, a, q, lists, what="three removes")


# ---- 6. a refused call changes nothing ----------------------------------------------------------------------------------
def test_untouched_on_refusal(monkeypatch):
    from kmcuda_amd import KnnIndex
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    p = ctypes.c_void_p
    with KnnIndex(x, c, a) as ix:
        before = snapshot(ix, q)
        with pytest.raises(ValueError):
            ix.remove([1, N])                                   # an id equal to n_rows
        with pytest.raises(ValueError):
            ix.remove(torch.tensor([1, N], device="cuda"))
        with pytest.raises(ValueError):
            ix.remove(numpy.array([[1, 2]]))                    # a wrong rank
        with pytest.raises(ValueError):
            ix.remove(torch.tensor([1, 2]))                     # a tensor that is not on the device
        with pytest.raises(TypeError):
            ix.remove(numpy.array([1.0, 2.0]))                  # a wrong dtype
        with pytest.raises(TypeError):
            ix.remove(torch.tensor([1.0, 2.0], device="cuda"))
        bad = numpy.array([1, 2, N], numpy.uint32)
        bad_dev = torch.from_numpy(bad.astype(numpy.int32)).cuda()
        lost = ctypes.c_uint32(123)
        assert ix.lib.kmamd_knn_index_remove(ix.h, 3, bad.ctypes.data_as(p), lost, -1) == 1   # kmcudaInvalidArguments
        assert ix.lib.kmamd_knn_index_remove(ix.h, 3, p(bad_dev.data_ptr()), lost, ix.device) == 1
        # device_ptrs naming another device; null ids
        assert ix.lib.kmamd_knn_index_remove(ix.h, 2, bad.ctypes.data_as(p), lost, ix.device + 1) == 1
        assert ix.lib.kmamd_knn_index_remove(ix.h, 2, None, lost, -1) == 1
        assert lost.value == 123
        assert ix.n_rows == N and ix.info() == (N, N, 2)
        assert_equal(snapshot(ix, q, radius=before["radius"]), before, "after the refusals")
        # the same call with the ids in range goes through
        assert ix.lib.kmamd_knn_index_remove(ix.h, 2, bad.ctypes.data_as(p), lost, -1) == 0 and lost.value == 2


# ---- 7. the torch surface -----------------------------------------------------------------------------------------------
def test_torch_tensors_equal_numpy(monkeypatch):
    from kmcuda_amd import KnnIndex
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    ids = numpy.random.default_rng(8).choice(N, 300, replace=False)
    with KnnIndex(x, c, a) as ix:
        assert ix.remove(ids[:200]) == 200 and ix.remove(ids[100:]) == 100
        want = snapshot(ix, q)
    dev = torch.device("cuda", 0)
    tx, tc, tq = (torch.from_numpy(v.copy()).to(dev) for v in (x, c, q))
    ta = torch.from_numpy(a.astype(numpy.int32)).to(dev)
    with KnnIndex(tx, tc, ta) as ix:
        assert ix.remove(torch.from_numpy(ids[:200].astype(numpy.int64)).to(dev)) == 200
        assert ix.remove(torch.from_numpy(ids[100:].astype(numpy.int32)).to(dev)) == 100
        assert ix.remove(ids[:10]) == 0   # (a host list on an index built from tensors)
        nb, dist = ix.query(tq, 7)
        assert nb.is_cuda and dist.is_cuda
        counts = ix.query_radius(tq, float(want["radius"]), count_only=True)
        assert (bits(ix.radii()) == bits(want["radii"])).all() and ix.info()[:2] == tuple(want["info"])
    assert (nb.cpu().numpy().view(numpy.uint32) == want["nb"]).all()
    assert (bits(dist.cpu().numpy()) == bits(want["dist"])).all()
    assert (counts.cpu().numpy().view(numpy.uint32) == want["r_count"]).all()


# ---- 8. repeatability ---------------------------------------------------------------------------------------------------
def test_same_sequence_same_bits(monkeypatch):
    from kmcuda_amd import KnnIndex
    set_env(monkeypatch, {})
    x, c, a, q = clustered(64)
    ids = numpy.random.default_rng(9).choice(N, 500, replace=True)
    runs = []
    for _ in range(2):
        with KnnIndex(x, c, a) as ix:
            ix.remove(ids[:250])
            ix.remove(ids[250:])
            runs.append(snapshot(ix, q))
    assert_equal(runs[1], runs[0], "second run")
