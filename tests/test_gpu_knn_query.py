"""k-NN of new rows against a clustered corpus (kmcuda_amd.KnnIndex / knn_query; knn_index.cpp and the search kernels'
query mode).

1. The corpus rows as queries, with their own clusters, at k + 1: column 0 is the row itself, columns 1..k are
   knn_cuda(k) bit for bit -- every search path (f16 filter, f32 filter, exact), both metrics, fp32 and fp16x2, feature
   counts from 64 to above the filters' 1024.
2. Outside queries against a float64 brute force; distances bit-equal to the oracle's arithmetic.
3. Query clusters: the computed ones are oracle.lloyd_assign's; passed-in or even wrong ones give the same lists.
4. Edges: NaN queries, k = N, Q = 1, ragged Q, a query beyond the half range, empty and NaN clusters, small chunks.
5. Reuse of one index and the torch surface."""
import numpy
import pytest

import oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PATHS = {"f16": {}, "f32": {"KMCUDA_AMD_FILTER": "f32"}, "exact": {"KMCUDA_AMD_KNN_EXACT": "1"}}


def mixture(n, d, centres=12, seed=0, spread=10.0):
    rng = numpy.random.default_rng(seed)
    mu = rng.uniform(0, spread, (centres, d)).astype(numpy.float32)
    lab = rng.integers(0, centres, n)
    return (mu[lab] + rng.standard_normal((n, d)).astype(numpy.float32)).astype(numpy.float32), mu


def unit(x):
    return (x / numpy.linalg.norm(x, axis=1, keepdims=True)).astype(numpy.float32)


_CACHE = {}


def clustered(n, d, metric="L2", half=False, clusters=16, seed=0):
    key = (n, d, metric, half, clusters, seed)
    if key not in _CACHE:
        x, _ = mixture(n, d, seed=seed)
        if metric != "L2":
            x = unit(x - x.mean(axis=0))
        if half:
            x = x.astype(numpy.float16)
        c, a, _ = oracle.kmeans(x, clusters, seed=seed, metric=metric, init="random")
        _CACHE[key] = (x, c, a)
    return _CACHE[key]


def set_env(monkeypatch, env):
    for name in ("KMCUDA_AMD_FILTER", "KMCUDA_AMD_KNN_EXACT"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def brute(q, x, k):
    q64, x64 = q.astype(numpy.float64), x.astype(numpy.float64)
    d2 = (q64 * q64).sum(1)[:, None] + (x64 * x64).sum(1)[None, :] - 2.0 * q64 @ x64.T
    d = numpy.sqrt(numpy.maximum(d2, 0.0))
    return numpy.argsort(d, axis=1, kind="stable")[:, :k], d


def assert_matches_truth(nb, q, x, k, what=""):
    """The lists equal the float64 top k except where two candidates tie within fp32 rounding."""
    ref, d = brute(q, x, k)
    rows = numpy.arange(len(q))[:, None]
    got_d, ref_d = d[rows, nb.astype(numpy.int64)], d[rows, ref]
    tol = 1e-5 * numpy.maximum(ref_d, 1.0)
    bad = (nb != ref) & (numpy.abs(got_d - ref_d) > tol)
    assert not bad.any(), "%s: %d of %d entries differ, first query %d" % (what, bad.sum(), bad.size,
                                                                            int(numpy.nonzero(bad)[0][0]))


# ---- 1. the corpus rows as queries ----------------------------------------------------------------------------------
# (above 1024 features every path is the exact search: one case covers it)
@pytest.mark.parametrize("path,d", [(p, d) for d in (64, 256, 512, 1024) for p in PATHS] + [("f16", 1152)])
@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_self_queries_equal_knn_cuda(monkeypatch, path, d, metric):
    from kmcuda_amd import KnnIndex, knn_cuda
    n = 1500 if d <= 256 else 800
    x, c, a = clustered(n, d, metric)
    k = 7
    set_env(monkeypatch, PATHS[path])
    self_nb = knn_cuda(k, x, c, a, metric=metric, device=1)
    with KnnIndex(x, c, a, metric=metric) as ix:
        nb, dist = ix.query(x, k + 1, query_assignments=a)
    assert (nb[:, 0] == numpy.arange(n)).all()
    if metric == "L2":
        assert (dist[:, 0] == 0).all()
    else:
        assert (dist[:, 0] < 1e-3).all()
    assert (nb[:, 1:] == self_nb).all(), "%d rows differ" % (nb[:, 1:] != self_nb).any(axis=1).sum()
    assert (numpy.diff(dist, axis=1) >= 0).all()


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("d", [64, 512])
@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_self_queries_equal_knn_cuda_fp16(monkeypatch, path, d, metric):
    from kmcuda_amd import KnnIndex, knn_cuda
    x, c, a = clustered(1000, d, metric, half=True)
    k = 6
    set_env(monkeypatch, PATHS[path])
    self_nb = knn_cuda(k, x, c, a, metric=metric, device=1)
    with KnnIndex(x, c, a, metric=metric) as ix:
        nb, dist = ix.query(x, k + 1, query_assignments=a)
    assert (nb[:, 0] == numpy.arange(len(x))).all()
    assert (nb[:, 1:] == self_nb).all(), "%d rows differ" % (nb[:, 1:] != self_nb).any(axis=1).sum()


def test_fp16_strict_honoured(monkeypatch):
    """KMCUDA_AMD_FP16_STRICT: the exact kernel's half2 variant, as knn_cuda() (not ignored).  Its distances are sums of
    halves, so ties are common: a list may differ from knn_cuda's (whose heap is one entry shorter) only among equal
    distances."""
    from kmcuda_amd import KnnIndex, knn_cuda
    x, c, a = clustered(800, 32, "L2", half=True)
    with KnnIndex(x, c, a) as ix:
        plain = ix.query(x, 6, query_assignments=a)[1]
    monkeypatch.setenv("KMCUDA_AMD_FP16_STRICT", "1")
    self_nb = knn_cuda(5, x, c, a, device=1)
    with KnnIndex(x, c, a) as ix:
        nb, dist = ix.query(x, 6, query_assignments=a)
    assert (dist != plain).any()   # the half2 arithmetic is in effect
    assert (dist[:, 0] == 0).all()
    differ = numpy.nonzero((nb[:, 1:] != self_nb).any(axis=1))[0]
    assert len(differ) <= len(x) // 10
    for i in differ:
        d = dist[i, 1:]
        assert (numpy.diff(d) == 0).any() or d[-1] == dist[i, -1], (i, nb[i], self_nb[i], dist[i])


# ---- 2. outside queries -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("d", [64, 512])
def test_outside_queries_against_the_truth(monkeypatch, path, d):
    from kmcuda_amd import KnnIndex
    x, c, a = clustered(3000, d)
    fresh, _ = mixture(1200, d, seed=0)   # same mixture centres (same seed), fresh draws below
    rng = numpy.random.default_rng(11)
    fresh = fresh[rng.permutation(len(fresh))] + 0.1 * rng.standard_normal(fresh.shape).astype(numpy.float32)
    far = (rng.uniform(-60, 80, (100, d))).astype(numpy.float32)
    copies = x[rng.choice(len(x), 100, replace=False)]
    q = numpy.ascontiguousarray(numpy.concatenate([fresh, far, copies]).astype(numpy.float32))
    k = 10
    set_env(monkeypatch, PATHS[path])
    with KnnIndex(x, c, a) as ix:
        nb, dist = ix.query(q, k)
    assert_matches_truth(nb, q, x, k, "%s D=%d" % (path, d))
    for i in range(len(q) - 100, len(q)):   # exact copies: the copied row first, at distance 0
        assert dist[i, 0] == 0.0
    pairs = rng.choice(len(q) * k, 300, replace=False)
    for p in pairs:
        i, j = divmod(int(p), k)
        ref = numpy.float32(oracle.distance(q[i], x[nb[i, j]], "L2"))
        assert dist[i, j] == ref, (i, j, dist[i, j], ref)


def test_angular_distances_are_the_oracles():
    from kmcuda_amd import KnnIndex
    x, c, a = clustered(1500, 64, "angular")
    rng = numpy.random.default_rng(5)
    q = unit(rng.standard_normal((300, 64)).astype(numpy.float32) + x[rng.choice(len(x), 300)] * 4)
    with KnnIndex(x, c, a, metric="angular") as ix:
        nb, dist = ix.query(q, 8)
    cos = q.astype(numpy.float64) @ x.astype(numpy.float64).T
    truth = numpy.argsort(-cos, axis=1, kind="stable")[:, :8]
    rows = numpy.arange(len(q))[:, None]
    assert (numpy.abs(cos[rows, nb.astype(numpy.int64)] - cos[rows, truth]) <= 1e-6).all()
    for p in rng.choice(len(q) * 8, 200, replace=False):
        i, j = divmod(int(p), 8)
        assert abs(dist[i, j] - oracle.distance(q[i], x[nb[i, j]], "angular")) <= 2 * numpy.spacing(numpy.float32(dist[i, j]))


# ---- 3. query clusters -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 512])
def test_assignments(d):
    from kmcuda_amd import KnnIndex
    x, c, a = clustered(2000, d)
    q, _ = mixture(700, d, seed=0)
    q = q + numpy.float32(0.05)
    with KnnIndex(x, c, a) as ix:
        nb, dist, qa = ix.query(q, 9, return_assignments=True)
        ref, _, _ = oracle.lloyd_assign(q, c)
        assert (qa == ref).all()
        nb2, dist2 = ix.query(q, 9, query_assignments=qa)
        assert (nb2 == nb).all() and (dist2 == dist).all()
        # any cluster with a finite centroid (the search skips the clusters whose centroid distance is NaN)
        finite = numpy.nonzero(numpy.isfinite(c).all(axis=1))[0]
        wrong = finite[numpy.random.default_rng(2).integers(0, len(finite), len(q))].astype(numpy.uint32)
        nb3, dist3 = ix.query(q, 9, query_assignments=wrong)
    # the prune is rigorous: any cluster gives the same lists (ties aside) and the same distances
    assert (dist3 == dist).all()
    assert ((nb3 == nb) | (dist3 == dist)).all()


def test_cluster_without_a_finite_centroid_is_refused():
    from kmcuda_amd import KnnIndex
    x, c, a = clustered(600, 16, clusters=6)
    c, a = c.copy(), a.copy()
    c[5] = numpy.nan
    a[a == 5] = 0
    with KnnIndex(x, c, a) as ix:
        with pytest.raises(ValueError):
            ix.query(x[:10], 3, query_assignments=numpy.full(10, 5, numpy.uint32))
        nb, _, qa = ix.query(x[:10], 3, return_assignments=True)   # computed clusters never name it
    assert (qa != 5).all() and (nb[:, 0] == numpy.arange(10)).all()


# ---- 4. edges -----------------------------------------------------------------------------------------------------
def test_nan_queries_k_equals_n_and_small_batches():
    from kmcuda_amd import KnnIndex
    x, c, a = clustered(300, 16, clusters=6)
    q = x[:5].copy()
    q[1, 3] = numpy.nan
    q[3, 0] = numpy.inf
    with KnnIndex(x, c, a) as ix:
        nb, dist = ix.query(q, 4)
        assert (nb[[1, 3]] == 0xFFFFFFFF).all() and numpy.isnan(dist[[1, 3]]).all()
        assert (nb[[0, 2, 4], 0] == [0, 2, 4]).all()
        full, fd = ix.query(x[:3], 300)   # k = N: every corpus row, sorted
        for i in range(3):
            assert sorted(full[i].tolist()) == list(range(300))
            assert (numpy.diff(fd[i]) >= 0).all()
        one, od = ix.query(x[7:8], 5)     # Q = 1
        assert one.shape == (1, 5) and one[0, 0] == 7
        e = ix.query(numpy.zeros((0, 16), numpy.float32), 3)
        assert e[0].shape == (0, 3) and e[1].shape == (0, 3)


@pytest.mark.parametrize("path", list(PATHS))
def test_ragged_batch_and_small_chunks(monkeypatch, path):
    from kmcuda_amd import KnnIndex
    x, c, a = clustered(2500, 96)
    rng = numpy.random.default_rng(8)
    q = (x[rng.choice(len(x), 777)] + rng.standard_normal((777, 96)).astype(numpy.float32)).astype(numpy.float32)
    set_env(monkeypatch, PATHS[path])
    with KnnIndex(x, c, a) as ix:
        nb, dist, qa = ix.query(q, 11, return_assignments=True)
        monkeypatch.setenv("KMCUDA_AMD_KNN_QUERY_CHUNK", "100")
        nb2, dist2, qa2 = ix.query(q, 11, return_assignments=True)
    assert (nb == nb2).all() and (dist == dist2).all() and (qa == qa2).all()
    assert_matches_truth(nb, q, x, 11, path)


@pytest.mark.parametrize("d", [64, 512])
def test_query_beyond_the_half_range(d):
    """A 1e6 outlier query: the chunk leaves the f16 filter (f32 filter / exact search), the answer stays right."""
    from kmcuda_amd import KnnIndex
    x, c, a = clustered(1500, d)
    q, _ = mixture(200, d, seed=0)
    q = q.copy()
    q[17, 5] = 1e6
    with KnnIndex(x, c, a) as ix:
        nb, dist = ix.query(q, 6)
        nb_ok, dist_ok = ix.query(numpy.delete(q, 17, axis=0), 6)
    assert_matches_truth(nb, q, x, 6, "outlier D=%d" % d)
    assert (numpy.delete(nb, 17, axis=0) == nb_ok).all() and (numpy.delete(dist, 17, axis=0) == dist_ok).all()


def test_empty_and_unassigned_corpus_clusters():
    from kmcuda_amd import KnnIndex
    x, c, a = clustered(1200, 32, clusters=10)
    x, a = x.copy(), a.copy()
    gone = numpy.nonzero(a == 4)[0]
    a[a == 4] = 5                  # cluster 4 empty (its centroid stays)
    x[::50] = numpy.nan            # rows without a cluster
    a[::50] = 0xFFFFFFFF
    nan_rows = set(range(0, 1200, 50))
    rng = numpy.random.default_rng(4)
    q = x[gone[:30]] + 0.2 * rng.standard_normal((30, 32)).astype(numpy.float32)   # near the empty cluster's centroid
    with KnnIndex(x, c, a) as ix:
        nb, dist, qa = ix.query(q, 12, return_assignments=True)
    assert not nan_rows & set(nb.ravel().tolist())
    keep = numpy.array(sorted(set(range(1200)) - nan_rows))
    sub = brute(q, x[keep], 12)[0]
    rows = numpy.arange(len(q))[:, None]
    _, d = brute(q, numpy.nan_to_num(x, nan=1e9), 12)
    assert (numpy.abs(d[rows, nb.astype(numpy.int64)] - d[rows, keep[sub]]) <= 1e-5 * numpy.maximum(d[rows, keep[sub]], 1)).all()


# ---- 5. reuse and surfaces ----------------------------------------------------------------------------------------
def test_reuse_equals_one_shot_and_torch_surface():
    from kmcuda_amd import KnnIndex, knn_query
    x, c, a = clustered(2000, 64)
    rng = numpy.random.default_rng(9)
    q1 = (x[rng.choice(2000, 300)] + rng.standard_normal((300, 64)).astype(numpy.float32)).astype(numpy.float32)
    q2 = (x[rng.choice(2000, 150)] + rng.standard_normal((150, 64)).astype(numpy.float32)).astype(numpy.float32)
    with KnnIndex(x, c, a) as ix:
        r1, r2 = ix.query(q1, 10), ix.query(q2, 5)
    o1, o2 = knn_query(10, x, c, a, q1), knn_query(5, x, c, a, q2)
    assert all((u == v).all() for u, v in zip(r1 + r2, o1 + o2))
    dev = torch.device("cuda", 0)
    tx, tc, ta, tq = (torch.from_numpy(v).to(dev) for v in (x, c, a.astype(numpy.int32), q1))
    with KnnIndex(tx, tc, ta) as ix:
        nb, dist, qa = ix.query(tq, 10, return_assignments=True)
    assert nb.is_cuda and dist.is_cuda and qa.is_cuda and nb.dtype == torch.int32
    assert (nb.cpu().numpy().view(numpy.uint32) == r1[0]).all() and (dist.cpu().numpy() == r1[1]).all()
    # numpy queries against a torch-built index: numpy out
    with KnnIndex(tx, tc, ta) as ix:
        nbn, distn = ix.query(q1, 10)
    assert isinstance(nbn, numpy.ndarray) and (nbn == r1[0]).all()
