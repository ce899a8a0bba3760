"""Multi-probe search of the k-NN index (KnnIndex.query(nprobe= / probes=)) against its executable
definition, tests/_probe_ref.probe_reference: the CPU oracle on the corpus restricted to each query's probe set.  L2 and
the half2 arithmetic bit for bit, angular under the allowance of tests/_angular.py.  Every f16 PROBE instantiation, the
tile / block / visit-map edges, lists that stay under-filled, equality with the exact call at nprobe = K, the entries a
caller's list may carry, non-finite queries, every switch that takes the exact probe kernel, chunking, the counters
(the search looks at nothing outside the probes) and recall, which can only grow with nprobe."""
import re

import numpy
import pytest

import oracle
from _probe_ref import FLT_MAX, NONE, check_probe, probe_reference, run_probe
from test_gpu_knn_edges import blobs, sized

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def unit(v):
    return (v / numpy.linalg.norm(v.astype(numpy.float64), axis=1, keepdims=True)).astype(numpy.float32)


def corpus(n, d, K, seed, metric="L2", half=False, spread=0.15):
    """Blobs with their oracle assignments (unit rows and centres for the angular metric, half values if asked)."""
    x, c, a = blobs(n, d, K, 1.0, seed=seed, spread=spread)
    if metric != "L2":
        x, c = unit(x - 0.5), unit(c - 0.5)
    if half:
        x, c = x.astype(numpy.float16), c.astype(numpy.float16)
    if metric != "L2" or half:
        a, _, _ = oracle.lloyd_assign(x.astype(numpy.float32), c.astype(numpy.float32), metric=metric)
    return x, c, a.astype(numpy.uint32)


def fresh(c, nq, seed, sigma=0.15, metric="L2"):
    """New rows around the centres, a tenth of them far from every cluster."""
    rs = numpy.random.RandomState(seed)
    c32 = c.astype(numpy.float32)
    q = c32[rs.randint(0, len(c), nq)] + rs.randn(nq, c.shape[1]) * sigma
    far = rs.choice(nq, max(1, nq // 10), replace=False)
    q[far] = rs.uniform(-1.0, 2.0, (len(far), c.shape[1]))
    q = q.astype(numpy.float32)
    if metric != "L2":
        q = unit(q)
    return numpy.ascontiguousarray(q.astype(c.dtype))


def nearest(q, c, p, first=None):
    """Q x p caller lists: the p nearest centres in float64 (first: column 0 instead, the rest follows without it)."""
    d2 = ((q[:, None, :].astype(numpy.float64) - c[None].astype(numpy.float64)) ** 2).sum(-1)
    order = numpy.argsort(d2, axis=1, kind="stable")
    if first is not None:
        first = numpy.broadcast_to(numpy.asarray(first), (len(q),))
        order = numpy.stack([numpy.concatenate([[f], o[o != f]]) for f, o in zip(first, order)])
    return numpy.ascontiguousarray(order[:, :p].astype(numpy.uint32))


# ----------------------------------------------------------------------------------------------------------------
# 1. every f16 instantiation: DP 16 .. 1024, padded and full, both metrics, computed probes
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "cos"])
@pytest.mark.parametrize("d", [10, 32, 64, 100, 256, 300, 768, 1000])
def test_every_f16_instantiation(d, metric, monkeypatch):
    from kmcuda_amd import kmeans_predict_top
    n, nq = (2000, 150) if d <= 256 else (1200, 90)
    x, c, a = cached(("inst", d, metric), lambda: corpus(n, d, 24, 300 + d, metric))
    q = fresh(c, nq, d, metric=metric)
    for p, k in ((1, 10), (3, 1), (3, 10), (24, 10)):
        used = check_probe(k, x, c, a, q, nprobe=p, metric=metric, expect="f16", monkeypatch=monkeypatch)[2]
        top = kmeans_predict_top(q, c, p, metric=metric, return_distances=False)
        assert (used == top).all(), (d, metric, p)


@pytest.mark.parametrize("metric", ["L2", "cos"])
@pytest.mark.parametrize("d", [64, 256])
def test_half_rows(d, metric, monkeypatch):
    from kmcuda_amd import kmeans_predict_top
    x, c, a = cached(("half", d, metric), lambda: corpus(2000, d, 24, 400 + d, metric, half=True))
    q = fresh(c, 150, d + 1, metric=metric)
    for p, k in ((1, 10), (3, 10), (24, 1)):
        used = check_probe(k, x, c, a, q, nprobe=p, metric=metric, expect="f16", monkeypatch=monkeypatch)[2]
        assert (used == kmeans_predict_top(q, c, p, metric=metric, return_distances=False)).all()


# ----------------------------------------------------------------------------------------------------------------
# 2. tile and block edges
# ----------------------------------------------------------------------------------------------------------------
SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 200, 0, 130, 5]


@pytest.mark.parametrize("d", [16, 64, 300])
def test_probed_cluster_sizes_around_the_tiles(d, monkeypatch):
    x, c, a = cached(("sizes", d), lambda: sized(SIZES, d, seed=500 + d))
    q = fresh(c, 200, d + 2, sigma=0.12)
    K = len(SIZES)
    check_probe(10, x, c, a, q, probes=nearest(q, c, 4), expect="f16", monkeypatch=monkeypatch)
    check_probe(10, x, c, a, q, probes=nearest(q, c, K), expect="f16", monkeypatch=monkeypatch)
    # an own cluster without corpus rows (clusters 0 and 9)
    own = numpy.where(numpy.arange(len(q)) % 2 == 0, 0, 9)
    check_probe(10, x, c, a, q, probes=nearest(q, c, 5, first=own), expect="f16", monkeypatch=monkeypatch)
    check_probe(3, x, c, a, q, probes=nearest(q, c, 1, first=own), expect="f16", monkeypatch=monkeypatch)


@pytest.mark.parametrize("d,nq", [(64, 511), (64, 512), (64, 513), (300, 127), (300, 128), (300, 129)])
def test_queries_of_one_cluster_around_the_block(d, nq, monkeypatch):
    x, c, a = cached(("block", d), lambda: corpus(1500, d, 20, 600 + d))
    q = fresh(c, nq, nq)
    check_probe(10, x, c, a, q, probes=nearest(q, c, 4, first=7), expect="f16", monkeypatch=monkeypatch)


def test_disjoint_probe_sets_in_one_block(monkeypatch):
    """Every query of the block shares the own cluster and nothing else; next to them queries whose only probe is the
    own cluster and queries with 64 probes."""
    K = 80
    x, c, a = cached(("disjoint",), lambda: corpus(3000, 64, K, 700, spread=0.05))
    q = fresh(c, 78, 3)
    probes = numpy.full((len(q), 64), K, numpy.uint32)
    probes[:, 0] = 0
    for i in range(len(q)):
        if i % 3 == 0:
            probes[i, 1] = 1 + i                              # own + one cluster nobody else names
        elif i % 3 == 1:
            probes[i] = nearest(q[i:i + 1], c, 64, first=0)    # 64 probes
        # else: the own cluster alone
    nb, dist, used, text = check_probe(10, x, c, a, q, probes=probes, expect="f16", monkeypatch=monkeypatch)
    alone = numpy.arange(len(q)) % 3 == 2
    assert (a[nb[alone][dist[alone] < FLT_MAX]] == 0).all()


# ----------------------------------------------------------------------------------------------------------------
# 3. the visit map's words; the smallest K
# ----------------------------------------------------------------------------------------------------------------
def test_visit_map_word_edges(monkeypatch):
    K = 97
    x, c, a = cached(("words",), lambda: corpus(3000, 32, K, 800, spread=0.05))
    q = fresh(c, 120, 4)
    ids = numpy.array([0, 31, 32, 63, 64, 96], numpy.uint32)
    rs = numpy.random.RandomState(0)
    probes = numpy.stack([rs.permutation(ids) for _ in range(len(q))]).astype(numpy.uint32)
    nb, dist, used, text = check_probe(10, x, c, a, q, probes=probes, expect="f16", monkeypatch=monkeypatch)
    assert numpy.isin(a[nb], ids).all()
    # one id per query, each in another word
    check_probe(10, x, c, a, q, probes=probes[:, :1].copy(), expect="f16", monkeypatch=monkeypatch)


@pytest.mark.parametrize("K,p", [(2, 1), (2, 2), (1, 1)])
def test_smallest_k(K, p, monkeypatch):
    x, c, a = cached(("small", K), lambda: corpus(600, 32, K, 900 + K))
    q = fresh(c, 100, 5)
    nb, dist, used, text = check_probe(10, x, c, a, q, nprobe=p, expect="f16", monkeypatch=monkeypatch)
    if K == 1:
        assert (used == 0).all()


# ----------------------------------------------------------------------------------------------------------------
# 4. under-filled lists
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"KMCUDA_AMD_KNN_EXACT": 1}])
def test_k_above_the_probed_rows(env, monkeypatch):
    x, c, a = cached(("under",), lambda: corpus(2000, 64, 24, 1000))
    q = fresh(c, 120, 6)
    k = 200
    nb, dist, used, text = check_probe(k, x, c, a, q, nprobe=2, env=env, monkeypatch=monkeypatch)
    counts = numpy.bincount(a, minlength=24)
    finite_rows = 0
    for i in range(len(q)):
        n = int(counts[used[i][used[i] < 24]].sum())
        if n < k:
            finite_rows += 1
            assert (dist[i, :n] < FLT_MAX).all() and (dist[i, n:] == FLT_MAX).all() and (nb[i, n:] == 0).all()
            assert numpy.isin(a[nb[i, :n]], used[i]).all()
    assert finite_rows > len(q) // 2


# ----------------------------------------------------------------------------------------------------------------
# 5. nprobe = K is the exact call
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,K", [(32, 24), (256, 64), (768, 16)])
def test_all_clusters_probed_equals_query(d, K, monkeypatch):
    from kmcuda_amd import KnnIndex
    x, c, a = cached(("full", d, K), lambda: corpus(2500 if d <= 256 else 1200, d, K, 1100 + d))
    q = fresh(c, 200, 7)
    with KnnIndex(x, c, a) as ix:
        nb0, dist0, qa0 = ix.query(q, 10, return_assignments=True)
        nb1, dist1, qa1, used = ix.query(q, 10, nprobe=K, return_assignments=True, return_probes=True)
    assert (nb0 == nb1).all()
    assert (dist0.view(numpy.uint32) == dist1.view(numpy.uint32)).all()
    assert (qa0 == qa1).all() and (used[:, 0] == qa0).all()
    assert (numpy.sort(used, axis=1) == numpy.arange(K)).all()


# ----------------------------------------------------------------------------------------------------------------
# 6. a caller's lists
# ----------------------------------------------------------------------------------------------------------------
def test_caller_probes(monkeypatch):
    from kmcuda_amd import KnnIndex, kmeans_predict_top
    K = 24
    x, c, a = cached(("caller",), lambda: corpus(2500, 64, K, 1200))
    q = fresh(c, 200, 8)
    top = kmeans_predict_top(q, c, 4, return_distances=False)
    with KnnIndex(x, c, a) as ix:
        nb0, dist0 = ix.query(q, 10, nprobe=4)
        nb1, dist1 = ix.query(q, 10, probes=top)
        # the same sets with fillers, repeats, the own cluster again and the later columns shuffled
        rs = numpy.random.RandomState(1)
        wide = numpy.full((len(q), 11), K, numpy.uint32)
        wide[:, 0] = top[:, 0]
        for i in range(len(q)):
            tail = numpy.concatenate([top[i, 1:], top[i, 1:3], top[i, :1], [K, K]])
            wide[i, 1:1 + len(tail)] = rs.permutation(tail)
        nb2, dist2 = ix.query(q, 10, probes=wide)
    for nb, dist in ((nb1, dist1), (nb2, dist2)):
        assert (nb == nb0).all() and (dist.view(numpy.uint32) == dist0.view(numpy.uint32)).all()
    check_probe(10, x, c, a, q, probes=wide, expect="f16", monkeypatch=monkeypatch)
    # a deliberately far own cluster: column 0 is the FARTHEST centre
    d2 = ((q[:, None, :].astype(numpy.float64) - c[None].astype(numpy.float64)) ** 2).sum(-1)
    far = nearest(q, c, 5, first=d2.argmax(axis=1))
    check_probe(10, x, c, a, q, probes=far, expect="f16", monkeypatch=monkeypatch)
    check_probe(10, x, c, a, q, probes=far, env={"KMCUDA_AMD_KNN_EXACT": 1}, expect="exact", monkeypatch=monkeypatch)


def test_invalid_caller_probes():
    from kmcuda_amd import KnnIndex
    K = 24
    x, c, a = cached(("caller",), lambda: corpus(2500, 64, K, 1200))
    q = fresh(c, 50, 9)
    good = nearest(q, c, 3)
    c_nan = c.copy()
    c_nan[5, 2] = numpy.nan
    a2 = numpy.where(a == 5, 6, a).astype(numpy.uint32)
    with KnnIndex(x, c_nan, a2) as ix:
        ok = numpy.where(good == 5, K, good).astype(numpy.uint32)
        ok[:, 0] = numpy.where(good[:, 0] == 5, 6, good[:, 0])
        ix.query(q, 5, probes=ok)                      # later columns may name anything <= K ...
        later = ok.copy()
        later[3, 2] = 5
        ix.query(q, 5, probes=later)                   # ... a NaN centroid's cluster too (the prune skips it)
        bad = ok.copy()
        bad[7, 0] = 5                                  # column 0 names a NaN centroid
        with pytest.raises(ValueError):
            ix.query(q, 5, probes=bad)
        bad = ok.copy()
        bad[7, 0] = K
        with pytest.raises(ValueError):
            ix.query(q, 5, probes=bad)
        # the library's own checks (the Python layer refuses these first)
        import ctypes
        nb = numpy.empty((len(q), 5), numpy.uint32)
        for i, j, v in ((7, 0, K), (7, 2, K + 1)):
            bad = ok.copy()
            bad[i, j] = v
            rc = ix.lib.kmamd_knn_index_query_probe(ix.h, 5, 3, len(q), ctypes.c_void_p(q.ctypes.data),
                                                    ctypes.c_void_p(bad.ctypes.data), ctypes.c_void_p(nb.ctypes.data),
                                                    None, None, -1)
            assert rc == 1, (i, j, v, rc)
        for k, p in ((0, 3), (5, 0), (5, K + 1), (5, 65)):
            rc = ix.lib.kmamd_knn_index_query_probe(ix.h, k, p, len(q), ctypes.c_void_p(q.ctypes.data), None,
                                                    ctypes.c_void_p(nb.ctypes.data), None, None, -1)
            assert rc == 1, (k, p, rc)
        assert ix.lib.kmamd_knn_index_query_probe(ix.h, 5, 3, 0, None, None, None, None, None, -1) == 0


# ----------------------------------------------------------------------------------------------------------------
# 7. non-finite queries
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"KMCUDA_AMD_KNN_EXACT": 1}])
def test_non_finite_queries(env, monkeypatch):
    x, c, a = cached(("nonfinite",), lambda: corpus(2000, 64, 24, 1300))
    q = fresh(c, 120, 10)
    q[3, 0] = numpy.nan
    q[40, 17] = numpy.nan
    q[77, 5] = numpy.inf
    q[78, 63] = -numpy.inf
    nb, dist, used, text = check_probe(10, x, c, a, q, nprobe=3, env=env, monkeypatch=monkeypatch)
    for i in (3, 40, 77, 78):
        assert (nb[i] == NONE).all() and numpy.isnan(dist[i]).all()
    # alone: a chunk that holds nothing else
    for i in (3, 40, 77):
        nb1, dist1, _, _ = check_probe(10, x, c, a, q[i:i + 1], nprobe=3, env=env, monkeypatch=monkeypatch)
        assert (nb1 == NONE).all() and numpy.isnan(dist1).all()
    check_probe(10, x, c, a, q, probes=nearest(numpy.nan_to_num(q, posinf=0, neginf=0), c, 3), env=env,
                monkeypatch=monkeypatch)


# ----------------------------------------------------------------------------------------------------------------
# 8. the searches without an f16 filter: the exact probe kernel
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "cos"])
@pytest.mark.parametrize("env", [{"KMCUDA_AMD_KNN_EXACT": 1}, {"KMCUDA_AMD_FILTER": "f32"}])
def test_exact_paths(env, metric, monkeypatch):
    x, c, a = cached(("paths", metric), lambda: corpus(2000, 64, 24, 1400, metric))
    q = fresh(c, 120, 11, metric=metric)
    for p in (1, 3, 24):
        check_probe(10, x, c, a, q, nprobe=p, metric=metric, env=env, expect="exact", monkeypatch=monkeypatch)


def test_wide_rows(monkeypatch):
    x, c, a = cached(("wide",), lambda: corpus(800, 1100, 12, 1500))
    q = fresh(c, 60, 12)
    check_probe(10, x, c, a, q, nprobe=3, expect="exact", monkeypatch=monkeypatch)


@pytest.mark.parametrize("d", [64, 512])
def test_beyond_the_half_range(d, monkeypatch):
    x, c, a = cached(("range", d), lambda: corpus(1500, d, 24, 1600 + d))
    q = fresh(c, 100, 13)
    x2 = x.copy()
    x2[11] += 2e5                                   # a corpus row (it keeps its cluster: legal, the radius grows)
    nb, dist, used, text = check_probe(10, x2, c, a, q, nprobe=3, expect="exact", monkeypatch=monkeypatch)
    assert "k-NN index: a centred row leaves the half range" in text
    q2 = q.copy()
    q2[5] = c[2] + 1e5                              # a query
    nb, dist, used, text = check_probe(10, x, c, a, q2, nprobe=3, expect="exact", monkeypatch=monkeypatch)
    assert text.count("k-NN query: a centred query leaves the half range, the exact search") == 1, text


def test_half2_arithmetic(monkeypatch):
    from kmcuda_amd import KnnIndex
    x, c, a = cached(("half", 64, "L2"), lambda: corpus(2000, 64, 24, 464, "L2", half=True))
    q = fresh(c, 100, 14)
    probes = nearest(q, c, 3)
    check_probe(10, x, c, a, q, probes=probes, env={"KMCUDA_AMD_FP16_STRICT": 1}, expect="exact", half2=True,
                monkeypatch=monkeypatch)
    with KnnIndex(x, c, a) as ix:
        with pytest.raises(ValueError):
            ix.query(q, 10, nprobe=3)


# ----------------------------------------------------------------------------------------------------------------
# 9. chunks, host and device buffers, repeated calls
# ----------------------------------------------------------------------------------------------------------------
def test_chunking_and_buffers(monkeypatch):
    x, c, a = cached(("chunks",), lambda: corpus(2500, 64, 24, 1700))
    q = fresh(c, 300, 15)
    q[100, 3] = numpy.nan
    (nb0, dist0, used0), _ = run_probe(10, x, c, a, q, nprobe=4)
    (nb1, dist1, used1), _ = run_probe(10, x, c, a, q, nprobe=4)                  # twice: the same bits
    (nb2, dist2, used2), _ = run_probe(10, x, c, a, q, nprobe=4, ptr="device")
    given = used0.copy()
    given[100] = 0   # (the ranking left the NaN query without a cluster: K; a caller's column 0 must name one)
    (nb3, dist3, used3), _ = run_probe(10, x, c, a, q, probes=given, ptr="device")
    assert (used3 == given).all()
    used3 = used0
    monkeypatch.setenv("KMCUDA_AMD_KNN_QUERY_CHUNK", "37")
    (nb4, dist4, used4), _ = run_probe(10, x, c, a, q, nprobe=4)
    monkeypatch.delenv("KMCUDA_AMD_KNN_QUERY_CHUNK")
    monkeypatch.setenv("KMCUDA_AMD_ASSIGN_TOP_ROWS", "128")
    (nb5, dist5, used5), _ = run_probe(10, x, c, a, q, nprobe=4)
    monkeypatch.setenv("KMCUDA_AMD_ASSIGN_TOP", "exact")
    (nb6, dist6, used6), _ = run_probe(10, x, c, a, q, nprobe=4)
    bits = lambda d: numpy.where(numpy.isnan(d), numpy.uint32(0x7FC00000), d.view(numpy.uint32))   # noqa: E731
    for nb, dist, used in ((nb1, dist1, used1), (nb2, dist2, used2), (nb3, dist3, used3), (nb4, dist4, used4),
                           (nb5, dist5, used5), (nb6, dist6, used6)):
        assert (nb == nb0).all() and (bits(dist) == bits(dist0)).all() and (used == used0).all()
    ref_nb, ref_dist = probe_reference(10, x, c, a, q, used0)
    assert (nb0 == ref_nb).all() and (bits(dist0) == bits(ref_dist)).all()


@pytest.mark.parametrize("chunk", [None, 37])
@pytest.mark.parametrize("ptr", ["host", "device"])
def test_without_distances(ptr, chunk, monkeypatch):
    """distances == nullptr in a probed query: the lists are those of the call that returns distances."""
    from kmcuda_amd import KnnIndex
    x, c, a = cached(("chunks",), lambda: corpus(2500, 64, 24, 1700))
    q = fresh(c, 300, 15)
    q[100, 3] = numpy.nan
    if chunk is not None:
        monkeypatch.setenv("KMCUDA_AMD_KNN_QUERY_CHUNK", str(chunk))
    if ptr == "device":
        dev = torch.device("cuda", 0)
        x, c, q = (torch.from_numpy(v).to(dev) for v in (x, c, q))
        a = torch.from_numpy(a.view(numpy.int32)).to(dev)
    with KnnIndex(x, c, a) as ix:
        nb, dist = ix.query(q, 10, nprobe=4)
        only = ix.query(q, 10, nprobe=4, return_distances=False)
    if ptr == "device":
        nb, dist, only = (t.cpu().numpy() for t in (nb, dist, only))
    assert only.shape == nb.shape == (300, 10) and (only == nb).all()
    assert (nb.view(numpy.uint32)[100] == NONE).all() and numpy.isnan(dist[100]).all()
    assert (nb.view(numpy.uint32)[numpy.arange(300) != 100, 0] != NONE).all()


# ----------------------------------------------------------------------------------------------------------------
# 10. the counters: nothing outside the probes is looked at
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"KMCUDA_AMD_KNN_EXACT": 1}])
def test_visited_work(env, monkeypatch):
    x, c, a = cached(("work",), lambda: corpus(3000, 64, 40, 1800))
    q = fresh(c, 400, 16)
    counts = numpy.append(numpy.bincount(a, minlength=40), 0)   # (a filler, 40, names no rows)
    monkeypatch.setenv("KMCUDA_AMD_KNN_STATS", "1")
    for key, v in env.items():
        monkeypatch.setenv(key, str(v))

    def visited(p):
        (nb, dist, used), text = run_probe(10, x, c, a, q, nprobe=p, verbosity=0)
        lines = re.findall(r"k-NN index probe query: (\d+) pairs in visited clusters", text)
        assert len(lines) == 1, text
        return int(lines[0]), used

    got, used = visited(1)
    assert got == int(counts[used[:, 0]].sum())
    got, used = visited(4)
    assert int(counts[used[:, 0]].sum()) <= got <= int(counts[used].sum())
    # the exact query() of the same index prints nothing new
    from kmcuda_amd import KnnIndex
    from test_gpu_kmeans import StdoutListener
    out = StdoutListener()
    with out:
        with KnnIndex(x, c, a) as ix:
            ix.query(q, 10)
    assert "probe" not in out.text


# ----------------------------------------------------------------------------------------------------------------
# 11. recall can only grow with nprobe
# ----------------------------------------------------------------------------------------------------------------
def test_recall_grows_with_nprobe():
    from kmcuda_amd import KnnIndex
    K, k = 64, 10
    x, c, a = cached(("recall",), lambda: corpus(4000, 32, K, 1900, spread=0.3))
    q = fresh(c, 500, 17, sigma=0.3)
    with KnnIndex(x, c, a) as ix:
        exact = ix.query(q, k, return_distances=False)
        recalls, prev_used = [], None
        for p in (1, 4, 16, 64):
            nb, used = ix.query(q, k, nprobe=p, return_distances=False, return_probes=True)
            if prev_used is not None:   # the probe sets are nested
                assert (used[:, :prev_used.shape[1]] == prev_used).all()
            prev_used = used
            hits = sum(len(numpy.intersect1d(nb[i], exact[i])) for i in range(len(q)))
            recalls.append(hits / float(exact.size))
    print("recall@10 at nprobe 1, 4, 16, 64:", recalls)
    assert all(b >= a_ for a_, b in zip(recalls, recalls[1:])), recalls
    assert recalls[-1] == 1.0, recalls
    assert recalls[0] < 1.0, recalls   # (the data make the question a real one)
