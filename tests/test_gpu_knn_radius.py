"""Radius search on the k-NN index (kmcuda_amd.KnnIndex.query_radius / knn_query_radius; knn_radius.hip).

The result is the brute-force set over the clustered corpus rows by the exact distance KnnIndex.query compares, in
ascending (cluster id, row index) order.  Ground truth: the CPU oracle's distance of every query to every clustered row
(tests/_radius_inputs.py), thresholded.

 1. equality with the oracle: counts, offsets, neighbors in order, distances -- both metrics, fp32 and fp16x2, the
    narrow (64, 256), wide (512) and exact-only (1152) feature counts, the default path and KMCUDA_AMD_KNN_EXACT
 2. the boundary: r = a pair's distance includes it, the float below does not
 3. r = 0 (duplicates) and r above every distance (all clustered rows, in the sorted copy's order)
 4. more than two blocks of one query cluster, Q = 1, a cluster of fewer than 32 rows, ragged cluster sizes
 5. query_assignments do not matter
 6. NaN / inf queries, rows without a cluster, an empty cluster and a NaN centroid, a query beyond the half range
 7. chunking   8. KMCUDA_AMD_FILTER=f32 and KMCUDA_AMD_FP16_STRICT   9. the fill contract through ctypes
10. the torch surface, sort, count_only, one index for query and query_radius, the one-shot call"""
import ctypes

import numpy
import pytest

import oracle
from _radius_inputs import all_distances, clustered, expected, fresh_queries, gap_radius, target_radius, truth, ulps_from

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 2000
ENV = ("KMCUDA_AMD_FILTER", "KMCUDA_AMD_KNN_EXACT", "KMCUDA_AMD_FP16_STRICT", "KMCUDA_AMD_KNN_QUERY_CHUNK")
PATHS = {"default": {}, "exact": {"KMCUDA_AMD_KNN_EXACT": "1"}}


def set_env(monkeypatch, env):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def radius_for(dm, metric):
    """Near the median distance to the 21st neighbour; angular: in the widest gap nearby, 4 ulp clear of every oracle
    distance (acos is ocml's on the device and libm's in the oracle: 2 ulp, tests/_angular.py)."""
    r = target_radius(dm)
    if metric != "L2":
        r = gap_radius(dm, r)
        assert ulps_from(dm, r) >= 4
    return r


def assert_equals(got, exp, metric="L2", what=""):
    """got: (offsets, neighbors, distances) of query_radius; exp: expected(...)."""
    offsets, nb, dist = got
    counts, eoffsets, enb, edist = exp
    assert offsets.dtype == numpy.int64 and nb.dtype == numpy.uint32 and dist.dtype == numpy.float32
    assert (numpy.diff(offsets) == counts).all(), "%s: %d counts differ" % (what, (numpy.diff(offsets) != counts).sum())
    assert (offsets == eoffsets).all() and nb.shape == enb.shape
    assert (nb == enb).all(), "%s: %d of %d neighbors differ" % (what, (nb != enb).sum(), len(enb))
    if metric == "L2":
        assert (dist.view(numpy.uint32) == edist.view(numpy.uint32)).all(), what
    else:
        assert (numpy.abs(dist - edist) <= 2 * numpy.spacing(numpy.maximum(dist, edist))).all(), what


# ---- 1. equality with the oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("d", [64, 256, 512, 1152])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16x2"])
@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_equals_the_oracle(monkeypatch, metric, half, d, path):
    from kmcuda_amd import KnnIndex
    x, c, a, q, dm = truth(N, d, metric, half)
    r = radius_for(dm, metric)
    exp = expected(dm, a, r)
    assert (exp[0] == 0).any() and numpy.median(exp[0]) >= 15 and exp[0].max() >= 100   # the inputs are what they should be
    set_env(monkeypatch, PATHS[path])
    with KnnIndex(x, c, a, metric=metric) as ix:
        counts = ix.query_radius(q, r, count_only=True)
        got = ix.query_radius(q, r)
        qnb, qdist = ix.query(q, N)
    what = "%s %s D=%d %s" % (metric, "fp16x2" if half else "fp32", d, path)
    assert counts.dtype == numpy.uint32 and (counts == exp[0]).all(), what
    assert_equals(got, exp, metric, what)
    # the same device arithmetic as query(): the distances of the same (query, row) pairs, bit for bit
    table = numpy.full((len(q), N), numpy.nan, numpy.float32)
    rows = numpy.nonzero(qnb[:, 0] != 0xFFFFFFFF)[0]
    table[rows[:, None], qnb[rows].astype(numpy.int64)] = qdist[rows]
    qi = numpy.repeat(numpy.arange(len(q)), numpy.diff(got[0]))
    assert (table[qi, got[1].astype(numpy.int64)].view(numpy.uint32) == got[2].view(numpy.uint32)).all(), what


# ---- 2. the boundary ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
def test_boundary(monkeypatch, path):
    from kmcuda_amd import KnnIndex
    x, c, a, q, dm = truth(N, 64)
    qi = 3
    idx = int(numpy.argsort(dm[qi], kind="stable")[9])
    r = dm[qi, idx]
    below = numpy.nextafter(r, numpy.float32(0))
    set_env(monkeypatch, PATHS[path])
    with KnnIndex(x, c, a) as ix:
        at, under = ix.query_radius(q, r), ix.query_radius(q, below)
    assert idx in at[1][at[0][qi]:at[0][qi + 1]]
    assert idx not in under[1][under[0][qi]:under[0][qi + 1]]
    assert_equals(at, expected(dm, a, r))
    assert_equals(under, expected(dm, a, below))


# ---- 3. / 6. a corpus with duplicates and rows without a cluster ---------------------------------------------------
_EDGE = {}


def edge_corpus():
    """The D = 64 L2 corpus (an empty cluster, a NaN centroid, a cluster of one row) with two planted duplicate rows and
    every 50th row without a cluster."""
    if not _EDGE:
        x, c, a = clustered(N, 64)
        x, a = x.copy(), a.copy()
        x[5] = x[900]
        x[77] = x[1234]
        a[10::50] = 0xFFFFFFFF
        a[60] = len(c) + 3
        _EDGE["corpus"] = (x, c, a)
    return _EDGE["corpus"]


def test_zero_radius_returns_duplicates():
    from kmcuda_amd import KnnIndex
    x, c, a = edge_corpus()
    rows = numpy.array([5, 900, 77, 1234] + list(range(100, 160)))
    q = numpy.ascontiguousarray(x[rows])
    dm = all_distances(x, c, a, q)
    with KnnIndex(x, c, a) as ix:
        got = ix.query_radius(q, 0.0)
    assert_equals(got, expected(dm, a, 0.0))
    offsets, nb, dist = got
    assert (dist == 0).all()
    assert set(nb[offsets[0]:offsets[1]]) == {5, 900} and set(nb[offsets[2]:offsets[3]]) == {77, 1234}
    for i, row in enumerate(rows):   # each row itself -- unless it has no cluster -- and nothing else but a duplicate
        hits = set(nb[offsets[i]:offsets[i + 1]].tolist())
        assert hits - {5, 900, 77, 1234} == ({int(row)} if a[row] < len(c) and row not in (5, 900, 77, 1234) else set())


def test_everything_within_a_huge_radius():
    from kmcuda_amd import KnnIndex
    x, c, a = edge_corpus()
    q = numpy.ascontiguousarray(fresh_queries(300, N, 64)[:40])
    dm = all_distances(x, c, a, q)
    r = numpy.nextafter(numpy.nanmax(dm), numpy.float32(numpy.inf))
    members = numpy.nonzero(a < len(c))[0]
    order = members[numpy.lexsort((members, a[members]))].astype(numpy.uint32)   # the sorted copy's order
    with KnnIndex(x, c, a) as ix:
        for radius in (r, 1e30):
            offsets, nb, dist = ix.query_radius(q, radius)
            assert offsets[-1] == 40 * len(members) and (numpy.diff(offsets) == len(members)).all()
            assert (nb.reshape(40, -1) == order[None, :]).all()
            assert (dist.reshape(40, -1) == dm[:, order]).all()


# ---- 4. blocks and tiles -------------------------------------------------------------------------------------------
def test_many_blocks_of_one_cluster_and_one_query():
    """1200 queries of ONE cluster: three blocks of the narrow kernel's 512 queries; the corpus has a cluster of one row
    and cluster sizes that are no multiple of the 64-row tile; then a single query."""
    from kmcuda_amd import KnnIndex
    x, c, a = clustered(N, 64)
    sizes = numpy.bincount(a, minlength=len(c))
    assert (sizes[sizes > 0] < 32).any() and (sizes % 64 != 0).any()
    rng = numpy.random.default_rng(21)
    q = (x[rng.choice(N, 1200)] + 0.7 * rng.standard_normal((1200, 64)).astype(numpy.float32)).astype(numpy.float32)
    dm = all_distances(x, c, a, q)
    r = target_radius(dm)
    one = int(numpy.argmax(sizes))
    with KnnIndex(x, c, a) as ix:
        got = ix.query_radius(q, r, query_assignments=numpy.full(1200, one, numpy.uint32))
        assert_equals(got, expected(dm, a, r))
        single = ix.query_radius(q[7:8], r)
    assert_equals(single, expected(dm[7:8], a, r))


# ---- 5. assignments do not matter ----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,d", [("L2", 64), ("angular", 64), ("L2", 1152)])
def test_assignments_do_not_matter(metric, d):
    from kmcuda_amd import KnnIndex
    x, c, a, q, dm = truth(N, d, metric)
    r = radius_for(dm, metric)
    exp = expected(dm, a, r)
    computed = oracle.lloyd_assign(q, c, metric=metric)[0]
    finite = numpy.nonzero(numpy.isfinite(c).all(axis=1))[0]
    rng = numpy.random.default_rng(2)
    with KnnIndex(x, c, a, metric=metric) as ix:
        base = ix.query_radius(q, r)
        assert_equals(base, exp, metric)
        for qa in (computed, numpy.full(len(q), finite[0], numpy.uint32), computed[rng.permutation(len(q))],
                   finite[rng.integers(0, len(finite), len(q))].astype(numpy.uint32)):
            got = ix.query_radius(q, r, query_assignments=qa)
            assert all((u == v).all() for u, v in zip(got, base))


# ---- 6. edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outlier", [False, True], ids=["f16", "beyond-the-half-range"])
def test_edges(outlier):
    """NaN and inf queries have no hits; rows without a cluster are never returned; with a 1e6 feature in one query the
    chunk takes the exact kernel and the answer stays the oracle's."""
    from kmcuda_amd import KnnIndex
    x, c, a = edge_corpus()
    q = numpy.ascontiguousarray(fresh_queries(300, N, 64)[:120]).copy()
    q[1, 3] = numpy.nan
    q[3, 0] = numpy.inf
    if outlier:
        q[17, 5] = 1e6
    dm = all_distances(x, c, a, q)
    r = target_radius(dm)
    exp = expected(dm, a, r)
    with KnnIndex(x, c, a) as ix:
        got = ix.query_radius(q, r)
        counts = ix.query_radius(q, r, count_only=True)
    assert_equals(got, exp)
    assert (counts == exp[0]).all() and counts[1] == 0 and counts[3] == 0 and counts.sum() > 0
    assert (a[got[1].astype(numpy.int64)] < len(c)).all()


# ---- 7. chunking --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
def test_chunking(monkeypatch, path):
    from kmcuda_amd import KnnIndex
    x, c, a, q, dm = truth(N, 64)
    q = q[:250].copy()
    r = radius_for(dm, "L2")
    set_env(monkeypatch, PATHS[path])
    dev = torch.device("cuda", 0)
    tq = torch.from_numpy(q).to(dev)
    with KnnIndex(x, c, a) as ix:
        whole = ix.query_radius(q, r)
        monkeypatch.setenv("KMCUDA_AMD_KNN_QUERY_CHUNK", "100")
        chunked = ix.query_radius(q, r)
        on_device = ix.query_radius(tq, r)
    assert_equals(whole, expected(dm[:250], a, r))
    assert all((u == v).all() for u, v in zip(chunked, whole))
    assert all(t.is_cuda for t in on_device)
    assert (on_device[0].cpu().numpy() == whole[0]).all()
    assert (on_device[1].cpu().numpy().view(numpy.uint32) == whole[1]).all()
    assert (on_device[2].cpu().numpy() == whole[2]).all()


# ---- 8. switches --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_filter_f32_is_the_exact_kernel(monkeypatch, metric):
    from kmcuda_amd import KnnIndex
    x, c, a, q, dm = truth(N, 64, metric)
    r = radius_for(dm, metric)
    set_env(monkeypatch, {})
    with KnnIndex(x, c, a, metric=metric) as ix:
        base = ix.query_radius(q, r)
    set_env(monkeypatch, {"KMCUDA_AMD_FILTER": "f32"})
    with KnnIndex(x, c, a, metric=metric) as ix:
        got = ix.query_radius(q, r)
    assert_equals(base, expected(dm, a, r), metric)
    assert all((u == v).all() for u, v in zip(got, base))


def test_fp16_strict(monkeypatch):
    """KMCUDA_AMD_FP16_STRICT: the hits by the reference's half2 arithmetic (oracle.knn_query(half2=True) thresholded)."""
    from kmcuda_amd import KnnIndex
    x, c, a = clustered(N, 64, "L2", half=True)
    q = fresh_queries(300, N, 64, "L2", half=True)
    dm = all_distances(x, c, a, q, half2=True)
    plain = truth(N, 64, "L2", True)[4]
    assert (dm != plain)[~numpy.isnan(dm)].any()   # another arithmetic
    r = target_radius(dm)
    set_env(monkeypatch, {"KMCUDA_AMD_FP16_STRICT": "1"})
    with KnnIndex(x, c, a) as ix:
        got = ix.query_radius(q, r)
    assert_equals(got, expected(dm, a, r))


# ---- 9. the fill contract through ctypes ---------------------------------------------------------------------------
def test_fill_contract():
    from kmcuda_amd import KnnIndex
    x, c, a, q, dm = truth(N, 64)
    r = radius_for(dm, "L2")
    counts, offsets, enb, edist = expected(dm, a, r)
    total, nq = int(offsets[-1]), len(q)
    vp, f32p = ctypes.c_void_p, ctypes.c_float
    SENT_I, SENT_F = 0xABCD1234, numpy.float32(-77.5)

    def buffers(extra=16):
        return numpy.full(total + extra, SENT_I, numpy.uint32), numpy.full(total + extra, SENT_F, numpy.float32)

    with KnnIndex(x, c, a) as ix:
        def fill(radius, offs, nb, dist):
            return ix.lib.kmamd_knn_index_radius_fill(ix.h, f32p(radius), nq, vp(q.ctypes.data), None, vp(offs.ctypes.data),
                                                      vp(nb.ctypes.data), vp(dist.ctypes.data) if dist is not None else None, -1)
        # the right offsets: success, and nothing behind the last range
        nb, dist = buffers()
        u64 = offsets.astype(numpy.uint64)
        assert fill(r, u64, nb, dist) == 0
        assert (nb[:total] == enb).all() and (dist[:total] == edist).all()
        assert (nb[total:] == SENT_I).all() and (dist[total:] == SENT_F).all()
        # distances = NULL: indices only
        nb, dist = buffers()
        assert fill(r, u64, nb, None) == 0
        assert (nb[:total] == enb).all() and (nb[total:] == SENT_I).all()
        # decreasing offsets: refused before anything is written
        nb, dist = buffers()
        bad = u64.copy()
        bad[100], bad[101] = bad[101], bad[100]
        assert bad[100] > bad[101]
        assert fill(r, bad, nb, dist) == 1
        assert (nb == SENT_I).all() and (dist == SENT_F).all()
        # offsets of a smaller radius, starting behind 7 slots of the caller's: refused after the search; every range
        # holds the first hits of ITS query (an overrun would land in the next query's range) and nothing else moved
        small = numpy.float32(0.97) * r
        scounts = expected(dm, a, small)[0]
        assert (scounts < counts).any()
        lead = 7
        soff = numpy.full(nq + 1, lead, numpy.uint64)
        soff[1:] += numpy.cumsum(scounts.astype(numpy.uint64))
        nb, dist = buffers(extra=lead + 16)
        assert fill(r, soff, nb, dist) == 1
        assert (nb[:lead] == SENT_I).all() and (dist[:lead] == SENT_F).all()
        assert (nb[int(soff[-1]):] == SENT_I).all() and (dist[int(soff[-1]):] == SENT_F).all()
        for i in range(nq):
            lo, n = int(soff[i]), int(scounts[i])
            assert (nb[lo:lo + n] == enb[offsets[i]:offsets[i] + n]).all(), i
            assert (dist[lo:lo + n] == edist[offsets[i]:offsets[i] + n]).all(), i
        # ... and ranges `slack` slots longer than the hits: refused too; the hits are at the head of their ranges, and
        # the slots the search did not fill are inside the ranges given (not the sentinels' business)
        slack = 3
        loff = numpy.zeros(nq + 1, numpy.uint64)
        loff[1:] = numpy.cumsum(counts.astype(numpy.uint64) + slack)
        nb = numpy.full(int(loff[-1]) + 16, SENT_I, numpy.uint32)
        dist = numpy.full(int(loff[-1]) + 16, SENT_F, numpy.float32)
        assert fill(r, loff, nb, dist) == 1
        assert (nb[int(loff[-1]):] == SENT_I).all() and (dist[int(loff[-1]):] == SENT_F).all()
        for i in range(nq):
            lo = int(loff[i])
            assert (nb[lo:lo + counts[i]] == enb[offsets[i]:offsets[i + 1]]).all()
        # device buffers, where the caller's own slots really are next to the ranges: the same three cases
        dev = torch.device("cuda", 0)
        tq = torch.from_numpy(q.copy()).to(dev)

        def dfill(offs, nb, dist):
            toff = torch.from_numpy(offs.astype(numpy.int64)).to(dev)
            return ix.lib.kmamd_knn_index_radius_fill(ix.h, f32p(r), nq, vp(tq.data_ptr()), None, vp(toff.data_ptr()),
                                                      vp(nb.data_ptr()), vp(dist.data_ptr()), 0)

        def dbuffers(size):
            return (torch.full((size,), 0x2BCD1234, dtype=torch.int32, device=dev),
                    torch.full((size,), float(SENT_F), dtype=torch.float32, device=dev))
        tnb, tdist = dbuffers(total + 16)
        assert dfill(u64, tnb, tdist) == 0
        assert (tnb[:total].cpu().numpy().view(numpy.uint32) == enb).all() and (tdist[:total].cpu().numpy() == edist).all()
        assert bool((tnb[total:] == 0x2BCD1234).all()) and bool((tdist[total:] == float(SENT_F)).all())
        tnb, tdist = dbuffers(total + 16)
        assert dfill(bad, tnb, tdist) == 1      # decreasing: the device-side check, before anything is written
        assert bool((tnb == 0x2BCD1234).all()) and bool((tdist == float(SENT_F)).all())
        tnb, tdist = dbuffers(int(soff[-1]) + 16)
        assert dfill(soff, tnb, tdist) == 1     # a smaller radius's ranges: no write outside a query's own range
        hnb, hdist = tnb.cpu().numpy().view(numpy.uint32), tdist.cpu().numpy()
        assert (hnb[:lead] == 0x2BCD1234).all() and (hnb[int(soff[-1]):] == 0x2BCD1234).all()
        assert (hdist[:lead] == SENT_F).all() and (hdist[int(soff[-1]):] == SENT_F).all()
        for i in range(nq):
            lo, n = int(soff[i]), int(scounts[i])
            assert (hnb[lo:lo + n] == enb[offsets[i]:offsets[i] + n]).all(), i
            assert (hdist[lo:lo + n] == edist[offsets[i]:offsets[i] + n]).all(), i
        # bad arguments
        nb, dist = buffers()
        for radius in (-1.0, float("nan"), float("inf")):
            assert fill(radius, u64, nb, dist) == 1
        assert ix.lib.kmamd_knn_index_radius_fill(ix.h, f32p(r), nq, None, None, vp(u64.ctypes.data), vp(nb.ctypes.data), None, -1) == 1
        assert ix.lib.kmamd_knn_index_radius_fill(ix.h, f32p(r), nq, vp(q.ctypes.data), None, None, vp(nb.ctypes.data), None, -1) == 1
        assert ix.lib.kmamd_knn_index_radius_fill(ix.h, f32p(r), nq, vp(q.ctypes.data), None, vp(u64.ctypes.data), None, None, -1) == 1
        assert ix.lib.kmamd_knn_index_radius_count(ix.h, f32p(r), nq, vp(q.ctypes.data), None, None, None, -1) == 1
        assert ix.lib.kmamd_knn_index_radius_count(ix.h, f32p(r), nq, vp(q.ctypes.data), None, vp(nb.ctypes.data), None, 5) == 1
        assert ix.lib.kmamd_knn_index_radius_count(ix.h, f32p(r), 0, None, None, None, None, -1) == 0
        assert (nb == SENT_I).all() and (dist == SENT_F).all()


# ---- 10. the surface ----------------------------------------------------------------------------------------------
def test_surface():
    from kmcuda_amd import KnnIndex, knn_query_radius
    x, c, a, q, dm = truth(N, 64)
    r = radius_for(dm, "L2")
    exp = expected(dm, a, r)
    dev = torch.device("cuda", 0)
    with KnnIndex(x, c, a) as ix:
        base = ix.query_radius(q, r)
        nb_before = ix.query(q, 5)[0]
        again = ix.query_radius(q, r)            # one index, both questions, alternately
        assert (ix.query(q, 5)[0] == nb_before).all()
        counts = ix.query_radius(q, r, count_only=True)
        offs_only, nb_only = ix.query_radius(q, r, return_distances=False)
        srt = ix.query_radius(q, r, sort=True)
        tq = torch.from_numpy(q.copy()).to(dev)
        t = ix.query_radius(tq, r)
        tcounts = ix.query_radius(tq, r, count_only=True)
        tsrt = ix.query_radius(tq, r, sort=True)
        tqa = torch.from_numpy(oracle.lloyd_assign(q, c)[0].astype(numpy.int32)).to(dev)
        t2 = ix.query_radius(tq, r, query_assignments=tqa, return_distances=False)
        empty = ix.query_radius(numpy.zeros((0, 64), numpy.float32), r)
    assert_equals(base, exp)
    assert all((u == v).all() for u, v in zip(again, base))
    assert (counts == numpy.diff(base[0])).all()
    assert (offs_only == base[0]).all() and (nb_only == base[1]).all()
    # sort: every query's slice by (distance, row index)
    qi = numpy.repeat(numpy.arange(len(q)), numpy.diff(base[0]))
    order = numpy.lexsort((base[1], base[2], qi))
    assert (srt[0] == base[0]).all() and (srt[1] == base[1][order]).all() and (srt[2] == base[2][order]).all()
    # device tensors in, device tensors out
    assert all(v.is_cuda for v in t) and tcounts.is_cuda
    assert t[0].dtype == torch.int64 and t[1].dtype == torch.int32 and t[2].dtype == torch.float32
    assert tcounts.dtype == torch.int32
    assert (t[0].cpu().numpy() == base[0]).all() and (t[1].cpu().numpy().view(numpy.uint32) == base[1]).all()
    assert (t[2].cpu().numpy() == base[2]).all() and (tcounts.cpu().numpy().view(numpy.uint32) == counts).all()
    assert (tsrt[1].cpu().numpy().view(numpy.uint32) == srt[1]).all() and (tsrt[2].cpu().numpy() == srt[2]).all()
    assert len(t2) == 2 and (t2[1].cpu().numpy().view(numpy.uint32) == base[1]).all()
    assert empty[0].tolist() == [0] and empty[1].shape == (0,) and empty[2].shape == (0,)
    one_shot = knn_query_radius(r, x, c, a, q)
    assert all((u == v).all() for u, v in zip(one_shot, base))
    assert (knn_query_radius(r, x, c, a, q, count_only=True) == counts).all()
