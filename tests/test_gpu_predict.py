"""kmeans_predict / kmamd_kmeans_assign on the GPU against the CPU oracle.

Expected values (the bar is bit equality, except the fp64 sums):
  assignments  oracle.lloyd_assign(x, c, assignments=full(n, K)): one reference pass from "no cluster"
  distances    oracle.distance(x[i], c[a[i]]) per row as uint32 views, NaN where a[i] == K
  counts       numpy.bincount over a < K
  sums         within members * 2^-52 relative of math.fsum over the returned distances (all terms are non-negative:
               the standard bound of an fp64 sum in any order), and bit-equal between two identical calls

Under the angular metric the oracle takes libm's acosf; the device's distance pass restates that function operation for
operation (acosf_fdlibm, csrc/exact.hpp), so the bar is bit equality there too.
"""
import ctypes
import math

import numpy
import pytest

import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch.device("cuda", 0)


def _metric_id(metric):
    return oracle.COS if metric == "angular" else oracle.L2


def _data(n, d, k, metric, dtype=numpy.float32, seed=None):
    rs = numpy.random.RandomState(n * 7 + d * 3 + k if seed is None else seed)
    x = rs.rand(n, d).astype(numpy.float32)
    if metric == "angular":
        x /= numpy.linalg.norm(x, axis=1)[:, None]
    c = x[rs.choice(n, k, replace=n < k)].copy()
    if n < k:   # (more centroids than rows: distinct centroids all the same)
        c = rs.rand(k, d).astype(numpy.float32)
        if metric == "angular":
            c /= numpy.linalg.norm(c, axis=1)[:, None]
    return x.astype(dtype), c.astype(dtype)


_expected_cache = {}


def _expected(x, c, metric, key=None):
    """(assignments, distances) of the oracle for the values x / c hold (halves widened exactly)."""
    if key is not None and key in _expected_cache:
        return _expected_cache[key]
    x32, c32 = x.astype(numpy.float32), c.astype(numpy.float32)
    n, k, m = len(x32), len(c32), _metric_id(metric)
    a, _, _ = oracle.lloyd_assign(x32, c32, assignments=numpy.full(n, k, numpy.uint32), metric=m)
    d = numpy.full(n, numpy.nan, numpy.float32)
    for i in numpy.nonzero(a < k)[0]:
        d[i] = oracle.distance(x32[i], c32[a[i]], m)
    a.setflags(write=False)
    d.setflags(write=False)
    if key is not None:
        _expected_cache[key] = (a, d)
    return a, d


def _check(got, x, c, metric, key=None, what="", then=None):
    """then(a, d, counts, sums): the caller's own assertions, run in front of the last check here."""
    a, d, (counts, sums) = got
    k = len(c)
    ref_a, ref_d = _expected(x, c, metric, key)
    a, d, counts, sums = (numpy.asarray(v) for v in (a, d, counts, sums))
    assert a.dtype == numpy.uint32 and d.dtype == numpy.float32 and counts.dtype == numpy.uint32
    assert sums.dtype == numpy.float64
    bad_a = numpy.nonzero(a != ref_a)[0]
    has = ref_a < k
    bits, ref_bits = d.view(numpy.uint32)[has].astype(numpy.int64), ref_d.view(numpy.uint32)[has].astype(numpy.int64)
    bad_d = numpy.nonzero(bits != ref_bits)[0]
    print("%s %s: %d of %d assignments and %d of %d distances differ from the oracle (by at most %d in the last place)"
          % (what, metric, bad_a.size, len(a), bad_d.size, int(has.sum()),
             int(numpy.abs(bits - ref_bits).max()) if bits.size else 0))
    assert bad_a.size == 0, (what, bad_a[:8], a[bad_a[:8]], ref_a[bad_a[:8]])
    assert numpy.isnan(d[~has]).all()
    assert (counts == numpy.bincount(a[a < k], minlength=k)).all()
    _check_sums(a, d, counts, sums, k)
    if then is not None:
        then(a, d, counts, sums)
    assert bad_d.size == 0, (what, bad_d[:8], d[has][bad_d[:8]], ref_d[has][bad_d[:8]])
    return a, d, counts, sums


def _check_sums(a, d, counts, sums, k):
    order = numpy.argsort(a, kind="stable")
    bounds = numpy.searchsorted(a[order], numpy.arange(k + 1))
    for cl in range(k):
        members = d[order[bounds[cl]:bounds[cl + 1]]]
        exact = math.fsum(float(v) for v in members)
        assert len(members) == counts[cl]
        if len(members) == 0:
            assert sums[cl] == 0.0 and not numpy.signbit(sums[cl])
        else:
            assert abs(sums[cl] - exact) <= len(members) * 2.0 ** -52 * exact, (cl, sums[cl], exact)


def _predict(x, c, metric):
    from kmcuda_amd import kmeans_predict
    return kmeans_predict(x, c, metric=metric, return_distances=True, return_cluster_stats=True)


def _same(got, want):
    """Two results of kmeans_predict(..., True, True), bit for bit (NaN distances compare as bits too)."""
    a, d, (cn, sm) = (got[0], got[1], got[2])
    a2, d2, (cn2, sm2) = (want[0], want[1], want[2])
    return ((numpy.asarray(a) == numpy.asarray(a2)).all()
            and (numpy.asarray(d).view(numpy.uint32) == numpy.asarray(d2).view(numpy.uint32)).all()
            and (numpy.asarray(cn) == numpy.asarray(cn2)).all()
            and (numpy.asarray(sm).view(numpy.uint64) == numpy.asarray(sm2).view(numpy.uint64)).all())


# ---------------------------------------------------------------------------------------------------------------
# 1. shapes: D reaches the fallback path (6), one exact 32-feature chunk, a partial last chunk (36, 100), the
#    register filter's edge (256) and the wide filter (320); N one row, under / over one 128-row block, many blocks
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [numpy.float32, numpy.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("metric", ["L2", "angular"])
@pytest.mark.parametrize("d", [6, 32, 36, 100, 256, 320])
def test_sweep_over_features(d, metric, dtype):
    x, c = _data(1000, d, 16, metric, dtype)
    got = _predict(x, c, metric)

    def again(*_):   # two identical calls: identical bits, the sums included
        assert _same(_predict(x, c, metric), got)
    _check(got, x, c, metric, what="1000x%d K=16 %s" % (d, numpy.dtype(dtype).name), then=again)


@pytest.mark.parametrize("dtype", [numpy.float32, numpy.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("metric", ["L2", "angular"])
@pytest.mark.parametrize("k", [2, 16, 300])
@pytest.mark.parametrize("n", [1, 127, 129, 1000])
def test_sweep_over_rows_and_clusters(n, k, metric, dtype):
    x, c = _data(n, 36, k, metric, dtype)
    _check(_predict(x, c, metric), x, c, metric, what="%dx36 K=%d %s" % (n, k, numpy.dtype(dtype).name))


def test_no_rows():
    from kmcuda_amd import kmeans_predict
    _, c = _data(10, 36, 4, "L2")
    a, d, (counts, sums) = kmeans_predict(numpy.zeros((0, 36), numpy.float32), c, return_distances=True,
                                          return_cluster_stats=True)
    assert a.shape == (0,) and d.shape == (0,) and (counts == 0).all() and (sums == 0.0).all()


# ---------------------------------------------------------------------------------------------------------------
# 2. edge rows and edge centroids, mid-block and as the very last row / centroid
# ---------------------------------------------------------------------------------------------------------------
_N_EDGE, _K_EDGE = 300, 12


def _far_centroid(d, metric, j=0):
    """A centroid no row of _data() is nearest to."""
    if metric == "angular":
        v = -numpy.ones(d, numpy.float32)
        v[j % d] = -2.0
        return v / numpy.linalg.norm(v)
    return numpy.full(d, 1e3 + j, numpy.float32)


@pytest.mark.parametrize("d", [36, 6], ids=["tiled", "fallback"])
@pytest.mark.parametrize("metric", ["L2", "angular"])
@pytest.mark.parametrize("where", ["mid", "last"])
@pytest.mark.parametrize("kind", ["nan_first", "nan_later", "equals_centroid", "nan_centroid", "duplicate_centroids",
                                  "empty_cluster"])
def test_edges(kind, where, metric, d):
    n, k = _N_EDGE, _K_EDGE
    x, c = _data(n, d, k, metric, seed=11)
    row = 70 if where == "mid" else n - 1
    cen = 5 if where == "mid" else k - 1
    if kind == "nan_first":
        x[row, 0] = numpy.nan
    elif kind == "nan_later":
        x[row, d - 1] = numpy.nan
    elif kind == "equals_centroid":
        x[row] = c[cen]
    elif kind == "nan_centroid":
        c[cen, d // 2] = numpy.nan
    elif kind == "duplicate_centroids":
        c[cen] = c[2]
        x[row] = c[2]
    elif kind == "empty_cluster":
        c[cen] = _far_centroid(d, metric)

    def then(a, dist, counts, sums):
        if kind in ("nan_first", "nan_later"):
            assert a[row] == k and numpy.isnan(dist[row]) and counts.sum() == n - 1
        elif kind == "equals_centroid":
            assert a[row] == cen
            if metric == "L2":
                assert dist[row] == 0.0
        elif kind == "nan_centroid":
            assert counts[cen] == 0 and sums[cen] == 0.0 and not (a == cen).any() and counts.sum() == n
        elif kind == "duplicate_centroids":
            assert a[row] == 2 and counts[cen] == 0 and not (a == cen).any()   # the lower index wins
            if metric == "L2":
                assert dist[row] == 0.0
        elif kind == "empty_cluster":
            assert counts[cen] == 0 and sums[cen] == 0.0 and counts.sum() == n
    _check(_predict(x, c, metric), x, c, metric, what="%s %s D=%d" % (kind, where, d), then=then)


@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_all_rows_in_one_cluster(metric):
    n, d, k = _N_EDGE, 36, _K_EDGE
    x, c = _data(n, d, k, metric, seed=13)
    for j in range(k):
        if j != 4:
            c[j] = _far_centroid(d, metric, j)

    def then(a, _d, counts, _s):
        assert (a == 4).all() and counts[4] == n and counts.sum() == n
    _check(_predict(x, c, metric), x, c, metric, what="one cluster", then=then)


# ---------------------------------------------------------------------------------------------------------------
# 3. chunking: 2001 rows in chunks of 1000 (a 1-row tail) and 999 (a 3-row tail)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("surface", ["numpy", "torch"])
@pytest.mark.parametrize("dtype", [numpy.float32, numpy.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("chunk", [1000, 999])
def test_chunks(chunk, dtype, surface, monkeypatch):
    x, c = _data(2001, 36, 16, "L2", dtype)
    if surface == "torch":
        xin, cin = torch.from_numpy(x).to(_dev()), torch.from_numpy(c).to(_dev())
    else:
        xin, cin = x, c

    def run():
        out = _predict(xin, cin, "L2")
        if surface == "torch":
            out = (out[0].cpu().numpy().view(numpy.uint32), out[1].cpu().numpy(),
                   (out[2][0].cpu().numpy().view(numpy.uint32), out[2][1].cpu().numpy()))
        return out
    whole = run()
    key = ("chunks", numpy.dtype(dtype).name)
    _check(whole, x, c, "L2", key=key, what="unchunked")
    monkeypatch.setenv("KMCUDA_AMD_ASSIGN_CHUNK", str(chunk))
    parts = run()
    a, dist, counts, sums = _check(parts, x, c, "L2", key=key, what="chunks of %d" % chunk)
    assert (a == whole[0]).all() and (dist.view(numpy.uint32) == whole[1].view(numpy.uint32)).all()
    assert (counts == whole[2][0]).all()
    assert _same(run(), parts)


# ---------------------------------------------------------------------------------------------------------------
# 4. paths: the f32 filter and the per-thread distance kernel give the default's bits
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", [("KMCUDA_AMD_FILTER", "f32"), ("KMCUDA_AMD_ASSIGN_DIST", "member")],
                         ids=["filter_f32", "dist_member"])
@pytest.mark.parametrize("metric", ["L2", "angular"])
@pytest.mark.parametrize("d", [36, 256])
def test_paths_give_the_same_bits(d, metric, switch, monkeypatch):
    x, c = _data(1000, d, 16, metric)
    x[17, 0] = numpy.nan   # a row without a cluster on every path
    default = _predict(x, c, metric)
    monkeypatch.setenv(*switch)
    assert _same(_predict(x, c, metric), default)


def test_distance_kernels_agree_on_any_assignment():
    """kmamd_assigned_distances: the tiled kernel and member_distances_kernel on assignments that are NOT the nearest
    centroids, with ids >= K (no centroid read, NaN) among them -- the same bits, and the oracle's."""
    import os
    from kmcuda_amd import _lib
    L = _lib.lib()
    dev = _dev()
    n, d, k = 700, 100, 9
    rs = numpy.random.RandomState(3)
    a = rs.randint(0, k, n).astype(numpy.uint32)
    a[[0, 127, 128, 300, n - 1]] = [k, k + 1, 0xFFFFFFFF, k, k]
    x2, c2 = _data(n, d, k, "L2", seed=29)
    # angular: unit rows at cosines spread over (-1, 1) from their centroid, a few at its very ends (both clamps and
    # all three branches of acosf)
    c1 = rs.randn(k, d)
    c1 /= numpy.linalg.norm(c1, axis=1)[:, None]
    u = rs.randn(n, d)
    own = c1[a % k]
    u -= (u * own).sum(axis=1)[:, None] * own
    u /= numpy.linalg.norm(u, axis=1)[:, None]
    t = rs.uniform(-1.0, 1.0, n)
    t[5:9] = [1.0, -1.0, 1.0 - 1e-7, -1.0 + 1e-7]
    x1 = (t[:, None] * own + numpy.sqrt(1.0 - t * t)[:, None] * u).astype(numpy.float32)
    c1 = c1.astype(numpy.float32)
    asg = torch.from_numpy(a.view(numpy.int32)).to(dev)
    for metric, x, c in ((0, x2, c2), (1, x1, c1)):
        xs, cs = torch.from_numpy(x).to(dev), torch.from_numpy(c).to(dev)
        outs = []
        for member in (False, True):
            if member:
                os.environ["KMCUDA_AMD_ASSIGN_DIST"] = "member"
            try:
                dist = torch.full((n,), -1.0, dtype=torch.float32, device=dev)
                torch.cuda.synchronize()
                rc = L.kmamd_assigned_distances(metric, n, d, k, 0, xs.data_ptr(), cs.data_ptr(), asg.data_ptr(),
                                                dist.data_ptr(), None)
                assert rc == 0
                torch.cuda.synchronize()
            finally:
                os.environ.pop("KMCUDA_AMD_ASSIGN_DIST", None)
            outs.append(dist.cpu().numpy())
        new, old = outs
        assert (new.view(numpy.uint32) == old.view(numpy.uint32)).all()
        assert numpy.isnan(new[a >= k]).all() and not numpy.isnan(new[a < k]).any()
        ref = numpy.array([oracle.distance(x[i], c[a[i]], metric) if a[i] < k else numpy.nan for i in range(n)],
                          numpy.float32)
        assert (new.view(numpy.uint32)[a < k] == ref.view(numpy.uint32)[a < k]).all()
        if metric == 1:   # the data does reach every branch
            has = a < k
            assert (ref[has] < 1.0).any() and (ref[has] > 2.2).any() and ((ref[has] > 1.1) & (ref[has] < 2.0)).any()


# ---------------------------------------------------------------------------------------------------------------
# 5. surfaces
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [numpy.float32, numpy.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_torch_in_torch_out(metric, dtype):
    x, c = _data(1000, 36, 16, metric, dtype)
    x[999, 0] = numpy.nan
    ref = _predict(x, c, metric)
    dev = _dev()
    a, d, (counts, sums) = _predict(torch.from_numpy(x).to(dev), torch.from_numpy(c).to(dev), metric)
    for t, dt in ((a, torch.int32), (d, torch.float32), (counts, torch.int32), (sums, torch.float64)):
        assert t.dtype == dt and t.device == dev
    got = (a.cpu().numpy().view(numpy.uint32), d.cpu().numpy(),
           (counts.cpu().numpy().view(numpy.uint32), sums.cpu().numpy()))
    assert _same(got, ref)
    assert int(a[999]) == 16
    from kmcuda_amd import kmeans_predict
    only = kmeans_predict(torch.from_numpy(x).to(dev), torch.from_numpy(c).to(dev), metric=metric)
    assert only.dtype == torch.int32 and (only == a).all()


def test_misaligned_device_view():
    x, c = _data(1001, 6, 16, "L2")
    dev = _dev()
    xs = torch.from_numpy(x).to(dev)[1:]
    assert xs.data_ptr() % 16 != 0 and xs.is_contiguous()
    a, d, (counts, sums) = _predict(xs, torch.from_numpy(c).to(dev), "L2")
    got = (a.cpu().numpy().view(numpy.uint32), d.cpu().numpy(),
           (counts.cpu().numpy().view(numpy.uint32), sums.cpu().numpy()))
    _check(got, x[1:], c, "L2", what="x[1:] D=6")


def test_raw_c_call_with_device_pointers():
    from kmcuda_amd import _lib
    L = _lib.lib()
    dev = _dev()
    n, d, k = 1000, 36, 16
    x, c = _data(n, d, k, "L2")
    ref_a, ref_d = _expected(x, c, "L2")
    xs, cs = torch.from_numpy(x).to(dev), torch.from_numpy(c).to(dev)
    asg = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rc = L.kmamd_kmeans_assign(0, n, d, k, 0, 0, 0, 0, xs.data_ptr(), cs.data_ptr(), asg.data_ptr(), None, None, None)
    assert rc == 0
    assert (asg.cpu().numpy().view(numpy.uint32) == ref_a).all()
    # only the sums: the distances are computed in chunk scratch
    asg2 = torch.full((n,), -1, dtype=torch.int32, device=dev)
    sums = torch.full((k,), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    rc = L.kmamd_kmeans_assign(0, n, d, k, 0, 0, 0, 0, xs.data_ptr(), cs.data_ptr(), asg2.data_ptr(), None, None,
                               sums.data_ptr())
    assert rc == 0
    a = asg2.cpu().numpy().view(numpy.uint32)
    assert (a == ref_a).all()
    _check_sums(a, numpy.asarray(ref_d), numpy.bincount(a[a < k], minlength=k), sums.cpu().numpy(), k)
    # a device other than the buffers': refused
    assert L.kmamd_kmeans_assign(0, n, d, k, 0, 1, 0, 0, xs.data_ptr(), cs.data_ptr(), asg2.data_ptr(), None, None,
                                 None) == 1
    assert isinstance(ctypes.c_void_p(xs.data_ptr()).value, int)


# ---------------------------------------------------------------------------------------------------------------
# 6. round trip: a run that stopped with 0 reassignments -- a further pass changes nothing
# ---------------------------------------------------------------------------------------------------------------
def test_round_trip_with_kmeans_cuda():
    from kmcuda_amd import kmeans_cuda, kmeans_predict
    rs = numpy.random.RandomState(41)
    x = (rs.rand(3000, 32) + (rs.randint(0, 8, 3000)[:, None] * 2.0)).astype(numpy.float32)
    cen, asg = kmeans_cuda(x, 20, init="random", yinyang_t=0, tolerance=0, seed=3, device=1)
    got = kmeans_predict(x, cen)
    assert (got == asg).all()
