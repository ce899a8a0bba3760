"""kmeans_predict_top / kmamd_kmeans_assign_top on the GPU against the CPU oracle.

Expected values, built here from the oracle's public functions (the bar is bit equality):
  key        L2: fma_rd(-2, kmo_kahan_dot(x, c), 0 + sum_squares(c)); angular: oracle.distance(x, c, COS)
  qualifies  key < FLT_MAX (a NaN key never does); the order is numpy's stable sort by key = (key, index)
  indices    the first m of that order, K in the slots beyond the qualifying centroids and in every slot of a row whose
             first feature is NaN
  distances  oracle.distance(x, c, metric) per slot as uint32 views, NaN beside K

Under the angular metric the key is the C library's acosf restated on the device, so all of it is bit equal as well;
only where column 0 is compared with kmeans_predict (the device library's acosf) does assert_only_acos_matters apply.
"""
import ctypes

import numpy
import pytest

import oracle
from _angular import assert_only_acos_matters

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_FLT_MAX = numpy.finfo(numpy.float32).max
_F32P = ctypes.POINTER(ctypes.c_float)


def _dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch.device("cuda", 0)


def _metric_id(metric):
    return oracle.COS if metric == "angular" else oracle.L2


def _data(n, d, k, metric, dtype=numpy.float32, seed=None):
    rs = numpy.random.RandomState(n * 7 + d * 3 + k if seed is None else seed)
    x = rs.rand(n, d).astype(numpy.float32)
    c = rs.rand(k, d).astype(numpy.float32)
    take = min(n, k) // 2   # half of the centroids are rows, where there are rows enough
    c[:take] = x[rs.choice(n, take, replace=False)]
    if metric == "angular":
        x /= numpy.linalg.norm(x, axis=1)[:, None]
        c /= numpy.linalg.norm(c, axis=1)[:, None]
    return x.astype(dtype), c.astype(dtype)


def _keys(x32, c32, metric):
    L = oracle.lib()
    n, d = x32.shape
    k = len(c32)
    xp = [ctypes.cast(x32.ctypes.data + 4 * d * i, _F32P) for i in range(n)]
    cp = [ctypes.cast(c32.ctypes.data + 4 * d * j, _F32P) for j in range(k)]
    keys = numpy.empty((n, k), numpy.float32)
    if metric == "angular":
        for i in range(n):
            keys[i] = [L.kmo_distance(oracle.COS, xp[i], cp[j], d) for j in range(k)]
    else:
        cs = [float(numpy.float32(0) + v) for v in oracle.sum_squares(c32)]
        dot, fma = L.kmo_kahan_dot, L.kmo_fma_rd
        for i in range(n):
            keys[i] = [fma(-2.0, dot(xp[i], cp[j], d), cs[j]) for j in range(k)]
    return keys


_expected_cache = {}


def _expected(x, c, metric, key=None):
    """(indices, distances) for m = min(K, 64); a smaller m is the leading columns."""
    if key is not None and key in _expected_cache:
        return _expected_cache[key]
    x32 = numpy.ascontiguousarray(x.astype(numpy.float32))
    c32 = numpy.ascontiguousarray(c.astype(numpy.float32))
    n, k = len(x32), len(c32)
    mm = min(k, 64)
    with numpy.errstate(all="ignore"):
        keys = _keys(x32, c32, metric)
        keys[numpy.isnan(keys) | (keys >= _FLT_MAX)] = numpy.inf
    keys[numpy.isnan(x32[:, 0])] = numpy.inf
    order = numpy.argsort(keys, axis=1, kind="stable")[:, :mm]
    idx = order.astype(numpy.uint32)
    idx[numpy.take_along_axis(keys, order, axis=1) == numpy.inf] = k
    dist = numpy.full((n, mm), numpy.nan, numpy.float32)
    mid = _metric_id(metric)
    for i, j in zip(*numpy.nonzero(idx < k)):
        dist[i, j] = oracle.distance(x32[i], c32[idx[i, j]], mid)
    idx.setflags(write=False)
    dist.setflags(write=False)
    if key is not None:
        _expected_cache[key] = (idx, dist)
    return idx, dist


def _top(x, c, m, metric, **kw):
    from kmcuda_amd import kmeans_predict_top
    return kmeans_predict_top(x, c, m, metric=metric, **kw)


def _bits(a):
    return numpy.ascontiguousarray(numpy.asarray(a)).view(numpy.uint32)


def _same(got, want):
    return (numpy.asarray(got[0]) == numpy.asarray(want[0])).all() and (_bits(got[1]) == _bits(want[1])).all()


def _check(got, x, c, m, metric, key=None, what=""):
    idx, dist = (numpy.asarray(v) for v in got)
    ref_i, ref_d = _expected(x, c, metric, key)
    ref_i, ref_d = ref_i[:, :m], ref_d[:, :m]
    assert idx.dtype == numpy.uint32 and dist.dtype == numpy.float32
    assert idx.shape == ref_i.shape and dist.shape == ref_d.shape
    bad_i = numpy.nonzero((idx != ref_i).any(axis=1))[0]
    bad_d = numpy.nonzero((_bits(dist) != _bits(ref_d)).any(axis=1))[0]
    print("%s %s m=%d: %d of %d rows differ in an index, %d in a distance" % (what, metric, m, bad_i.size, len(idx),
                                                                             bad_d.size))
    assert bad_i.size == 0, (what, m, bad_i[:4], idx[bad_i[:4]], ref_i[bad_i[:4]])
    assert bad_d.size == 0, (what, m, bad_d[:4], dist[bad_d[:4]], ref_d[bad_d[:4]])
    return idx, dist


def _ms(k):
    return sorted({1, min(2, k), min(5, k), min(k, 64)})


# ---------------------------------------------------------------------------------------------------------------
# 1. shapes: D reaches the scalar row loads (6), a full filter width (32), padded ones (36, 100), the register filter's
#    edge (256) and the exact-only width (320); N one row, under / over one 128-row block, many blocks; K below one
#    32-centroid tile, and more than a lane's 64
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [numpy.float32, numpy.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("metric", ["L2", "angular"])
@pytest.mark.parametrize("d", [6, 32, 36, 100, 256, 320])
def test_sweep_over_features(d, metric, dtype):
    x, c = _data(1000, d, 16, metric, dtype)
    key = ("features", d, metric, numpy.dtype(dtype).name)
    for m in _ms(16):
        _check(_top(x, c, m, metric), x, c, m, metric, key, "1000x%d K=16 %s" % (d, numpy.dtype(dtype).name))


@pytest.mark.parametrize("dtype", [numpy.float32, numpy.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("metric", ["L2", "angular"])
@pytest.mark.parametrize("k", [2, 16, 300])
@pytest.mark.parametrize("n", [1, 127, 129, 1000])
def test_sweep_over_rows_and_clusters(n, k, metric, dtype):
    x, c = _data(n, 36, k, metric, dtype)
    key = ("rows", n, k, metric, numpy.dtype(dtype).name)
    for m in _ms(k):
        _check(_top(x, c, m, metric), x, c, m, metric, key, "%dx36 K=%d %s" % (n, k, numpy.dtype(dtype).name))


def test_no_rows():
    _, c = _data(10, 36, 4, "L2")
    idx, dist = _top(numpy.zeros((0, 36), numpy.float32), c, 3, "L2")
    assert idx.shape == (0, 3) and dist.shape == (0, 3)
    assert idx.dtype == numpy.uint32 and dist.dtype == numpy.float32


# ---------------------------------------------------------------------------------------------------------------
# 2. column 0 is kmeans_predict's assignment; m = 1 is kmeans_predict with distances
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "angular"])
@pytest.mark.parametrize("d", [36, 320])
def test_column_0_is_kmeans_predict(d, metric):
    from kmcuda_amd import kmeans_predict
    x, c = _data(1000, d, 40, metric)
    x[17, 0] = numpy.nan
    c[3, 1] = numpy.nan
    a, dist = kmeans_predict(x, c, metric=metric, return_distances=True)
    idx, _ = _top(x, c, 5, metric)
    one_i, one_d = _top(x, c, 1, metric)
    assert one_i.shape == (1000, 1) and (one_i[:, 0] == idx[:, 0]).all()
    if metric == "angular":
        differ = assert_only_acos_matters(x, c, a, idx[:, 0], what="column 0 against kmeans_predict")
        print("angular: %d rows differ from kmeans_predict by the acosf" % differ)
    else:
        assert (idx[:, 0] == a).all()
    same = idx[:, 0] == a
    assert (_bits(one_d[:, 0])[same] == _bits(dist)[same]).all()
    assert idx[17, 0] == 40 and numpy.isnan(one_d[17, 0])


# ---------------------------------------------------------------------------------------------------------------
# 3. edge rows and edge centroids, mid-block and as the very last row
# ---------------------------------------------------------------------------------------------------------------
_N_EDGE, _K_EDGE, _M_EDGE = 300, 12, 4


@pytest.mark.parametrize("d", [36, 320], ids=["filtered", "exact_only"])
@pytest.mark.parametrize("metric", ["L2", "angular"])
@pytest.mark.parametrize("where", ["mid", "last"])
@pytest.mark.parametrize("kind", ["nan_first", "nan_later", "equals_centroid", "nan_centroid", "few_finite_centroids",
                                  "overflowing_centroid", "duplicates_in_top", "duplicates_straddle_m",
                                  "coincident_centroids", "one_float_apart"])
def test_edges(kind, where, metric, d):
    n, k, m = _N_EDGE, _K_EDGE, _M_EDGE
    x, c = _data(n, d, k, metric, seed=11)
    row = 70 if where == "mid" else n - 1
    ref0_i, _ = _expected(x, c, metric, ("edges", d, metric))
    near = ref0_i[row].astype(numpy.int64)   # the row's centroids, nearest first, before the edit
    if kind == "nan_first":
        x[row, 0] = numpy.nan
    elif kind == "nan_later":
        x[row, d - 1] = numpy.nan
    elif kind == "equals_centroid":
        x[row] = c[near[2]]
    elif kind == "nan_centroid":
        c[near[1], d // 2] = numpy.nan
    elif kind == "few_finite_centroids":
        c[[j for j in range(k) if j not in (near[0], near[5])], 3] = numpy.nan   # 2 < m qualify
    elif kind == "overflowing_centroid":
        if metric == "L2":
            c[near[0]] = 3e19   # its squared norm, and so its key, overflows: it never qualifies
        else:
            c[near[0], 0] = numpy.inf
            c[near[1], 0] = -numpy.inf
    elif kind == "duplicates_in_top":
        lo, hi = sorted((near[1], near[6]))
        c[hi] = c[near[1]]
        c[lo] = c[hi]
    elif kind == "duplicates_straddle_m":
        js = sorted((near[m - 1], near[8], near[10]))   # three copies of the m-th nearest: ranks m-1, m, m+1
        src = c[near[m - 1]].copy()
        c[js] = src
    elif kind == "coincident_centroids":
        js = sorted((near[3], near[7], near[9]))
        x[row] = c[near[3]]
        c[js] = x[row]   # angular: products >= 1 (or the same product) -- the lowest index first
    elif kind == "one_float_apart":
        c[near[4]] = numpy.nextafter(c[near[0]], numpy.float32(2), dtype=numpy.float32)

    idx, dist = _check(_top(x, c, m, metric), x, c, m, metric, what="%s %s D=%d" % (kind, where, d))
    if kind in ("nan_first", "nan_later"):
        assert (idx[row] == k).all() and numpy.isnan(dist[row]).all()
    elif kind == "equals_centroid":
        assert idx[row, 0] == near[2] or metric == "angular"
        if metric == "L2":
            assert dist[row, 0] == 0.0
    elif kind == "nan_centroid":
        assert not (idx == near[1]).any()
    elif kind == "few_finite_centroids":
        assert (idx[:, 2:] == k).all() and numpy.isnan(dist[:, 2:]).all() and (idx[:, :2] < k).all()
    elif kind == "overflowing_centroid" and metric == "L2":
        assert not (idx == near[0]).any()
    elif kind == "duplicates_in_top":
        at = list(idx[row])
        assert at.index(lo) + 1 == at.index(hi)
    elif kind == "duplicates_straddle_m":
        assert idx[row, m - 1] == js[0] and js[1] not in idx[row] and js[2] not in idx[row]
    elif kind == "coincident_centroids":
        assert list(idx[row, :3]) == js
        assert (dist[row, :3] == 0.0).all() or metric == "angular"


# ---------------------------------------------------------------------------------------------------------------
# 4. paths and chunks give the same bits
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", [("KMCUDA_AMD_ASSIGN_TOP", "exact"), ("KMCUDA_AMD_FILTER", "f32")],
                         ids=["exact", "filter_f32"])
@pytest.mark.parametrize("metric", ["L2", "angular"])
@pytest.mark.parametrize("d", [36, 256])
def test_paths_give_the_same_bits(d, metric, switch, monkeypatch):
    x, c = _data(1000, d, 70, metric)
    x[17, 0] = numpy.nan
    x[18, 5] = numpy.nan
    c[9] = c[4]
    default = _top(x, c, 8, metric)
    monkeypatch.setenv(*switch)
    assert _same(_top(x, c, 8, metric), default)


@pytest.mark.parametrize("surface", ["numpy", "torch"])
@pytest.mark.parametrize("dtype", [numpy.float32, numpy.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("chunk", [1000, 999])
def test_chunks(chunk, dtype, surface, monkeypatch):
    x, c = _data(2500, 36, 16, "L2", dtype)
    if surface == "torch":
        xin, cin = torch.from_numpy(x).to(_dev()), torch.from_numpy(c).to(_dev())
    else:
        xin, cin = x, c

    def run():
        out = _top(xin, cin, 5, "L2")
        if surface == "torch":
            assert out[0].dtype == torch.int32 and out[1].dtype == torch.float32 and out[0].device == _dev()
            out = (out[0].cpu().numpy().view(numpy.uint32), out[1].cpu().numpy())
        return out
    key = ("chunks", numpy.dtype(dtype).name)
    whole = _check(run(), x, c, 5, "L2", key, "unchunked")
    monkeypatch.setenv("KMCUDA_AMD_ASSIGN_CHUNK", str(chunk))
    assert _same(run(), whole)
    monkeypatch.setenv("KMCUDA_AMD_ASSIGN_TOP_ROWS", "300")   # 384-row score matrices: three per chunk, the last short
    assert _same(run(), whole)


def test_misaligned_device_view():
    x, c = _data(1001, 6, 16, "L2")
    dev = _dev()
    xs = torch.from_numpy(x).to(dev)[1:]
    assert xs.data_ptr() % 16 != 0 and xs.is_contiguous()
    idx, dist = _top(xs, torch.from_numpy(c).to(dev), 3, "L2")
    _check((idx.cpu().numpy().view(numpy.uint32), dist.cpu().numpy()), x[1:], c, 3, "L2", what="x[1:] D=6")
    only = _top(xs, torch.from_numpy(c).to(dev), 3, "L2", return_distances=False)
    assert only.dtype == torch.int32 and (only == idx).all()


# ---------------------------------------------------------------------------------------------------------------
# 5. the filter filters: by its own bound E ~ 6e-8 (D + 8) mass ~ 1e-2 against key gaps in the hundreds, the contenders
#    of a row are about m; the cap K / 2 is a condition, not a measurement
# ---------------------------------------------------------------------------------------------------------------
def _stats():
    from kmcuda_amd import _lib
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert _lib.lib().kmamd_assign_top_stats(ctypes.byref(a), ctypes.byref(b)) == 0
    return a.value, b.value


def test_the_filter_filters(monkeypatch):
    rs = numpy.random.RandomState(5)
    k, d, n, m = 64, 32, 4096, 4
    c = (10.0 * rs.randn(k, d)).astype(numpy.float32)
    x = (c[rs.randint(0, k, n)] + 0.5 * rs.randn(n, d)).astype(numpy.float32)
    default = _top(x, c, m, "L2")
    exact, total = _stats()
    print("filtered: %d exact keys of %d pairs (%.4f)" % (exact, total, exact / total))
    assert total == n * k
    assert n * m <= exact <= total // 2
    monkeypatch.setenv("KMCUDA_AMD_ASSIGN_TOP", "exact")
    assert _same(_top(x, c, m, "L2"), default)
    exact, total = _stats()
    assert exact == total == n * k


# ---------------------------------------------------------------------------------------------------------------
# 6. the raw C call with device pointers, a round trip with kmeans_cuda, repeatability
# ---------------------------------------------------------------------------------------------------------------
def test_raw_c_call_with_device_pointers():
    from kmcuda_amd import _lib
    L = _lib.lib()
    dev = _dev()
    n, d, k, m = 1000, 36, 16, 3
    x, c = _data(n, d, k, "L2")
    xs, cs = torch.from_numpy(x).to(dev), torch.from_numpy(c).to(dev)
    top = torch.full((n, m), -1, dtype=torch.int32, device=dev)
    dist = torch.full((n, m), -1.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    rc = L.kmamd_kmeans_assign_top(0, n, d, k, m, 0, 0, 0, 0, xs.data_ptr(), cs.data_ptr(), top.data_ptr(),
                                   dist.data_ptr())
    assert rc == 0
    _check((top.cpu().numpy().view(numpy.uint32), dist.cpu().numpy()), x, c, m, "L2", what="raw call")
    # without distances; then a device other than the buffers': refused, outputs untouched
    top2 = torch.full((n, m), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert L.kmamd_kmeans_assign_top(0, n, d, k, m, 0, 0, 0, 0, xs.data_ptr(), cs.data_ptr(), top2.data_ptr(),
                                     None) == 0
    assert (top2 == top).all()
    top3 = torch.full((n, m), -1, dtype=torch.int32, device=dev)
    assert L.kmamd_kmeans_assign_top(0, n, d, k, m, 0, 1, 0, 0, xs.data_ptr(), cs.data_ptr(), top3.data_ptr(),
                                     None) == 1
    assert (top3 == -1).all()


def test_round_trip_with_kmeans_cuda():
    from kmcuda_amd import kmeans_cuda, kmeans_predict
    rs = numpy.random.RandomState(41)
    x = (rs.rand(3000, 32) + (rs.randint(0, 8, 3000)[:, None] * 2.0)).astype(numpy.float32)
    cen, asg = kmeans_cuda(x, 20, init="random", yinyang_t=0, tolerance=0, seed=3, device=1)
    idx, dist = _top(x, cen, 2, "L2")
    agree = kmeans_predict(x, cen) == asg
    assert agree.all()
    assert (idx[agree, 0] == asg[agree]).all()
    assert (idx[:, 1] != idx[:, 0]).all() and (idx[:, 1] < 20).all()


@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_two_identical_calls_give_identical_bits(metric):
    x, c = _data(3000, 100, 300, metric)
    assert _same(_top(x, c, 8, metric), _top(x, c, 8, metric))
