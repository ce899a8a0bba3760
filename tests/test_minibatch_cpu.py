"""Mini-batch K-means without a device: the restatement's exactness assertion on the grid fixtures, the draw's index
arithmetic, and the refusals of the kmamd_minibatch_* entry points that come before any device work -- InvalidArguments,
the handle left null, the outputs byte for byte what they were (on a machine without a device any answer that came
after a device call would be NoSuchDevice).  Only refused calls are issued here."""
import ctypes

import numpy
import pytest

import _minibatch_ref as ref
from _seed_parallel_ref import hash64

_SENTINEL = 0x5A5A5A5A
_K, _D, _N = 4, 8, 64


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("shape", ref.GRID_SHAPES, ids=["%dx%d-k%d" % s for s in ref.GRID_SHAPES])
def test_grid_fixture_sums_do_not_depend_on_their_order(shape, weighted):
    """step(exact=True) asserts fsum == forward sum == reverse sum for every cluster, feature and step."""
    res = ref.grid_restated(*shape, weighted)
    n, d, k = shape
    assert len(res) == ref.STEPS
    for r in res:
        assert r["centroids"].shape == (k, d) and r["centroids"].dtype == numpy.float32
        assert len(r["assignments"]) == n and (r["assignments"] < k).all()
    _, _, weights = ref.grid(*shape, weighted)
    total = sum(float(w.sum()) for w in weights) if weighted else float(ref.STEPS * n)
    assert res[-1]["weights"].sum() == total


def _mulhi_limbs(h, n):
    """The high 64 bits of h * n from 32-bit limbs (no integer wider than 64 bits + carries)."""
    m = 0xFFFFFFFF
    h0, h1, n0, n1 = h & m, h >> 32, n & m, n >> 32
    ll, lh, hl, hh = h0 * n0, h0 * n1, h1 * n0, h1 * n1
    mid = (ll >> 32) + (lh & m) + (hl & m)
    return hh + (lh >> 32) + (hl >> 32) + (mid >> 32)


@pytest.mark.parametrize("n", [1, 5003, 2 ** 32 - 1])
def test_draw_indices(n):
    for seed, t in ((0, 0), (7, 3), (0xFFFFFFFF, 0xFFFFFFFF), (12345, 1 << 20)):
        rows = ref.draw(seed, t, 300, n)
        direct = [_mulhi_limbs(hash64(seed, t, j), n) for j in range(300)]
        assert rows.tolist() == direct
        assert ((rows >= 0) & (rows < n)).all()
        if n == 1:
            assert not rows.any()
    # the counter enters as 32 bits, and the slots of a step differ
    assert (ref.draw(3, (1 << 32) + 5, 50, 5003) == ref.draw(3, 5, 50, 5003)).all()
    if n > 1:
        assert len(set(ref.draw(3, 5, 300, n).tolist())) > 1


def _built():
    import __graft_entry__
    __graft_entry__.build()
    from kmcuda_amd import _lib
    return _lib.lib()


# (what is wrong, the arguments that differ from a valid host call)
_CREATE = [
    ("metric 2", dict(metric=2)),
    ("D = 0", dict(d=0)),
    ("D = 65536", dict(d=65536)),
    ("K = 1", dict(k=1)),
    ("K = 0", dict(k=0)),
    ("device = -1", dict(device=-1)),
    ("device_ptrs != device", dict(device=0, device_ptrs=1)),
    ("null centroids", dict(centroids=None)),
    ("negative cluster weight", dict(cw=[1.0, -1.0, 0.0, 2.0])),
    ("NaN cluster weight", dict(cw=[1.0, float("nan"), 0.0, 2.0])),
    ("infinite cluster weight", dict(cw=[1.0, float("inf"), 0.0, 2.0])),
]


@pytest.mark.parametrize("what,over", _CREATE, ids=[row[0] for row in _CREATE])
def test_create_refused_before_any_device_call(what, over):
    L = _built()
    a = dict(metric=0, d=_D, k=_K, device=0, device_ptrs=-1, cw=None)
    a.update(over)
    c = numpy.random.default_rng(5).standard_normal((_K, _D)).astype(numpy.float32)
    cw = None if a["cw"] is None else numpy.array(a["cw"], numpy.float64)
    before = c.tobytes()
    h = ctypes.c_void_p()
    rc = L.kmamd_minibatch_create(ctypes.byref(h), a["metric"], a["d"], a["k"], a["device"], a["device_ptrs"], 0,
                                  None if "centroids" in over else c.ctypes.data,
                                  None if cw is None else cw.ctypes.data)
    assert rc == 1, what   # kmcudaInvalidArguments
    assert not h.value, what
    assert c.tobytes() == before


def test_create_refuses_a_null_handle_pointer():
    L = _built()
    c = numpy.zeros((_K, _D), numpy.float32)
    assert L.kmamd_minibatch_create(None, 0, _D, _K, 0, -1, 0, c.ctypes.data, None) == 1


def test_calls_on_a_null_handle_are_refused_with_outputs_untouched():
    L = _built()
    x = numpy.random.default_rng(6).standard_normal((_N, _D)).astype(numpy.float32)
    w = numpy.ones(_N, numpy.float32)
    asg = numpy.full(_N, _SENTINEL, numpy.uint32)
    cen = numpy.full((_K, _D), -7.5, numpy.float32)
    cw = numpy.full(_K, -7.5, numpy.float64)
    steps = ctypes.c_uint64(_SENTINEL)
    before = (asg.tobytes(), cen.tobytes(), cw.tobytes())
    assert L.kmamd_minibatch_step(None, _N, 0, x.ctypes.data, w.ctypes.data, asg.ctypes.data, -1) == 1
    assert L.kmamd_minibatch_fit(None, _N, 0, x.ctypes.data, w.ctypes.data, 16, 2, 0, -1) == 1
    assert L.kmamd_minibatch_read(None, cen.ctypes.data, cw.ctypes.data, ctypes.byref(steps), -1) == 1
    L.kmamd_minibatch_destroy(None)   # a no-op
    assert (asg.tobytes(), cen.tobytes(), cw.tobytes()) == before
    assert steps.value == _SENTINEL


def test_python_arguments_are_checked_before_the_device_is_touched():
    from kmcuda_amd import MiniBatchKMeans, kmeans_minibatch
    c = numpy.zeros((_K, _D), numpy.float32)
    x = numpy.zeros((_N, _D), numpy.float32)
    with pytest.raises(ValueError):
        MiniBatchKMeans(c, metric="manhattan")
    with pytest.raises(ValueError):
        MiniBatchKMeans(c[:1])
    with pytest.raises(ValueError):
        MiniBatchKMeans(numpy.zeros(8, numpy.float32))
    with pytest.raises(TypeError):
        MiniBatchKMeans(c, device="0")
    with pytest.raises(TypeError):
        MiniBatchKMeans(c.astype(numpy.float64))
    with pytest.raises(ValueError):
        MiniBatchKMeans(c, cluster_weights=numpy.array([1.0, -1.0, 0.0, 0.0]))
    with pytest.raises(ValueError):
        MiniBatchKMeans(c, cluster_weights=numpy.array([1.0, numpy.nan, 0.0, 0.0]))
    with pytest.raises(ValueError):
        MiniBatchKMeans(c, cluster_weights=numpy.zeros(3))
    with pytest.raises(TypeError):
        MiniBatchKMeans(c, cluster_weights=numpy.zeros(_K, numpy.float32))
    with pytest.raises(ValueError):
        kmeans_minibatch(x, 1, 16, 2, init=c)
    with pytest.raises(ValueError):
        kmeans_minibatch(x, _K, 0, 2, init=c)
    with pytest.raises(TypeError):
        kmeans_minibatch(x, _K, 16, 2.5, init=c)
    with pytest.raises(ValueError):
        kmeans_minibatch(x, _K, 16, 2, init="k-means++")
    with pytest.raises(ValueError):
        kmeans_minibatch(x, _K, 16, 2, init=c[:, :4])
    with pytest.raises(ValueError):
        kmeans_minibatch(x[:0], _K, 16, 2, init=c)
