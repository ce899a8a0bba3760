"""The refusals of the batched K-means calls, on a machine without a device: the C ABI answers
InvalidArguments with the outputs bit for bit what they were -- any answer that came after a device call would be
NoSuchDevice here -- and the Python calls raise before the library is asked for anything.  Only refused calls are
issued."""
import numpy
import pytest

_SENTINEL = 0x5A5A5A5A
_B, _N, _D, _K = 2, 64, 8, 4

# (what is wrong, the arguments that differ from a valid host call)
C_TABLE = [
    ("no problems", dict(b=0)),
    ("layout 2", dict(layout=2)),
    ("angular", dict(metric=1)),
    ("fp16", dict(fp16=1)),
    ("D = 0", dict(d=0)),
    ("D = 65", dict(d=65)),
    ("k = 0", dict(k=0)),
    ("panel beyond the LDS bound", dict(k=2049)),
    ("device = -1", dict(device=-1)),
    ("device_ptrs != device", dict(device_ptrs=1)),
]
FIT_TABLE = C_TABLE + [("k > N", dict(k=_N + 1)), ("sample weights", dict(weights=True)), ("max_iter = 0", dict(it=0)),
                       ("tolerance > 1", dict(tol=1.5)), ("init 2", dict(init=2))]


def _built():
    import __graft_entry__
    __graft_entry__.build()
    from kmcuda_amd import _lib
    return _lib.lib()


def _args(over):
    a = dict(b=_B, n=_N, d=_D, k=_K, layout=0, metric=0, fp16=0, device=0, device_ptrs=-1, weights=False, it=5,
             tol=0.0, init=0)
    a.update(over)
    return a


@pytest.mark.parametrize("what,over", C_TABLE + [("uint8 codes with k = 257", dict(k=257, u8=1))],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_assign_batched_refused_with_outputs_untouched(what, over):
    L, a = _built(), _args(over)
    x, c = numpy.zeros((_B, _N, 65), numpy.float32), numpy.zeros((_B, 4096, 65), numpy.float32)
    asg, dist = numpy.full((_B, _N), _SENTINEL, numpy.uint32), numpy.full((_B, _N), -7.5, numpy.float32)
    before = asg.tobytes(), dist.tobytes()
    rc = L.kmamd_kmeans_assign_batched(a["b"], a["n"], a["d"], a["k"], a["layout"], a["metric"], a["fp16"],
                                       a["device"], a["device_ptrs"], 0, a.get("u8", 0), x.ctypes.data, c.ctypes.data,
                                       asg.ctypes.data, dist.ctypes.data)
    assert rc == 1, what   # kmcudaInvalidArguments
    assert (asg.tobytes(), dist.tobytes()) == before, what


@pytest.mark.parametrize("what,over", FIT_TABLE, ids=[row[0] for row in FIT_TABLE])
def test_kmeans_batched_refused_with_outputs_untouched(what, over):
    L, a = _built(), _args(over)
    x, w = numpy.zeros((_B, _N, 65), numpy.float32), numpy.ones((_B, _N), numpy.float32)
    cen = numpy.full((_B, 4096, 65), -7.5, numpy.float32)
    asg, its = numpy.full((_B, _N), _SENTINEL, numpy.uint32), numpy.full(_B, _SENTINEL, numpy.uint32)
    before = cen.tobytes(), asg.tobytes(), its.tobytes()
    rc = L.kmamd_kmeans_batched(a["b"], a["n"], a["d"], a["k"], a["layout"], a["metric"], a["fp16"], a["init"],
                                a["tol"], a["it"], 0, a["device"], a["device_ptrs"], 0, x.ctypes.data,
                                w.ctypes.data if a["weights"] else None, cen.ctypes.data, asg.ctypes.data,
                                its.ctypes.data)
    assert rc == 1, what
    assert (cen.tobytes(), asg.tobytes(), its.tobytes()) == before, what


def test_max_clusters_is_the_panel_bound():
    from kmcuda_amd import batched
    L = _built()
    for d in range(0, 70):
        assert batched.max_clusters(d) == L.kmamd_batched_max_clusters(d)
    assert [batched.max_clusters(d) for d in (1, 4, 5, 8, 16, 17, 32, 64, 65)] == [4096, 4096, 2048, 2048, 1024, 512,
                                                                                   512, 256, 0]


_X = numpy.zeros((_B, _N, _D), numpy.float32)
_C = numpy.zeros((_B, _K, _D), numpy.float32)
PY_TABLE = [
    ("wrong rank", dict(samples=_X[0]), ValueError),
    ("columns without problems", dict(samples=_X[0], layout="columns"), ValueError),
    ("D > 64", dict(samples=numpy.zeros((_B, _N, 65), numpy.float32)), ValueError),
    ("k > N", dict(k=_N + 1), ValueError),
    ("panel beyond the LDS bound", dict(samples=numpy.zeros((1, 4096, _D), numpy.float32), k=2049), ValueError),
    ("fp16", dict(samples=_X.astype(numpy.float16)), ValueError),
    ("float64", dict(samples=_X.astype(numpy.float64)), TypeError),
    ("angular", dict(metric="cos"), ValueError),
    ("sample weights", dict(sample_weight=numpy.ones((_B, _N), numpy.float32)), ValueError),
    ("unknown layout", dict(layout="rows"), ValueError),
    ("unknown init", dict(init="k-means++"), ValueError),
    ("init of another shape", dict(init=_C[:, :3]), ValueError),
]


@pytest.mark.parametrize("what,over,exc", PY_TABLE, ids=[row[0] for row in PY_TABLE])
def test_python_calls_raise_before_the_library(monkeypatch, what, over, exc):
    from kmcuda_amd import _lib, batched

    def no_library():
        raise AssertionError("the library was asked")
    monkeypatch.setattr(_lib, "lib", no_library)
    kw = dict(samples=_X, k=_K, init="random")
    kw.update(over)
    with pytest.raises(exc):
        batched.kmeans_batched(kw.pop("samples"), kw.pop("k"), **kw)
    if "init" in over or what == "k > N":
        return
    kw = dict(samples=_X, centroids=_C if over.get("k", _K) == _K else numpy.zeros((1, over["k"], _D), numpy.float32))
    kw.update({key: v for key, v in over.items() if key != "k"})
    with pytest.raises(exc):
        batched.kmeans_predict_batched(kw.pop("samples"), kw.pop("centroids"), **kw)
