"""The refusals of knn_rerank, on a machine without a device: the C ABI answers InvalidArguments with
the outputs bit for bit what they were -- any answer that came after a device call would be NoSuchDevice here -- and
the Python call raises before the library is asked for anything.  Only refused or empty calls are issued."""
import numpy
import pytest

from kmcuda_amd import knn_rerank

_Q, _N, _D, _R, _TOP = 3, 50, 8, 20, 5

# (what is wrong, the arguments that differ from a valid host call)
C_TABLE = [
    ("k = 0", dict(k=0)), ("k = 257", dict(k=257, r=300)), ("k > R", dict(k=_R + 1)),
    ("R = 0", dict(r=0)), ("R = 1025", dict(r=1025)),
    ("D = 0", dict(width=0)), ("N = 0", dict(rows=0)), ("N = 2^32 - 1", dict(rows=(1 << 32) - 1)),
    ("angular", dict(metric=1)), ("fp16", dict(fp16=1)),
    ("device = -1", dict(device=-1)), ("device_ptrs != device", dict(device_ptrs=1)),
] + [("no " + name, {name: None}) for name in ("queries", "samples", "candidates", "indices", "distances")]


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from kmcuda_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("what,over", C_TABLE, ids=[row[0] for row in C_TABLE])
def test_c_abi_refuses_with_outputs_untouched(what, over):
    floats, ints = numpy.zeros(_N * _D, numpy.float32), numpy.zeros(_Q * 1025, numpy.uint32)
    idx, dist = numpy.full((_Q, 257), 0x5A5A5A5A, numpy.uint32), numpy.full((_Q, 257), -7.5, numpy.float32)
    a = dict(rows=_N, width=_D, r=_R, k=_TOP, metric=0, fp16=0, device=0, device_ptrs=-1, queries=floats.ctypes.data,
             samples=floats.ctypes.data, candidates=ints.ctypes.data, indices=idx.ctypes.data,
             distances=dist.ctypes.data)
    a.update(over)
    before = idx.tobytes(), dist.tobytes()
    rc = _lib().kmamd_knn_rerank(_Q, a["rows"], a["width"], a["r"], a["k"], a["metric"], a["fp16"], a["device"],
                                 a["device_ptrs"], 0, a["queries"], a["samples"], a["candidates"], a["indices"],
                                 a["distances"])
    assert rc == 1, what   # kmcudaInvalidArguments
    assert (idx.tobytes(), dist.tobytes()) == before, what


def test_no_queries_is_success():
    x = numpy.zeros((_N, _D), numpy.float32)
    assert _lib().kmamd_knn_rerank(0, _N, _D, _R, _TOP, 0, 0, 0, -1, 0, None, x.ctypes.data, None, None, None) == 0
    idx, dist = knn_rerank(numpy.zeros((0, _D), numpy.float32), x, numpy.zeros((0, _R), numpy.uint32), _TOP)
    assert idx.shape == dist.shape == (0, _TOP) and idx.dtype == numpy.uint32 and dist.dtype == numpy.float32


_VALID = dict(queries=numpy.zeros((_Q, _D), numpy.float32), rows=numpy.zeros((_N, _D), numpy.float32),
              candidates=numpy.zeros((_Q, _R), numpy.uint32), k=_TOP)
PY_TABLE = [
    ("k = 0", dict(k=0), ValueError),
    ("k = 257", dict(k=257, candidates=numpy.zeros((_Q, 300), numpy.uint32)), ValueError),
    ("k > R", dict(k=_R + 1), ValueError),
    ("k = 2.0", dict(k=2.0), TypeError),
    ("R = 0", dict(candidates=numpy.zeros((_Q, 0), numpy.uint32)), ValueError),
    ("R = 1025", dict(candidates=numpy.zeros((_Q, 1025), numpy.uint32)), ValueError),
    ("candidates of another Q", dict(candidates=numpy.zeros((_Q + 1, _R), numpy.uint32)), ValueError),
    ("float candidates", dict(candidates=numpy.zeros((_Q, _R), numpy.float32)), TypeError),
    ("D = 0", dict(queries=numpy.zeros((_Q, 0), numpy.float32), rows=numpy.zeros((_N, 0), numpy.float32)), ValueError),
    ("N = 0", dict(rows=numpy.zeros((0, _D), numpy.float32)), ValueError),
    ("rows of another width", dict(rows=numpy.zeros((_N, _D + 1), numpy.float32)), ValueError),
    ("fp16", dict(rows=numpy.zeros((_N, _D), numpy.float16)), ValueError),
    ("angular", dict(metric="cos"), ValueError),
    ("device = -1", dict(device=-1), ValueError),
]


@pytest.mark.parametrize("what,over,exc", PY_TABLE, ids=[row[0] for row in PY_TABLE])
def test_python_raises_before_the_library(monkeypatch, what, over, exc):
    from kmcuda_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was asked")))
    kw = dict(_VALID, **over)
    args = [kw.pop(n) for n in ("queries", "rows", "candidates", "k")]
    with pytest.raises(exc):
        knn_rerank(*args, **kw)
