"""kmeans_predict_top (kmcuda_amd/predict.py, C ABI kmamd_kmeans_assign_top / kmamd_assign_top_stats): the surface and
every refusal that is decided before a device is touched."""
import ctypes
import fnmatch
import os
import re
import subprocess

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kmamd_kmeans_assign_top", "kmamd_assign_top_stats")
_SENTINEL = 0x5A5A5A5A


def _built():
    import __graft_entry__
    __graft_entry__.build()
    from kmcuda_amd import _lib
    return _lib


def test_importable_declared_and_listed():
    import kmcuda_amd
    from kmcuda_amd import _lib
    from kmcuda_amd.predict import kmeans_predict_top
    assert kmcuda_amd.kmeans_predict_top is kmeans_predict_top
    with open(os.path.join(ROOT, "include", "kmcuda_amd.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    with open(os.path.join(ROOT, "kmcuda_amd", "csrc", "exports.map")) as f:
        patterns = re.findall(r"^\s*([\w*]+);", f.read().split("local:")[0], flags=re.M)
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns)


def test_library_exports_the_symbols_with_argtypes():
    _l = _built()
    L = _l.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _l.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert set(NAMES) <= exported
    fn = L.kmamd_kmeans_assign_top
    assert fn.restype is _l.i32 and len(fn.argtypes) == 13
    assert fn.argtypes[2] is ctypes.c_uint16 and fn.argtypes[4] is _l.u32 and fn.argtypes[5] is _l.i32
    assert L.kmamd_assign_top_stats.restype is _l.i32 and len(L.kmamd_assign_top_stats.argtypes) == 2


def test_stats_before_any_call_and_null_pointers():
    L = _built().lib()
    a, b = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.kmamd_assign_top_stats(ctypes.byref(a), ctypes.byref(b)) == 0
    assert a.value <= b.value or b.value == 0
    assert L.kmamd_assign_top_stats(None, None) == 0


@pytest.fixture
def no_device(monkeypatch):
    """Fails the test if the library is loaded at all: validation must come first."""
    from kmcuda_amd import _lib

    def boom():
        raise AssertionError("the device library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", boom)


def _xc(n=64, d=8, k=4, dtype=numpy.float32):
    rng = numpy.random.default_rng(5)
    x = rng.standard_normal((n, d)).astype(dtype)
    return x, x[:k].copy()


@pytest.mark.parametrize("m", [0, -1, 5, 65])
def test_m_out_of_range(no_device, m):
    from kmcuda_amd import kmeans_predict_top
    x, c = _xc()
    with pytest.raises(ValueError):
        kmeans_predict_top(x, c, m)


def test_m_above_64_with_many_centroids(no_device):
    from kmcuda_amd import kmeans_predict_top
    x, c = _xc(n=100, k=100)
    with pytest.raises(ValueError):
        kmeans_predict_top(x, c, 65)


@pytest.mark.parametrize("m", [2.0, "2", None, True])
def test_m_must_be_an_integer(no_device, m):
    from kmcuda_amd import kmeans_predict_top
    x, c = _xc()
    with pytest.raises(TypeError):
        kmeans_predict_top(x, c, m)


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.int32])
def test_wrong_dtype(no_device, dtype):
    from kmcuda_amd import kmeans_predict_top
    x, c = _xc()
    with pytest.raises(TypeError):
        kmeans_predict_top(x.astype(dtype), c, 2)
    with pytest.raises(TypeError):
        kmeans_predict_top(x, c.astype(dtype), 2)


def test_centroids_dtype_must_match(no_device):
    from kmcuda_amd import kmeans_predict_top
    x, c = _xc()
    with pytest.raises(TypeError):
        kmeans_predict_top(x, c.astype(numpy.float16), 2)
    with pytest.raises(TypeError):
        kmeans_predict_top(x.astype(numpy.float16), c, 2)


def test_shapes(no_device):
    from kmcuda_amd import kmeans_predict_top
    x, c = _xc()
    for bad_x, bad_c in ((x[0], c), (x, c[0]), (x[:, :, None], c), (x, c[:, :7]), (x[:, :6], c), (x, c[:1]),
                         (x, c[:0])):
        with pytest.raises(ValueError):
            kmeans_predict_top(bad_x, bad_c, 1)


def test_host_torch_tensor_is_neither_kind(no_device):
    torch = pytest.importorskip("torch")
    from kmcuda_amd import kmeans_predict_top
    x, c = _xc()
    with pytest.raises(ValueError):
        kmeans_predict_top(torch.from_numpy(x), c, 2)


def test_odd_features_with_float16(no_device):
    from kmcuda_amd import kmeans_predict_top
    x, c = _xc(d=7, dtype=numpy.float16)
    with pytest.raises(ValueError):
        kmeans_predict_top(x, c, 2)


def test_strict_half2_refused_from_python(no_device, monkeypatch):
    from kmcuda_amd import kmeans_predict_top
    x, c = _xc(dtype=numpy.float16)
    monkeypatch.setenv("KMCUDA_AMD_FP16_STRICT", "1")
    with pytest.raises(ValueError):
        kmeans_predict_top(x, c, 2)


def test_metric_and_device(no_device):
    from kmcuda_amd import kmeans_predict_top
    x, c = _xc()
    with pytest.raises(ValueError):
        kmeans_predict_top(x, c, 2, metric="manhattan")
    with pytest.raises(TypeError):
        kmeans_predict_top(x, c, 2, metric=3)
    with pytest.raises(ValueError):
        kmeans_predict_top(x, c, 2, device=-1)
    with pytest.raises(TypeError):
        kmeans_predict_top(x, c, 2, device="0")


def _raw_call(L, x, c, fp16, m=2, **over):
    n, d = x.shape
    k = c.shape[0]
    top = numpy.full((n, 64), _SENTINEL, numpy.uint32)
    dist = numpy.full((n, 64), numpy.float32(-7.5), numpy.float32)
    a = dict(metric=0, n=n, d=d, k=k, m=m, device=0, device_ptrs=-1, samples=x.ctypes.data, centroids=c.ctypes.data,
             top=top.ctypes.data)
    a.update(over)
    rc = L.kmamd_kmeans_assign_top(a["metric"], a["n"], a["d"], a["k"], a["m"], a["device"], a["device_ptrs"],
                                   int(fp16), 0, a["samples"], a["centroids"], a["top"], dist.ctypes.data)
    untouched = (top == _SENTINEL).all() and (dist == numpy.float32(-7.5)).all()
    return rc, untouched


@pytest.mark.parametrize("over", [dict(m=0), dict(m=5), dict(m=65), dict(metric=2), dict(d=0), dict(k=1), dict(k=0),
                                  dict(samples=None), dict(centroids=None), dict(top=None), dict(device=-1),
                                  dict(device=0, device_ptrs=1)])
def test_c_call_refuses_with_outputs_untouched(over):
    L = _built().lib()
    x, c = _xc()
    rc, untouched = _raw_call(L, x, c, False, **over)
    assert rc == 1 and untouched


def test_c_call_refuses_m_above_64_with_many_centroids():
    L = _built().lib()
    x, c = _xc(n=100, k=100)
    rc, untouched = _raw_call(L, x, c, False, m=65)
    assert rc == 1 and untouched
    rc, _ = _raw_call(L, x, c, False, m=64, device=1 << 20)   # in range: past the checks, to "no such device"
    assert rc == 2


def test_c_call_refuses_odd_half_features():
    L = _built().lib()
    x, c = _xc(d=7, dtype=numpy.float16)
    rc, untouched = _raw_call(L, x, c, True)
    assert rc == 1 and untouched


def test_c_call_refuses_strict_half2_with_outputs_untouched(monkeypatch):
    L = _built().lib()
    x, c = _xc(dtype=numpy.float16)
    monkeypatch.setenv("KMCUDA_AMD_FP16_STRICT", "1")
    rc, untouched = _raw_call(L, x, c, True)
    assert rc == 1 and untouched
    # the switch concerns half rows only: fp32 rows get past the check (to the device, or to "no such device")
    x32, c32 = _xc()
    rc, _ = _raw_call(L, x32, c32, False, device=1 << 20)
    assert rc == 2
