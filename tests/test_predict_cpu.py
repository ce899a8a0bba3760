"""kmeans_predict (kmcuda_amd/predict.py, C ABI kmamd_kmeans_assign): the surface and every refusal that is decided
before a device is touched."""
import ctypes
import os
import re
import subprocess

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "kmamd_kmeans_assign"
_SENTINEL = 0x5A5A5A5A


def _built():
    import __graft_entry__
    __graft_entry__.build()
    from kmcuda_amd import _lib
    return _lib


def test_importable_declared_and_listed():
    import kmcuda_amd
    from kmcuda_amd import kmeans_predict, _lib  # noqa: F401
    assert callable(kmcuda_amd.kmeans_predict)
    assert NAME in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "kmcuda_amd.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, header)
    with open(os.path.join(ROOT, "kmcuda_amd", "csrc", "exports.map")) as f:
        patterns = re.findall(r"^\s*([\w*]+);", f.read().split("local:")[0], flags=re.M)
    import fnmatch
    assert any(fnmatch.fnmatchcase(NAME, p) for p in patterns)


def test_library_exports_the_symbol_with_argtypes():
    _l = _built()
    L = _l.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _l.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert NAME in exported
    fn = getattr(L, NAME)
    assert fn.restype is _l.i32 and len(fn.argtypes) == 14
    assert fn.argtypes[2] is ctypes.c_uint16 and fn.argtypes[5] is _l.i32


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


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.int32])
def test_wrong_dtype(no_device, dtype):
    from kmcuda_amd import kmeans_predict
    x, c = _xc()
    with pytest.raises(TypeError):
        kmeans_predict(x.astype(dtype), c)
    with pytest.raises(TypeError):
        kmeans_predict(x, c.astype(dtype))


def test_centroids_dtype_must_match(no_device):
    from kmcuda_amd import kmeans_predict
    x, c = _xc()
    with pytest.raises(TypeError):
        kmeans_predict(x, c.astype(numpy.float16))
    with pytest.raises(TypeError):
        kmeans_predict(x.astype(numpy.float16), c)


def test_not_two_dimensional(no_device):
    from kmcuda_amd import kmeans_predict
    x, c = _xc()
    with pytest.raises(ValueError):
        kmeans_predict(x[0], c)
    with pytest.raises(ValueError):
        kmeans_predict(x, c[0])
    with pytest.raises(ValueError):
        kmeans_predict(x[:, :, None], c)
    with pytest.raises(ValueError):
        kmeans_predict(x, c[:, :, None])


def test_feature_mismatch(no_device):
    from kmcuda_amd import kmeans_predict
    x, c = _xc()
    with pytest.raises(ValueError):
        kmeans_predict(x, c[:, :7])
    with pytest.raises(ValueError):
        kmeans_predict(x[:, :6], c)


def test_mixed_numpy_and_torch(no_device):
    torch = pytest.importorskip("torch")
    from kmcuda_amd import kmeans_predict
    x, c = _xc()

    class FakeDeviceTensor:
        """What _rows sees of a device tensor, without a device."""
        __module__ = "torch"
        dtype = torch.float32
        is_cuda = True
        shape = (4, 8)

        class device:
            index = 0

        def dim(self):
            return 2

        def contiguous(self):
            return self
    FakeDeviceTensor.__module__ = "torch"
    with pytest.raises(TypeError):
        kmeans_predict(x, FakeDeviceTensor())
    with pytest.raises(TypeError):
        kmeans_predict(FakeDeviceTensor(), c)
    with pytest.raises(ValueError):   # a host tensor is neither kind
        kmeans_predict(torch.from_numpy(x), c)


def test_odd_features_with_float16(no_device):
    from kmcuda_amd import kmeans_predict
    x, c = _xc(d=7, dtype=numpy.float16)
    with pytest.raises(ValueError):
        kmeans_predict(x, c)


def test_one_centroid(no_device):
    from kmcuda_amd import kmeans_predict
    x, c = _xc()
    with pytest.raises(ValueError):
        kmeans_predict(x, c[:1])
    with pytest.raises(ValueError):
        kmeans_predict(x, c[:0])


def test_metric_and_device(no_device):
    from kmcuda_amd import kmeans_predict
    x, c = _xc()
    with pytest.raises(ValueError):
        kmeans_predict(x, c, metric="manhattan")
    with pytest.raises(TypeError):
        kmeans_predict(x, c, metric=3)
    with pytest.raises(ValueError):
        kmeans_predict(x, c, device=-1)
    with pytest.raises(TypeError):
        kmeans_predict(x, c, device="0")


def _raw_call(L, x, c, fp16, **over):
    n, d = x.shape
    k = c.shape[0]
    asg = numpy.full(n, _SENTINEL, numpy.uint32)
    dist = numpy.full(n, numpy.float32(-7.5), numpy.float32)
    counts = numpy.full(k, _SENTINEL, numpy.uint32)
    sums = numpy.full(k, -7.5, numpy.float64)
    a = dict(metric=0, n=n, d=d, k=k, device=0, device_ptrs=-1, samples=x.ctypes.data, centroids=c.ctypes.data,
             assignments=asg.ctypes.data)
    a.update(over)
    rc = L.kmamd_kmeans_assign(a["metric"], a["n"], a["d"], a["k"], a["device"], a["device_ptrs"], int(fp16), 0,
                               a["samples"], a["centroids"], a["assignments"], dist.ctypes.data, counts.ctypes.data,
                               sums.ctypes.data)
    untouched = ((asg == _SENTINEL).all() and (dist == numpy.float32(-7.5)).all() and (counts == _SENTINEL).all()
                 and (sums == -7.5).all())
    return rc, untouched


def test_c_call_refuses_strict_half2_with_outputs_untouched(monkeypatch):
    """KMCUDA_AMD_FP16_STRICT=1 with fp16x2 rows: InvalidArguments before any device work (this machine may have no
    device at all: any later answer would be NoSuchDevice)."""
    L = _built().lib()
    x, c = _xc(dtype=numpy.float16)
    monkeypatch.setenv("KMCUDA_AMD_FP16_STRICT", "1")
    rc, untouched = _raw_call(L, x, c, True)
    assert rc == 1 and untouched
    # the switch concerns half rows only: fp32 rows get past the check (to the device, or to "no such device")
    x32, c32 = _xc()
    rc, _ = _raw_call(L, x32, c32, False, device=1 << 20)
    assert rc == 2


@pytest.mark.parametrize("over", [dict(metric=2), dict(d=0), dict(k=1), dict(k=0), dict(samples=None),
                                  dict(centroids=None), dict(assignments=None), dict(device=-1),
                                  dict(device=0, device_ptrs=1)])
def test_c_call_refuses_bad_sizes_and_null_pointers(over):
    L = _built().lib()
    x, c = _xc()
    rc, untouched = _raw_call(L, x, c, False, **over)
    assert rc == 1 and untouched


def test_c_call_refuses_odd_half_features():
    L = _built().lib()
    x, c = _xc(d=7, dtype=numpy.float16)
    rc, untouched = _raw_call(L, x, c, True)
    assert rc == 1 and untouched
