"""The common front of the three chunked row calls (kmcuda_amd/csrc/host_job.hpp: rows_call_begin): one table of bad
common arguments through kmamd_kmeans_assign, kmamd_kmeans_assign_top and kmamd_kmeans_seed_parallel.  Every row is
InvalidArguments with the outputs bit for bit what they were -- also on a machine without a device, where any answer
that came after a device call would be NoSuchDevice.  Only refused calls are issued here."""
import numpy
import pytest

_SENTINEL = 0x5A5A5A5A
_N, _K, _M = 64, 4, 2

# (what is wrong, the arguments that differ from a valid host call, fp16x2, KMCUDA_AMD_FP16_STRICT)
TABLE = [
    ("metric 2", dict(metric=2), False, None),
    ("D = 0", dict(d=0), False, None),
    ("odd D with fp16x2", dict(d=7), True, None),
    ("device = -1", dict(device=-1), False, None),
    ("device_ptrs != device", dict(device=0, device_ptrs=1), False, None),
    ("fp16x2 with KMCUDA_AMD_FP16_STRICT=1", dict(), True, "1"),
]


def _built():
    import __graft_entry__
    __graft_entry__.build()
    from kmcuda_amd import _lib
    return _lib.lib()


def _outputs(spec):
    """Named output buffers, each filled with its sentinel, and their bytes as they are before the call."""
    out = {name: numpy.full(shape, fill, dtype) for name, (shape, fill, dtype) in spec.items()}
    return out, {name: buf.tobytes() for name, buf in out.items()}


def _assign(L, a, x, c, fp16):
    out, before = _outputs(dict(asg=(_N, _SENTINEL, numpy.uint32), dist=(_N, -7.5, numpy.float32),
                                counts=(_K, _SENTINEL, numpy.uint32), sums=(_K, -7.5, numpy.float64)))
    rc = L.kmamd_kmeans_assign(a["metric"], _N, a["d"], _K, a["device"], a["device_ptrs"], int(fp16), 0,
                               x.ctypes.data, c.ctypes.data, out["asg"].ctypes.data, out["dist"].ctypes.data,
                               out["counts"].ctypes.data, out["sums"].ctypes.data)
    return rc, out, before


def _assign_top(L, a, x, c, fp16):
    out, before = _outputs(dict(top=((_N, _M), _SENTINEL, numpy.uint32), dist=((_N, _M), -7.5, numpy.float32)))
    rc = L.kmamd_kmeans_assign_top(a["metric"], _N, a["d"], _K, _M, a["device"], a["device_ptrs"], int(fp16), 0,
                                   x.ctypes.data, c.ctypes.data, out["top"].ctypes.data, out["dist"].ctypes.data)
    return rc, out, before


def _seed_parallel(L, a, x, c, fp16):
    out, before = _outputs(dict(cen=(c.shape, -7.5, c.dtype), rows=(16, _SENTINEL, numpy.uint32),
                                counts=(16, _SENTINEL, numpy.uint32), total=(1, _SENTINEL, numpy.uint32),
                                ends=(65, _SENTINEL, numpy.uint32), fell=(1, 77, numpy.int32)))
    rc = L.kmamd_kmeans_seed_parallel(a["metric"], _N, a["d"], _K, 3, 8.0, 0, a["device"], a["device_ptrs"], int(fp16),
                                      0, x.ctypes.data, out["cen"].ctypes.data, out["rows"].ctypes.data,
                                      out["counts"].ctypes.data, 16, out["total"].ctypes.data,
                                      out["ends"].ctypes.data, out["fell"].ctypes.data)
    return rc, out, before


@pytest.mark.parametrize("call", [_assign, _assign_top, _seed_parallel], ids=["assign", "assign_top", "seed_parallel"])
@pytest.mark.parametrize("what,over,fp16,strict", TABLE, ids=[row[0] for row in TABLE])
def test_refused_before_any_device_call_with_outputs_untouched(monkeypatch, call, what, over, fp16, strict):
    L = _built()
    if strict is None:
        monkeypatch.delenv("KMCUDA_AMD_FP16_STRICT", raising=False)
    else:
        monkeypatch.setenv("KMCUDA_AMD_FP16_STRICT", strict)
    # the buffers are as wide as a valid call's (8 features, or the 7 of the odd row), whatever D the call is told
    width = over.get("d") or 8
    x = numpy.random.default_rng(5).standard_normal((_N, width)).astype(numpy.float16 if fp16 else numpy.float32)
    c = x[:_K].copy()
    a = dict(metric=0, d=width, device=0, device_ptrs=-1)
    a.update(over)
    rc, out, before = call(L, a, x, c, fp16)
    assert rc == 1, what   # kmcudaInvalidArguments
    for name, buf in out.items():
        assert buf.tobytes() == before[name], (what, name)

