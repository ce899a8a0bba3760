"""CPU checks of the sample-weight boundary (kmamd_kmeans_weighted, kmamd_set_weights, the `sample_weight` keyword):
what is exported, and every refusal that is decided before a device is touched."""
import ctypes
import os
import re
import subprocess

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SENTINEL = 0x5A5A5A5A


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from kmcuda_amd import _lib
    return _lib


def test_the_two_new_symbols_and_nothing_else():
    """nm -D: kmamd_kmeans_weighted and kmamd_set_weights are exported, declared in kmcuda_amd.h and listed with their
    argument types in _lib.EXPORTS; nothing leaves the library that the two headers do not declare."""
    _l = _lib()
    L = _l.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _l.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert {"kmamd_kmeans_weighted", "kmamd_set_weights"} <= exported
    declared = set()
    for header in ("kmcuda.h", "kmcuda_amd.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        declared |= {m.group(1) for m in re.finditer(r"\b(kmeans_cuda|knn_cuda|kmamd_\w+)\s*\(", text)}
    assert exported == declared | {"PyInit_libKMCUDA"}
    assert {"kmamd_kmeans_weighted", "kmamd_set_weights"} <= set(_l.EXPORTS)
    assert len(L.kmamd_kmeans_weighted.argtypes) == len(L.kmeans_cuda.argtypes) + 1
    assert len(L.kmamd_set_weights.argtypes) == 2
    # kmcuda.h is the reference's header: it does not know the call
    assert "weight" not in open(os.path.join(ROOT, "include", "kmcuda.h")).read().lower()


@pytest.mark.parametrize("module", ["kmcuda_amd", "libKMCUDA"])
def test_python_refuses_malformed_weights_without_gpu(module):
    """Wrong length, wrong dtype, wrong dimension: ValueError from the mirror module and from the native one, before
    any device is looked for."""
    _lib()
    mod = __import__(module)
    x = numpy.random.RandomState(0).rand(100, 4).astype(numpy.float32)
    good = numpy.ones(100, numpy.float32)
    for bad in (good[:99], numpy.ones(101, numpy.float32),          # length
                good.astype(numpy.float64), good.astype(numpy.int32),   # dtype
                numpy.ones((100, 1), numpy.float32), numpy.float32(1.0).reshape(())):   # dimension
        with pytest.raises(ValueError, match="sample_weight"):
            mod.kmeans_cuda(x, 5, sample_weight=bad)
    with pytest.raises(ValueError, match="sample_weight"):
        mod.kmeans_cuda(x, 5, sample_weight=[1.0] * 100)            # not an array
    # device-pointer mode: a raw pointer, by the convention of the other buffers
    with pytest.raises(ValueError, match="sample_weight"):
        mod.kmeans_cuda((0x1000, 0, (100, 4)), 5, sample_weight=good)
    with pytest.raises(ValueError, match="sample_weight"):
        mod.kmeans_cuda((0x1000, 0, (100, 4)), 5, sample_weight=0)


def _weighted_call(L, init=0, fp16x2=0, weights=None, init_params=None):
    n, d, k = 100, 4, 10
    x = numpy.random.RandomState(1).rand(n, d * (2 if fp16x2 else 1)).astype(numpy.float16 if fp16x2 else numpy.float32)
    cen = numpy.full((k, x.shape[1]), 7, x.dtype)
    asg = numpy.full(n, _SENTINEL, numpy.uint32)
    avg = ctypes.c_float(-3.0)
    w = numpy.ones(n, numpy.float32) if weights is None else weights
    rc = L.kmamd_kmeans_weighted(init, init_params, 0.01, 0.0, 0, n, d, k, 3, 0, -1, fp16x2, 0, x.ctypes.data,
                                 cen.ctypes.data, asg.ctypes.data, ctypes.cast(ctypes.byref(avg), ctypes.c_void_p),
                                 w.ctypes.data)
    untouched = (cen == 7).all() and (asg == _SENTINEL).all() and avg.value == -3.0
    return rc, untouched


def test_c_abi_refuses_reference_arithmetic_modes_with_weights_without_gpu(monkeypatch):
    """afkmc2, KMCUDA_AMD_EXACT_UPDATE=1 and KMCUDA_AMD_FP16_STRICT=1 (fp16x2 rows) restate the reference's own
    arithmetic: with weights they are InvalidArguments before any device is touched, outputs untouched."""
    L = _lib().lib()
    m = ctypes.c_uint32(0)
    assert _weighted_call(L, init=2, init_params=ctypes.byref(m)) == (1, True)     # kmcudaInitMethodAFKMC2
    monkeypatch.setenv("KMCUDA_AMD_EXACT_UPDATE", "1")
    assert _weighted_call(L) == (1, True)
    monkeypatch.delenv("KMCUDA_AMD_EXACT_UPDATE")
    monkeypatch.setenv("KMCUDA_AMD_FP16_STRICT", "1")
    assert _weighted_call(L, fp16x2=1) == (1, True)
    # the reference's argument checks come first and are unchanged (kmcuda.cc:19-61)
    monkeypatch.delenv("KMCUDA_AMD_FP16_STRICT")
    x = numpy.zeros((100, 4), numpy.float32)
    cen = numpy.zeros((10, 4), numpy.float32)
    asg = numpy.zeros(100, numpy.uint32)
    w = numpy.ones(100, numpy.float32)
    for K, D, N in ((1, 4, 100), (10, 0, 100), (10, 4, 5)):
        assert L.kmamd_kmeans_weighted(0, None, 0.01, 0.1, 0, N, D, K, 3, 0, -1, 0, 0, x.ctypes.data, cen.ctypes.data,
                                       asg.ctypes.data, None, w.ctypes.data) == 1


def test_exactly_summable_inputs_sum_the_same_in_every_order():
    """The premise of tests/test_gpu_weighted_update.py, kept checked without a GPU: rows m / 1024 and weights j 2^e
    (tests/_weighted_inputs.py) at the largest row count the GPU tests may use.  The per-cluster float64 sums of w * x
    and of w, added one row after the other in three random orders, are identical bit for bit, and on a small cluster
    they equal the rational sum (fractions.Fraction: no rounding anywhere)."""
    from fractions import Fraction
    from _weighted_inputs import MAX_ROWS, cluster_sums, exact_rows, exact_weights, index_weights
    rs = numpy.random.RandomState(3)
    n, d, k = MAX_ROWS, 5, 7
    x = exact_rows(rs, n, d)
    assert x.dtype == numpy.float32 and x.min() >= 0 and x.max() < 1 and (x * 1024 == numpy.round(x * 1024)).all()
    labels = rs.randint(0, k - 1, n).astype(numpy.int32)
    labels[rs.choice(n, 300, replace=False)] = k - 1          # the small cluster
    labels[rs.choice(n, 50, replace=False)] = -1              # rows of no cluster
    small = numpy.nonzero(labels == k - 1)[0]
    assert 200 < len(small) <= 300
    for w in (exact_weights(rs, n), index_weights(n)):
        assert w.dtype == numpy.float32 and w.min() >= 2.0 ** -6 and w.max() <= 15 * 2.0 ** 6
        assert (w * 64 == numpy.round(w * 64)).all()          # multiples of 2^-6 ...
        p = w.astype(numpy.float64)[:, None] * x.astype(numpy.float64) * 65536
        assert (p == numpy.round(p)).all() and p.max() < 2.0 ** 26   # ... products multiples of 2^-16 below 2^10
        sums = [cluster_sums(x, w, labels, k, order=rs.permutation(n)) for _ in range(3)]
        for sx, sw in sums[1:]:
            assert sx.tobytes() == sums[0][0].tobytes() and sw.tobytes() == sums[0][1].tobytes()
        assert sums[0][0].max() < 2.0 ** 26 and sums[0][1].max() < 2.0 ** 26
        fw = sum(Fraction(float(w[i])) for i in small)
        assert Fraction(float(sums[0][1][k - 1])) == fw
        for f in range(d):
            fx = sum(Fraction(float(w[i])) * Fraction(float(x[i, f])) for i in small)
            assert Fraction(float(sums[0][0][k - 1, f])) == fx
        # the pairwise order of numpy.sum (what the GPU tests' reference uses) gives the same bits again
        rows = numpy.nonzero(labels == 2)[0]
        assert ((w[rows].astype(numpy.float64)[:, None] * x[rows].astype(numpy.float64)).sum(0).tobytes()
                == sums[0][0][2].tobytes())
