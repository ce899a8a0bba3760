"""The refusals of the precomputed-term IVF-PQ search on a machine without a device: the Python calls
raise before the library is asked for anything, the C ABI answers InvalidArguments with the outputs untouched."""
import numpy
import pytest

from kmcuda_amd import ivfpq_search, ivfpq_terms
from test_ivfpq_cpu import _DSUB, _K, _KSUB, _L, _M, _NPROBE, _Q, _TOP, _VALID, _lib

torch = pytest.importorskip("torch")
_TERMS = numpy.zeros((_K, _M, _KSUB), numpy.float32)

SEARCH_TABLE = [
    ("K + 1 clusters", dict(terms=numpy.zeros((_K + 1, _M, _KSUB), numpy.float32)), ValueError),
    ("256 columns", dict(terms=numpy.zeros((_K, _M, 256), numpy.float32)), ValueError),
    ("flat", dict(terms=_TERMS.reshape(-1)), ValueError),
    ("float64", dict(terms=_TERMS.astype(numpy.float64)), TypeError),
    ("a tensor beside arrays", dict(terms=torch.from_numpy(_TERMS)), (ValueError, TypeError)),
    ("angular", dict(terms=_TERMS, metric="cos"), ValueError),
]
TERMS_TABLE = [
    ("codebooks of another width", dict(codebooks=numpy.zeros((_M, _KSUB, _DSUB - 1), numpy.float32)), ValueError),
    ("ksub = 257", dict(codebooks=numpy.zeros((_M, 257, _DSUB), numpy.float32)), ValueError),
    ("no cluster", dict(centroids=numpy.zeros((0, _M * _DSUB), numpy.float32)), ValueError),
    ("float64", dict(centroids=numpy.zeros((_K, _M * _DSUB), numpy.float64)), TypeError),
    ("a tensor beside an array", dict(codebooks=torch.zeros((_M, _KSUB, _DSUB))), (ValueError, TypeError)),
    ("angular", dict(metric="cos"), ValueError),
]


@pytest.fixture
def no_library(monkeypatch):
    from kmcuda_amd import _lib as loader
    monkeypatch.setattr(loader, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was asked")))


@pytest.mark.parametrize("what,over,exc", SEARCH_TABLE, ids=[row[0] for row in SEARCH_TABLE])
def test_search_raises_before_the_library(no_library, what, over, exc):
    kw = dict(_VALID)
    kw.update(over)
    args = [kw.pop(n) for n in ("queries", "centroids", "codebooks", "codes", "ids", "offsets", "probes", "k")]
    with pytest.raises(exc):
        ivfpq_search(*args, **kw)


@pytest.mark.parametrize("what,over,exc", TERMS_TABLE, ids=[row[0] for row in TERMS_TABLE])
def test_terms_raises_before_the_library(no_library, what, over, exc):
    kw = dict(centroids=_VALID["centroids"], codebooks=_VALID["codebooks"])
    kw.update(over)
    with pytest.raises(exc):
        ivfpq_terms(kw.pop("centroids"), kw.pop("codebooks"), **kw)


def test_c_abi_refuses_with_outputs_untouched():
    L, floats, ints = _lib(), numpy.zeros(_K * _M * _DSUB * _KSUB, numpy.float32), numpy.zeros(1000, numpy.uint32)
    idx, dist = numpy.full((_Q, _TOP), 0x5A5A5A5A, numpy.uint32), numpy.full((_Q, _TOP), -7.5, numpy.float32)
    f, i = floats.ctypes.data, ints.ctypes.data
    for terms, metric in ((None, 0), (f, 1)):
        assert L.kmamd_ivfpq_search_precomputed(_Q, _L, _M * _DSUB, _K, _M, _DSUB, _KSUB, _TOP, _NPROBE, metric, 0, 0,
                                                -1, 0, f, f, f, i, i, i, i, terms, idx.ctypes.data,
                                                dist.ctypes.data) == 1
    assert (idx == 0x5A5A5A5A).all() and (dist == -7.5).all()
    out = numpy.full(_K * _M * _KSUB, -7.5, numpy.float32)
    for clusters, width, m, ksub, device, ptrs, cen in [(0, 32, _M, _KSUB, 0, -1, f), (_K, 33, _M, _KSUB, 0, -1, f),
                                                        (_K, 0, 0, _KSUB, 0, -1, f), (_K, 32, _M, 257, 0, -1, f),
                                                        (_K, 32, _M, _KSUB, -1, -1, f), (_K, 32, _M, _KSUB, 0, 1, f),
                                                        (_K, 32, _M, _KSUB, 0, -1, None)]:
        assert L.kmamd_ivfpq_terms(clusters, width, m, _DSUB, ksub, device, ptrs, 0, cen, f, out.ctypes.data) == 1
    assert (out == -7.5).all()
