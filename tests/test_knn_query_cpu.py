"""k-NN of new rows (kmcuda_amd.KnnIndex / knn_query, C ABI kmamd_knn_index_*): the surface and its argument checks,
which all run before any device is touched."""
import os

import numpy
import pytest


def _corpus(n=64, d=8, k=4, dtype=numpy.float32):
    rng = numpy.random.default_rng(3)
    x = rng.standard_normal((n, d)).astype(dtype)
    c = x[:k].copy()
    a = (numpy.arange(n) % k).astype(numpy.uint32)
    return x, c, a


def test_importable_and_exported():
    import kmcuda_amd
    from kmcuda_amd import KnnIndex, knn_query  # noqa: F401
    from kmcuda_amd import _lib
    assert callable(kmcuda_amd.knn_query) and isinstance(kmcuda_amd.KnnIndex, type)
    for name in ("kmamd_knn_index_create", "kmamd_knn_index_query", "kmamd_knn_index_destroy"):
        assert name in _lib.EXPORTS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "kmcuda_amd.h")) as f:
        header = f.read()
    for name in ("kmamd_knn_index_create(", "kmamd_knn_index_query(", "kmamd_knn_index_destroy("):
        assert name in header


def test_library_symbols():
    from kmcuda_amd import _lib
    try:
        L = _lib.lib()
    except ImportError:
        pytest.skip("the HIP library has not been built")
    for name in ("kmamd_knn_index_create", "kmamd_knn_index_query", "kmamd_knn_index_destroy"):
        assert getattr(L, name) is not None


@pytest.fixture
def no_device(monkeypatch):
    """Fails the test if the library is loaded at all: validation must come first."""
    from kmcuda_amd import _lib

    def boom():
        raise AssertionError("the device library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", boom)


@pytest.mark.parametrize("k", [0, -1, 65, 70000])
def test_k_range(no_device, k):
    from kmcuda_amd import knn_query
    x, c, a = _corpus()
    with pytest.raises(ValueError):
        knn_query(k, x, c, a, x[:3])


def test_k_type(no_device):
    from kmcuda_amd import knn_query
    x, c, a = _corpus()
    with pytest.raises(TypeError):
        knn_query(2.5, x, c, a, x[:3])


def test_feature_mismatch(no_device):
    from kmcuda_amd import knn_query
    x, c, a = _corpus()
    with pytest.raises(ValueError):
        knn_query(3, x, c, a, numpy.zeros((5, 7), numpy.float32))
    with pytest.raises(ValueError):
        knn_query(3, x, c[:, :7], a, x[:3])


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.int32])
def test_wrong_query_dtype(no_device, dtype):
    from kmcuda_amd import knn_query
    x, c, a = _corpus()
    with pytest.raises(TypeError):
        knn_query(3, x, c, a, x[:3].astype(dtype))


def test_query_dtype_must_match_corpus(no_device):
    from kmcuda_amd import knn_query
    x, c, a = _corpus()
    with pytest.raises(TypeError):
        knn_query(3, x, c, a, x[:3].astype(numpy.float16))
    xh, ch, ah = _corpus(dtype=numpy.float16)
    with pytest.raises(TypeError):
        knn_query(3, xh, ch, ah, xh[:3].astype(numpy.float32))


def test_wrong_corpus_dtype(no_device):
    from kmcuda_amd import knn_query
    x, c, a = _corpus()
    with pytest.raises(TypeError):
        knn_query(3, x.astype(numpy.float64), c, a, x[:3])


def test_one_dimensional_queries(no_device):
    from kmcuda_amd import knn_query
    x, c, a = _corpus()
    with pytest.raises(ValueError):
        knn_query(3, x, c, a, x[0])


def test_query_assignments(no_device):
    from kmcuda_amd import knn_query
    x, c, a = _corpus()
    q = x[:5]
    with pytest.raises(ValueError):   # wrong length
        knn_query(3, x, c, a, q, query_assignments=numpy.zeros(4, numpy.uint32))
    with pytest.raises(ValueError):   # 2-D
        knn_query(3, x, c, a, q, query_assignments=numpy.zeros((5, 1), numpy.uint32))
    with pytest.raises(ValueError):   # a cluster id past K
        knn_query(3, x, c, a, q, query_assignments=numpy.array([0, 1, 2, 3, 4], numpy.uint32))
    with pytest.raises(TypeError):
        knn_query(3, x, c, a, q, query_assignments=numpy.zeros(5, numpy.float32))


def test_corpus_checks(no_device):
    from kmcuda_amd import knn_query
    x, c, a = _corpus()
    with pytest.raises(ValueError):
        knn_query(3, x, c, a[:-1], x[:3])
    with pytest.raises(ValueError):
        knn_query(3, x, c, a, x[:3], metric="manhattan")
    xh = numpy.zeros((8, 3), numpy.float16)
    with pytest.raises(ValueError):   # fp16x2: an even number of halves per row
        knn_query(2, xh, xh[:2], numpy.zeros(8, numpy.uint32), xh[:1])


def test_mixed_kinds_are_refused(no_device):
    torch = pytest.importorskip("torch")
    from kmcuda_amd import knn_query
    x, c, a = _corpus()
    with pytest.raises((TypeError, ValueError)):   # a host tensor is no device buffer
        knn_query(3, torch.from_numpy(x), c, a, x[:3])
