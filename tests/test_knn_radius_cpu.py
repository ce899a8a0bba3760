"""Radius search on the k-NN index (kmcuda_amd.KnnIndex.query_radius / knn_query_radius, C ABI
kmamd_knn_index_radius_count / _fill): the surface and its argument checks, which all run before any device is touched."""
import os

import numpy
import pytest

NAMES = ("kmamd_knn_index_radius_count", "kmamd_knn_index_radius_fill")


def _corpus(n=64, d=8, k=4, dtype=numpy.float32):
    rng = numpy.random.default_rng(3)
    x = rng.standard_normal((n, d)).astype(dtype)
    c = x[:k].copy()
    a = (numpy.arange(n) % k).astype(numpy.uint32)
    return x, c, a


def test_importable_and_exported():
    import kmcuda_amd
    from kmcuda_amd import KnnIndex, knn_query_radius  # noqa: F401
    from kmcuda_amd import _lib
    assert callable(kmcuda_amd.knn_query_radius) and callable(KnnIndex.query_radius)
    for name in NAMES:
        assert name in _lib.EXPORTS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "kmcuda_amd.h")) as f:
        header = f.read()
    for name in NAMES:
        assert name + "(" in header


def test_library_symbols():
    from kmcuda_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("the HIP library has not been built")
    L = _lib.lib()   # (a library that is there and does not load is a failure)
    for name in NAMES:
        fn = getattr(L, name)
        assert fn is not None and fn.argtypes[1] is _lib.f32


@pytest.fixture
def no_device(monkeypatch):
    """Fails the test if the library is loaded at all: validation must come first."""
    from kmcuda_amd import _lib

    def boom():
        raise AssertionError("the device library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", boom)


@pytest.mark.parametrize("radius", [-1.0, -1e-30, float("nan"), float("inf"), 1e39, 10 ** 400])
def test_radius_range(no_device, radius):
    from kmcuda_amd import knn_query_radius
    x, c, a = _corpus()
    with pytest.raises(ValueError):
        knn_query_radius(radius, x, c, a, x[:3])


@pytest.mark.parametrize("radius", ["1", None, True, [1.0], numpy.ones(2, numpy.float32), 1j])
def test_radius_type(no_device, radius):
    from kmcuda_amd import knn_query_radius
    x, c, a = _corpus()
    with pytest.raises(TypeError):
        knn_query_radius(radius, x, c, a, x[:3])


def test_sort_needs_distances(no_device):
    from kmcuda_amd import knn_query_radius
    x, c, a = _corpus()
    with pytest.raises(ValueError):
        knn_query_radius(1.0, x, c, a, x[:3], return_distances=False, sort=True)


def test_feature_mismatch(no_device):
    from kmcuda_amd import knn_query_radius
    x, c, a = _corpus()
    with pytest.raises(ValueError):
        knn_query_radius(1.0, x, c, a, numpy.zeros((5, 7), numpy.float32))
    with pytest.raises(ValueError):
        knn_query_radius(1.0, x, c[:, :7], a, x[:3])
    with pytest.raises(ValueError):
        knn_query_radius(1.0, x, c, a, x[0])


@pytest.mark.parametrize("dtype", [numpy.float64, numpy.int32, numpy.float16])
def test_wrong_query_dtype(no_device, dtype):
    from kmcuda_amd import knn_query_radius
    x, c, a = _corpus()
    with pytest.raises(TypeError):
        knn_query_radius(1.0, x, c, a, x[:3].astype(dtype))


def test_half_corpus_wants_half_queries(no_device):
    from kmcuda_amd import knn_query_radius
    xh, ch, ah = _corpus(dtype=numpy.float16)
    with pytest.raises(TypeError):
        knn_query_radius(1.0, xh, ch, ah, xh[:3].astype(numpy.float32))


def test_query_assignments(no_device):
    from kmcuda_amd import knn_query_radius
    x, c, a = _corpus()
    q = x[:5]
    with pytest.raises(ValueError):   # wrong length
        knn_query_radius(1.0, x, c, a, q, query_assignments=numpy.zeros(4, numpy.uint32))
    with pytest.raises(ValueError):   # 2-D
        knn_query_radius(1.0, x, c, a, q, query_assignments=numpy.zeros((5, 1), numpy.uint32))
    with pytest.raises(ValueError):   # a cluster id past K
        knn_query_radius(1.0, x, c, a, q, query_assignments=numpy.array([0, 1, 2, 3, 4], numpy.uint32))
    with pytest.raises(TypeError):
        knn_query_radius(1.0, x, c, a, q, query_assignments=numpy.zeros(5, numpy.float32))


def test_corpus_checks(no_device):
    from kmcuda_amd import knn_query_radius
    x, c, a = _corpus()
    with pytest.raises(ValueError):
        knn_query_radius(1.0, x, c, a[:-1], x[:3])
    with pytest.raises(ValueError):
        knn_query_radius(1.0, x, c, a, x[:3], metric="manhattan")
    with pytest.raises(TypeError):
        knn_query_radius(1.0, x.astype(numpy.float64), c, a, x[:3])


def test_method_checks_before_the_library(no_device):
    """KnnIndex.query_radius on an index object that never reached the device: the same checks, in the same place."""
    from kmcuda_amd import KnnIndex
    ix = KnnIndex.__new__(KnnIndex)
    ix.h, ix.lib = 1, None
    ix.n_rows, ix.features, ix.clusters, ix.fp16, ix.device = 64, 8, 4, False, 0
    x, _, _ = _corpus()
    with pytest.raises(ValueError):
        ix.query_radius(x[:3], -0.5)
    with pytest.raises(TypeError):
        ix.query_radius(x[:3], "wide")
    with pytest.raises(ValueError):
        ix.query_radius(x[:3], 1.0, return_distances=False, sort=True)
    with pytest.raises(ValueError):
        ix.query_radius(x[:3, :7], 1.0)
    ix.h = None
    with pytest.raises(ValueError):
        ix.query_radius(x[:3], 1.0)
