"""The allow-mask of radius search (KnnIndex.query_radius_allow, knn_query_radius(allow=); C ABI
kmamd_knn_index_radius_count_allow / _fill_allow) without a GPU: the surface and the refusals that come
before any device call."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy
import pytest

from test_knn_allow_cpu import INVALID_ARGUMENTS, Refuses, _corpus, _read

SYMBOLS = {"kmamd_knn_index_radius_count_allow": 9, "kmamd_knn_index_radius_fill_allow": 10}


# ---- the surface ----------------------------------------------------------------------------------------------------
def test_declared_in_the_header():
    header = _read("include", "kmcuda_amd.h")
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    assert ("int kmamd_knn_index_radius_count_allow(kmamd_knn_index *ix, float radius, uint32_t n_queries, "
            "const void *queries, const uint32_t *query_assignments, uint32_t *counts, uint32_t *query_assignments_out, "
            "int32_t device_ptrs, const uint8_t *allow );") in flat
    assert ("int kmamd_knn_index_radius_fill_allow(kmamd_knn_index *ix, float radius, uint32_t n_queries, "
            "const void *queries, const uint32_t *query_assignments, const uint64_t *offsets, uint32_t *neighbors, "
            "float *distances , int32_t device_ptrs, const uint8_t *allow );") in flat
    # the unmasked pair keeps its signatures
    assert ("int kmamd_knn_index_radius_count(kmamd_knn_index *ix, float radius, uint32_t n_queries, const void *queries, "
            "const uint32_t *query_assignments, uint32_t *counts, uint32_t *query_assignments_out, "
            "int32_t device_ptrs);") in flat
    assert ("int kmamd_knn_index_radius_fill(kmamd_knn_index *ix, float radius, uint32_t n_queries, const void *queries, "
            "const uint32_t *query_assignments, const uint64_t *offsets , uint32_t *neighbors, float *distances , "
            "int32_t device_ptrs);") in flat
    # the contract is said where a caller reads it
    text = re.sub(r"[\s*]+", " ", header)
    for said in ("allow[i] != 0", "the flag of a row that has no cluster is ignored", "every count is 0",
                 "a count under one mask followed by a fill under another",
                 "n_queries == 0 is success before the mask is looked at",
                 "allow == NULL is exactly kmamd_knn_index_radius_count / _fill"):
        assert said in text, said


def test_in_lib_exports_with_argtypes():
    from kmcuda_amd import _lib
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
    try:
        L = _lib.lib()
    except ImportError:
        pytest.skip("the HIP library has not been built")
    for name, nargs in SYMBOLS.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
        assert fn.argtypes[1] is _lib.f32 and fn.restype is _lib.i32


def test_dynamic_symbols():
    from kmcuda_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("the HIP library has not been built")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in SYMBOLS:
        assert name in names


def test_null_handle_is_refused_without_a_device():
    from kmcuda_amd import _lib
    try:
        L = _lib.lib()
    except ImportError:
        pytest.skip("the HIP library has not been built")
    allow = (ctypes.c_uint8 * 4)(1, 1, 0, 1)
    q = (_lib.f32 * 4)(0.0, 0.0, 0.0, 0.0)
    counts = (_lib.u32 * 2)(5, 6)
    offsets = (ctypes.c_uint64 * 3)(0, 1, 2)
    nb = (_lib.u32 * 2)(7, 8)
    dist = (_lib.f32 * 2)(1.0, 2.0)
    vp = lambda b: ctypes.cast(b, ctypes.c_void_p)   # noqa: E731
    assert L.kmamd_knn_index_radius_count_allow(None, 1.0, 2, vp(q), None, vp(counts), None, -1,
                                                vp(allow)) == INVALID_ARGUMENTS
    assert L.kmamd_knn_index_radius_fill_allow(None, 1.0, 2, vp(q), None, vp(offsets), vp(nb), vp(dist), -1,
                                               vp(allow)) == INVALID_ARGUMENTS
    # (a null handle is refused before n_queries == 0 is success, as in the unmasked pair)
    assert L.kmamd_knn_index_radius_count_allow(None, 1.0, 0, None, None, None, None, -1, None) == INVALID_ARGUMENTS
    assert list(counts) == [5, 6] and list(nb) == [7, 8] and list(dist) == [1.0, 2.0]


def test_python_surface():
    import kmcuda_amd
    from kmcuda_amd import KnnIndex, knn_query_radius
    assert list(inspect.signature(KnnIndex.query_radius_allow).parameters) == [
        "self", "queries", "radius", "allow", "query_assignments", "return_distances", "sort", "count_only"]
    p = inspect.signature(KnnIndex.query_radius_allow).parameters
    assert p["allow"].default is inspect.Parameter.empty and p["query_assignments"].default is None
    assert p["return_distances"].default is True and p["sort"].default is False and p["count_only"].default is False
    assert inspect.signature(knn_query_radius).parameters["allow"].default is None
    assert "allow" not in inspect.signature(KnnIndex.query_radius).parameters
    doc = re.sub(r"\s+", " ", kmcuda_amd.knn_index.__doc__)
    assert "query_radius_allow(queries, radius, mask)" in doc
    assert "query_radius_allow" in kmcuda_amd.__doc__


# ---- refused arguments, before any device call ----------------------------------------------------------------------
def bad_masks(n):
    """(exception, mask) for an index of n rows and numpy queries."""
    out = [(ValueError, numpy.ones(n - 1, bool)), (ValueError, numpy.ones(n + 1, numpy.uint8)),
           (ValueError, numpy.ones((n, 1), bool)), (ValueError, numpy.ones((1, n), numpy.uint8))]
    out += [(TypeError, bad) for bad in (numpy.ones(n, numpy.float32), numpy.ones(n, numpy.float64),
                                         numpy.ones(n, numpy.int32), numpy.ones(n, numpy.int8), [True] * n)]
    return out


def test_knn_query_radius_refuses_a_bad_mask_before_the_index_is_built(monkeypatch):
    from kmcuda_amd import _lib, knn_query_radius
    monkeypatch.setattr(_lib, "lib", lambda: Refuses())
    x, c, a, q = _corpus()
    n = len(x)
    for exc, bad in bad_masks(n):
        for count_only in (False, True):
            with pytest.raises(exc):
                knn_query_radius(0.5, x, c, a, q, allow=bad, count_only=count_only)
    torch = pytest.importorskip("torch")
    for mask in (torch.ones(n, dtype=torch.bool), torch.ones(n, dtype=torch.uint8)):   # numpy queries, a tensor mask
        with pytest.raises(TypeError):
            knn_query_radius(0.5, x, c, a, q, allow=mask)
    # the radius and the flags are still checked, and first
    with pytest.raises(ValueError):
        knn_query_radius(-1.0, x, c, a, q, allow=numpy.ones(n, bool))
    with pytest.raises(ValueError):
        knn_query_radius(0.5, x, c, a, q, allow=numpy.ones(n, bool), return_distances=False, sort=True)


def test_an_open_index_refuses_a_bad_mask_before_the_library_is_called():
    from kmcuda_amd import KnnIndex
    ix = KnnIndex.__new__(KnnIndex)
    ix.h, ix.lib, ix.n_rows, ix.features, ix.clusters, ix.fp16, ix.device = 1, Refuses(), 10, 4, 3, False, 0
    q = numpy.zeros((2, 4), numpy.float32)
    for exc, bad in bad_masks(10) + [(TypeError, None)]:
        for count_only in (False, True):
            with pytest.raises(exc):
                ix.query_radius_allow(q, 0.5, bad, count_only=count_only)
    with pytest.raises(TypeError):
        ix.query_radius_allow(q, 0.5)   # the mask is not optional here
    with pytest.raises(ValueError):
        ix.query_radius_allow(q, -0.5, numpy.ones(10, bool))
    with pytest.raises(ValueError):
        ix.query_radius_allow(q[:, :3], 0.5, numpy.ones(10, bool))
    ix.h = None   # (nothing to destroy)
    with pytest.raises(ValueError):
        ix.query_radius_allow(q, 0.5, numpy.ones(10, bool))
