"""Rows removed from a k-NN index in place (KnnIndex.remove / radii, C ABI kmamd_knn_index_remove / kmamd_knn_index_radii):
the surface, and the refusals that come before any device is touched."""
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"kmamd_knn_index_remove": 5, "kmamd_knn_index_radii": 2}
INVALID_ARGUMENTS = 1   # kmcudaInvalidArguments (include/kmcuda.h)


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_declared_in_the_header_with_the_issue_s_signature():
    header = _read("include", "kmcuda_amd.h")
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("int kmamd_knn_index_remove(kmamd_knn_index *ix, uint32_t n_ids, const uint32_t *ids, uint32_t *n_removed , "
            "int32_t device_ptrs);") in flat
    assert "int kmamd_knn_index_radii(kmamd_knn_index *ix, float *radii );" in flat
    # the contract the header states: no reclaimed memory, not safe against concurrent calls (worded as add's)
    assert "Memory is NOT reclaimed" in header
    assert header.count("NOT safe against a concurrent call on the same index") >= 2


def test_exported_by_the_version_script():
    script = _read("kmcuda_amd", "csrc", "exports.map")
    assert "kmamd_*;" in script   # every kmamd_ symbol leaves the library


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
        assert fn.restype is _lib.i32


def test_dynamic_symbols():
    from kmcuda_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("the HIP library has not been built")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in SYMBOLS:
        assert name in names


def test_null_handle_is_refused_without_a_device():
    """Both calls look at the handle first: no device is opened for a null one (this test runs without a GPU)."""
    import ctypes
    from kmcuda_amd import _lib
    try:
        L = _lib.lib()
    except ImportError:
        pytest.skip("the HIP library has not been built")
    ids = (_lib.u32 * 3)(0, 1, 2)
    lost = _lib.u32(7)
    assert L.kmamd_knn_index_remove(None, 3, ctypes.cast(ids, ctypes.c_void_p), lost, -1) == INVALID_ARGUMENTS
    assert lost.value == 7
    assert L.kmamd_knn_index_remove(None, 0, None, lost, -1) == INVALID_ARGUMENTS
    assert lost.value == 7
    radii = (_lib.f32 * 4)(1.0, 2.0, 3.0, 4.0)
    assert L.kmamd_knn_index_radii(None, ctypes.cast(radii, ctypes.c_void_p)) == INVALID_ARGUMENTS
    assert list(radii) == [1.0, 2.0, 3.0, 4.0]


def test_python_surface():
    import kmcuda_amd
    from kmcuda_amd import KnnIndex
    assert kmcuda_amd.KnnIndex is KnnIndex
    assert str(inspect.signature(KnnIndex.remove)) == "(self, ids)"
    assert list(inspect.signature(KnnIndex.radii).parameters) == ["self"]
    assert "remove" in kmcuda_amd.__doc__ and "remove" in kmcuda_amd.knn_index.__doc__


def test_closed_index_refuses():
    import numpy
    from kmcuda_amd import KnnIndex
    ix = KnnIndex.__new__(KnnIndex)   # an index that was never opened reads as closed
    ix.h = None
    with pytest.raises(ValueError):
        ix.remove(numpy.zeros(2, numpy.uint32))
    with pytest.raises(ValueError):
        ix.radii()


def test_ids_are_checked_before_the_library_is_called():
    """Wrong dtype: TypeError; wrong rank or an id outside [0, n_rows): ValueError -- on an index whose handle would
    crash the library if it were ever passed on."""
    import numpy
    from kmcuda_amd import KnnIndex

    class Refuses:
        def __getattr__(self, name):
            raise AssertionError("the library was called (%s)" % name)

    ix = KnnIndex.__new__(KnnIndex)
    ix.h, ix.lib, ix.n_rows, ix.device = 1, Refuses(), 10, 0
    for bad in (numpy.zeros(2, numpy.float32), numpy.zeros(2, bool), [0.5, 1.0]):
        with pytest.raises(TypeError):
            ix.remove(bad)
    for bad in (numpy.zeros((2, 1), numpy.uint32), numpy.array([3, 10]), numpy.array([-1, 2]), [[1]]):
        with pytest.raises(ValueError):
            ix.remove(bad)
    ix.h = None   # (nothing to destroy)


def test_switch_documented():
    assert "KMCUDA_AMD_KNN_REMOVE_TIME" in _read("INTEGRATION.md")
    assert "KMCUDA_AMD_KNN_REMOVE_TIME" in _read("kmcuda_amd", "csrc", "knn_host.cpp")
