"""Rows added to a k-NN index in place (KnnIndex.add / info, C ABI kmamd_knn_index_add / kmamd_knn_index_info): the
surface, and the refusals that come before any device is touched."""
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"kmamd_knn_index_add": 7, "kmamd_knn_index_info": 4}
INVALID_ARGUMENTS = 1   # kmcudaInvalidArguments (include/kmcuda.h)


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_declared_in_the_header_with_the_issue_s_signature():
    header = _read("include", "kmcuda_amd.h")
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("int kmamd_knn_index_add(kmamd_knn_index *ix, uint32_t n_rows, const void *rows, const uint32_t *assignments , "
            "uint32_t *assignments_out , uint32_t *first_row , int32_t device_ptrs);") in flat
    assert ("int kmamd_knn_index_info(kmamd_knn_index *ix, uint32_t *n_rows, uint32_t *n_clustered, int *filter );") in flat
    # the contract the header states: add(B) is add(B, kmeans_predict(B, centroids)); not safe against concurrent calls
    assert "add(B) is exactly add(B, kmeans_predict(B, centroids))" in header
    assert "NOT safe against a concurrent call" in header


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
    from kmcuda_amd import _lib
    try:
        L = _lib.lib()
    except ImportError:
        pytest.skip("the HIP library has not been built")
    first = _lib.u32(7)
    assert L.kmamd_knn_index_add(None, 3, None, None, None, first, -1) == INVALID_ARGUMENTS
    assert first.value == 7
    assert L.kmamd_knn_index_add(None, 0, None, None, None, None, -1) == INVALID_ARGUMENTS
    assert L.kmamd_knn_index_info(None, None, None, None) == INVALID_ARGUMENTS


def test_python_surface():
    import kmcuda_amd
    from kmcuda_amd import KnnIndex
    assert kmcuda_amd.KnnIndex is KnnIndex
    sig = inspect.signature(KnnIndex.add)
    assert list(sig.parameters) == ["self", "rows", "assignments", "return_assignments"]
    assert sig.parameters["assignments"].default is None
    assert sig.parameters["return_assignments"].default is False
    assert list(inspect.signature(KnnIndex.info).parameters) == ["self"]


def test_closed_index_refuses():
    import numpy
    from kmcuda_amd import KnnIndex
    ix = KnnIndex.__new__(KnnIndex)   # an index that was never opened reads as closed
    ix.h = None
    with pytest.raises(ValueError):
        ix.add(numpy.zeros((2, 4), numpy.float32))
    with pytest.raises(ValueError):
        ix.info()


def test_switch_documented():
    assert "KMCUDA_AMD_KNN_ADD_CHUNK" in _read("INTEGRATION.md")
    assert "KMCUDA_AMD_KNN_ADD_CHUNK" in _read("kmcuda_amd", "csrc", "knn_host.cpp")
