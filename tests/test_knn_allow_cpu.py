"""The allow-mask of the k-NN index queries (KnnIndex.query(allow=), knn_query(allow=); C ABI kmamd_knn_index_query_allow
/ _query_probe_allow / _radii_allow) without a GPU: the surface, the refusals that come before any
device call, the pack rule of the device's mask preparation restated in numpy, and the definition itself on the CPU
oracle -- a masked search is the search on the assignments with every denied row's set to K."""
import inspect
import os
import re
import subprocess

import numpy
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"kmamd_knn_index_query_allow": 10, "kmamd_knn_index_query_probe_allow": 11, "kmamd_knn_index_radii_allow": 4}
INVALID_ARGUMENTS = 1   # kmcudaInvalidArguments (include/kmcuda.h)
NONE = 0xFFFFFFFF
FLT_MAX = numpy.finfo(numpy.float32).max
PAD_ROWS = 64           # KNN16_PAD_ROWS (kmcuda_amd/csrc/kernels.hpp)


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ---- the surface ----------------------------------------------------------------------------------------------------
def test_declared_in_the_header():
    header = _read("include", "kmcuda_amd.h")
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    assert ("int kmamd_knn_index_query_allow(kmamd_knn_index *ix, uint32_t k, uint32_t n_queries, const void *queries, "
            "const uint32_t *query_assignments, uint32_t *neighbors, float *distances, uint32_t *query_assignments_out, "
            "int32_t device_ptrs, const uint8_t *allow );") in flat
    assert ("int kmamd_knn_index_query_probe_allow(kmamd_knn_index *ix, uint32_t k, uint32_t nprobe, uint32_t n_queries, "
            "const void *queries, const uint32_t *probes , uint32_t *neighbors, float *distances , uint32_t *probes_out , "
            "int32_t device_ptrs, const uint8_t *allow );") in flat
    assert "int kmamd_knn_index_radii_allow(kmamd_knn_index *ix, const uint8_t *allow , int32_t device_ptrs , float *radii_host );" in flat
    # the contract: what is out of scope and what does not exist is said where a caller reads it
    assert "NO masked f32 filter" in header
    assert "Radius search" in header and "takes no mask" in header
    assert "KNN16_PAD_ROWS 64" in _read("kmcuda_amd", "csrc", "kernels.hpp")


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
    import ctypes
    from kmcuda_amd import _lib
    try:
        L = _lib.lib()
    except ImportError:
        pytest.skip("the HIP library has not been built")
    allow = (ctypes.c_uint8 * 4)(1, 1, 0, 1)
    nb = (_lib.u32 * 2)(5, 6)
    q = (_lib.f32 * 4)(0.0, 0.0, 0.0, 0.0)
    vp = lambda b: ctypes.cast(b, ctypes.c_void_p)   # noqa: E731
    assert L.kmamd_knn_index_query_allow(None, 1, 2, vp(q), None, vp(nb), None, None, -1, vp(allow)) == INVALID_ARGUMENTS
    assert L.kmamd_knn_index_query_probe_allow(None, 1, 1, 2, vp(q), None, vp(nb), None, None, -1,
                                               vp(allow)) == INVALID_ARGUMENTS
    assert list(nb) == [5, 6]
    radii = (_lib.f32 * 2)(1.0, 2.0)
    assert L.kmamd_knn_index_radii_allow(None, vp(allow), -1, vp(radii)) == INVALID_ARGUMENTS
    assert list(radii) == [1.0, 2.0]


def test_python_surface():
    import kmcuda_amd
    from kmcuda_amd import KnnIndex, knn_query
    assert inspect.signature(KnnIndex.query).parameters["allow"].default is None
    assert inspect.signature(knn_query).parameters["allow"].default is None
    assert "allow" not in inspect.signature(KnnIndex.query_radius).parameters   # out of scope, and documented as such
    assert list(inspect.signature(KnnIndex.radii_allow).parameters) == ["self", "allow"]
    assert "allow=" in kmcuda_amd.__doc__ and "allow=" in kmcuda_amd.knn_index.__doc__
    assert "query_radius takes no mask" in re.sub(r"\s+", " ", kmcuda_amd.knn_index.__doc__)


# ---- refused arguments, before any device call ----------------------------------------------------------------------
def _corpus(n=40, d=4, K=3, nq=5, seed=0):
    rs = numpy.random.RandomState(seed)
    x = rs.rand(n, d).astype(numpy.float32)
    c = rs.rand(K, d).astype(numpy.float32)
    a = rs.randint(0, K, n).astype(numpy.uint32)
    q = rs.rand(nq, d).astype(numpy.float32)
    return x, c, a, q


class Refuses:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def test_knn_query_refuses_a_bad_mask_before_the_index_is_built(monkeypatch):
    """Wrong length, 2-D, a float dtype, a mask on the other side than the queries: each raises, and neither the library
    nor a device has been touched (the loader itself is replaced by one that fails the test)."""
    from kmcuda_amd import _lib, knn_query
    monkeypatch.setattr(_lib, "lib", lambda: Refuses())
    x, c, a, q = _corpus()
    n = len(x)
    with pytest.raises(ValueError):
        knn_query(3, x, c, a, q, allow=numpy.ones(n - 1, bool))
    with pytest.raises(ValueError):
        knn_query(3, x, c, a, q, allow=numpy.ones(n + 1, numpy.uint8))
    with pytest.raises(ValueError):
        knn_query(3, x, c, a, q, allow=numpy.ones((n, 1), bool))
    with pytest.raises(ValueError):
        knn_query(3, x, c, a, q, nprobe=2, allow=numpy.ones((1, n), numpy.uint8))
    for bad in (numpy.ones(n, numpy.float32), numpy.ones(n, numpy.float64), numpy.ones(n, numpy.int32),
                numpy.ones(n, numpy.int8), [True] * n):
        with pytest.raises(TypeError):
            knn_query(3, x, c, a, q, allow=bad)
        with pytest.raises(TypeError):
            knn_query(3, x, c, a, q, nprobe=2, allow=bad)
    torch = pytest.importorskip("torch")
    # numpy queries, a tensor mask: the other side
    for mask in (torch.ones(n, dtype=torch.bool), torch.ones(n, dtype=torch.uint8)):
        with pytest.raises(TypeError):
            knn_query(3, x, c, a, q, allow=mask)


def test_an_open_index_refuses_a_bad_mask_before_the_library_is_called():
    from kmcuda_amd import KnnIndex
    ix = KnnIndex.__new__(KnnIndex)
    ix.h, ix.lib, ix.n_rows, ix.features, ix.clusters, ix.fp16, ix.device = 1, Refuses(), 10, 4, 3, False, 0
    q = numpy.zeros((2, 4), numpy.float32)
    for bad in (numpy.ones(9, bool), numpy.ones(11, bool), numpy.ones((10, 1), numpy.uint8)):
        with pytest.raises(ValueError):
            ix.query(q, 2, allow=bad)
        with pytest.raises(ValueError):
            ix.radii_allow(bad)
    for bad in (numpy.ones(10, numpy.float32), numpy.ones(10, numpy.int64), [1] * 10, None):
        if bad is not None:
            with pytest.raises(TypeError):
                ix.query(q, 2, nprobe=2, allow=bad)
        with pytest.raises(TypeError):
            ix.radii_allow(bad)
    ix.h = None   # (nothing to destroy)


def test_the_mask_is_handed_over_as_contiguous_bytes():
    from kmcuda_amd.knn_index import _check_allow
    m = numpy.zeros(20, bool)
    m[::3] = True
    for given in (m, m.astype(numpy.uint8), numpy.repeat(m, 2)[::2], (m * 7).astype(numpy.uint8)):
        out = _check_allow(given, 20, False, 0)
        assert out.dtype == numpy.uint8 and out.flags.c_contiguous and out.shape == (20,)
        assert ((out != 0) == m).all()
    assert _check_allow(None, 20, False, 0) is None


# ---- the pack rule --------------------------------------------------------------------------------------------------
def pack(allow, assignments, K):
    """What the device's mask preparation writes, in numpy: 64-bit words over the SORTED positions, bit[p] =
    allow[order[p]] != 0 for the positions that have a cluster, zeros from the last clustered row on, through the f16
    filter's tile padding and one word further."""
    a = numpy.asarray(assignments, dtype=numpy.uint32)
    n = len(a)
    order = numpy.argsort(numpy.minimum(a, K), kind="stable")
    assigned = int((a < K).sum())
    nwords = (n + PAD_ROWS + 63) // 64 + 1
    bit = numpy.zeros(nwords * 64, bool)
    bit[:assigned] = numpy.asarray(allow)[order[:assigned]] != 0
    return numpy.packbits(bit, bitorder="little").view(numpy.uint64), order


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_pack_rule(n):
    rs = numpy.random.RandomState(n)
    K = 5
    a = rs.randint(0, K + 2, n).astype(numpy.uint32)   # K and K + 1: no cluster
    allow = (rs.rand(n) < 0.5).astype(numpy.uint8) * rs.randint(1, 255, n).astype(numpy.uint8)
    words, order = pack(allow, a, K)
    assert len(words) == (n + 64 + 63) // 64 + 1
    words32 = words.view(numpy.uint32)
    assigned = int((a < K).sum())
    # order is the index's: clusters ascending, row ids ascending inside one, the rows without a cluster last
    assert (numpy.diff(numpy.minimum(a[order], K)) >= 0).all()
    for p in range(len(words) * 64):
        got = (int(words32[p >> 5]) >> (p & 31)) & 1          # how the search kernels read it
        want = int(p < assigned and allow[order[p]] != 0)
        assert got == want, p
    # a sub-tile's 32 bits from two words, as the f16 search takes them at any tile base
    for base in range(0, n, 7):
        two = (int(words32[(base >> 5) + 1]) << 32) | int(words32[base >> 5])
        sub = (two >> (base & 31)) & 0xFFFFFFFF
        for rho in range(32):
            p = base + rho
            assert (sub >> rho) & 1 == int(p < assigned and allow[order[p]] != 0)
    # the flag of a row without a cluster is ignored
    flipped = allow.copy()
    flipped[a >= K] ^= 1
    assert (pack(flipped, a, K)[0] == words).all()


# ---- the definition, on the oracle ----------------------------------------------------------------------------------
def test_the_definition_on_the_oracle():
    """oracle.knn_query on the assignments with the denied rows' set to K equals a brute-force search over the allowed
    rows in float64, on data without near ties; all-true is the plain call; all-false the all-filler result."""
    rs = numpy.random.RandomState(3)
    n, d, K, nq, k = 600, 8, 6, 60, 5
    centres = rs.rand(K, d) * 10
    x = (centres[rs.randint(0, K, n)] + rs.randn(n, d)).astype(numpy.float32)
    c = centres.astype(numpy.float32)
    a, _, _ = oracle.lloyd_assign(x, c)
    a[::50] = K                                     # some rows have no cluster whatever the mask says
    q = (centres[rs.randint(0, K, nq)] + rs.randn(nq, d)).astype(numpy.float32)
    allow = rs.rand(n) < 0.4
    allow[a == 2] = False                           # a cluster without an allowed row
    ap = numpy.where(allow, a, K).astype(numpy.uint32)
    nb, dist = oracle.knn_query(k, x, c, ap, q)
    rows = numpy.nonzero(allow & (a < K))[0]
    d2 = ((q[:, None, :].astype(numpy.float64) - x[rows][None].astype(numpy.float64)) ** 2).sum(-1)
    order = numpy.argsort(d2, axis=1, kind="stable")[:, :k]
    gaps = numpy.diff(numpy.sort(d2, axis=1)[:, :k + 1], axis=1)
    assert (gaps > 1e-4).all()                      # (separated: float32 rounding cannot reorder them)
    assert (nb == rows[order]).all()
    assert numpy.allclose(dist, numpy.sqrt(numpy.take_along_axis(d2, order, axis=1)), rtol=1e-5)
    assert not numpy.isin(nb, numpy.nonzero(~allow)[0]).any()
    # every flag set: the unmasked call
    full = oracle.knn_query(k, x, c, numpy.where(numpy.ones(n, bool), a, K).astype(numpy.uint32), q)
    plain = oracle.knn_query(k, x, c, a, q)
    assert (full[0] == plain[0]).all() and (full[1].view(numpy.uint32) == plain[1].view(numpy.uint32)).all()
    # no row allowed: index 0 at FLT_MAX; a NaN query: no neighbours
    q2 = q.copy()
    q2[7, 3] = numpy.nan
    nb0, dist0 = oracle.knn_query(k, x, c, numpy.full(n, K, numpy.uint32), q2)
    fin = numpy.arange(nq) != 7
    assert (nb0[fin] == 0).all() and (dist0[fin] == FLT_MAX).all()
    assert (nb0[7] == NONE).all() and numpy.isnan(dist0[7]).all()
    # fewer allowed rows than k: the tail stays at the filler
    few = numpy.zeros(n, bool)
    few[rows[:3]] = True
    nb3, dist3 = oracle.knn_query(k, x, c, numpy.where(few, a, K).astype(numpy.uint32), q)
    assert (numpy.sort(nb3[:, :3], axis=1) == numpy.sort(rows[:3])).all()
    assert (nb3[:, 3:] == 0).all() and (dist3[:, 3:] == FLT_MAX).all()
