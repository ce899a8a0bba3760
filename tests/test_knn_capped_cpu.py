"""The capped search of the k-NN index (KnnIndex.query(max_distance=r), knn_query(max_distance=r); C ABI
kmamd_knn_index_query_capped / _query_probe_capped) without a GPU: the definition in executable form
(tests/_capped_ref.py) held to the oracle at cap = FLT_MAX, the truncation property on tie-free blobs, the prune being
fed by the cap, and the surface with the refusals that come before any device call."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy
import pytest

import oracle
from _capped_ref import FLT_MAX, NONE, Corpus, bits, capped_reference, truncated
from test_gpu_knn_edges import blobs, degenerate, unit_corpus
from test_gpu_knn_query_edges import batch, degenerate_queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"kmamd_knn_index_query_capped": 11, "kmamd_knn_index_query_probe_capped": 12}
INVALID_ARGUMENTS = 1   # kmcudaInvalidArguments (include/kmcuda.h)
KS = (10, 3, 40)

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def blob_fixture(d):
    """(x, c, a, q, Corpus): 1500 rows in 24 blobs, queries = fresh blob draws + far-outside rows + copies of corpus
    rows (test_gpu_knn_query_edges.batch)."""
    def make():
        x, c, a = blobs(1500, d, 24, 1.0, seed=100 + d, spread=0.05)
        q = batch(x, c, 0.05, seed=d, fresh=120)
        return x, c, a, q, Corpus(x, c, a)
    return cached(("blobs", d), make)


def tie_free(d):
    """The queries of blob_fixture(d) that have no two corpus rows at the same distance (most of them: 1500 float32
    distances collide now and then).  Truncation is a property of such inputs; the definition holds with ties too."""
    def make():
        _, _, _, q, corpus = blob_fixture(d)
        free = numpy.array([len(set(corpus._distances(row)[0])) == corpus.N for row in q])
        assert free.sum() >= 0.6 * len(q)
        return free
    return cached(("tie free", d), make)


def oracle_lists(d, k):
    x, c, a, q, _ = blob_fixture(d)
    return cached(("oracle", d, k), lambda: oracle.knn_query(k, x, c, a, q))


def same(got, ref, what):
    assert (got[0] == ref[0]).all(), what
    assert (bits(got[1]) == bits(ref[1])).all(), what


# ---- 1. the restatement is the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", [16, 64])
def test_restatement_is_the_oracle_on_blobs(d, k):
    _, _, _, q, corpus = blob_fixture(d)
    ref = oracle_lists(d, k)
    assert (ref[1] == FLT_MAX).sum() == 0 and len(q) <= 300
    same(capped_reference(k, corpus, q), ref, (d, k))
    same(capped_reference(k, corpus, q, cap=numpy.inf), ref, (d, k))


def test_restatement_is_the_oracle_on_degenerate_inputs():
    """NaN rows and centroids, empty and one-row clusters, duplicate rows; NaN / inf queries; k beyond the candidates
    (a filler tail)."""
    x, c, a, q, bad = degenerate_queries(16)
    assert (x.view(numpy.uint32) == degenerate(16)[0].view(numpy.uint32)).all() and len(bad) == 8 and len(q) <= 300
    corpus = Corpus(x, c, a)
    qa, _, _ = oracle.lloyd_assign(q, c)
    for k in (10, len(x)):
        qq, qaa = (q, qa) if k == 10 else (q[:6], qa[:6])
        ref = oracle.knn_query(k, x, c, a, qq, query_assignments=qaa)
        same(capped_reference(k, corpus, qq, qaa), ref, k)
    ref = oracle.knn_query(10, x, c, a, q, query_assignments=qa)
    assert (ref[0] == NONE).all(axis=1).any() and numpy.isnan(ref[1]).any()


def test_restatement_is_the_oracle_angular():
    n, K = 1200, 16
    x = unit_corpus(n, 16, seed=7)
    c = x[numpy.random.RandomState(7).choice(n, K, replace=False)].copy()
    a, _, _ = oracle.lloyd_assign(x, c, metric=oracle.COS)
    q = batch(x, c, 0.3, seed=8, fresh=80, unit=True)
    for k in (10, 3):
        same(capped_reference(k, Corpus(x, c, a, "angular"), q), oracle.knn_query(k, x, c, a, q, metric="angular"), k)


def test_restatement_is_the_oracle_half2():
    rs = numpy.random.RandomState(5)
    x = rs.randn(600, 32).astype(numpy.float16)
    c = x[rs.choice(600, 8, replace=False)].copy()
    a, _, _ = oracle.lloyd_assign(x.astype(numpy.float32), c.astype(numpy.float32))
    q = numpy.concatenate([rs.randn(60, 32), x[:10].astype(numpy.float64)]).astype(numpy.float16)
    ref = oracle.knn_query(10, x, c, a, q, half2=True)
    assert (bits(ref[1]) != bits(oracle.knn_query(10, x, c, a, q)[1])).any()   # the half2 arithmetic is in effect
    same(capped_reference(10, Corpus(x, c, a, half2=True), q), ref, "half2")


# ---- 2. truncation ----------------------------------------------------------------------------------------------------
def blob_caps(d, k):
    """0, percentiles of the oracle's k-th distances, one returned distance (inclusiveness), above every distance."""
    ref_nb, ref_dist = oracle_lists(d, k)
    kth = ref_dist[:, k - 1]
    caps = [0.0] + [float(numpy.float32(numpy.percentile(kth, p))) for p in (5, 25, 50, 75)]
    caps.append(float(ref_dist[len(ref_dist) // 2, k // 2]))
    caps.append(float(numpy.float32(ref_dist.max() * 1.5)))
    return caps


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", [16, 64])
def test_truncation(d, k):
    _, _, _, q, corpus = blob_fixture(d)
    ref = oracle_lists(d, k)
    caps = blob_caps(d, k)
    free = tie_free(d)
    cut = []
    for cap in caps:
        got = capped_reference(k, corpus, q, cap=cap)
        want = truncated(ref[0], ref[1], cap)
        same((got[0][free], got[1][free]), (want[0][free], want[1][free]), (d, k, cap))
        assert (bits(got[1]) == bits(want[1])).all(), (d, k, cap)   # (a tie can swap two indices, never a distance)
        cut.append(int((got[1] == FLT_MAX).sum()))
    # the cases are what they are meant to be: only copies of corpus rows survive cap 0, the percentiles cut some lists
    # and not others, the entry at exactly the cap is kept, the last cap cuts nothing
    assert 0 < ref[1].size - cut[0] <= 40 and cut[0] > cut[1] > cut[2] > cut[3] > cut[4] > 0 and cut[-1] == 0
    at = capped_reference(k, corpus, q, cap=caps[5])[1]
    assert (at == numpy.float32(caps[5])).any()


# ---- 3. the prune is fed by the cap -----------------------------------------------------------------------------------
def prune_fixture():
    """(x, c, a, q, cap): blobs wide enough to overlap, 100 fresh queries, the cap at the 10th percentile of the 10th
    distances.  Shared with tests/test_gpu_knn_capped.py."""
    def make():
        x, c, a = blobs(1500, 16, 24, 1.0, seed=116, spread=0.10)
        rs = numpy.random.RandomState(117)
        q = (c[rs.randint(0, 24, 100)] + rs.randn(100, 16) * 0.10).astype(numpy.float32)
        kth = oracle.knn_query(10, x, c, a, q)[1][:, 9]
        return x, c, a, q, float(numpy.float32(numpy.percentile(kth, 10)))
    return cached("prune", make)


def test_the_prune_is_fed_by_the_cap():
    x, c, a, q, cap = prune_fixture()
    corpus = Corpus(x, c, a)
    _, _, uncapped = capped_reference(10, corpus, q)
    _, _, capped = capped_reference(10, corpus, q, cap=cap)
    print("pairs in visited clusters: %d capped, %d uncapped, of %d" % (capped, uncapped, len(q) * len(x)))
    assert capped < uncapped <= len(q) * len(x)


# ---- 4. the surface ---------------------------------------------------------------------------------------------------
def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_declared_in_the_header():
    header = _read("include", "kmcuda_amd.h")
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    assert ("int kmamd_knn_index_query_capped(kmamd_knn_index *ix, uint32_t k, float max_distance, uint32_t n_queries, "
            "const void *queries, const uint32_t *query_assignments, uint32_t *neighbors, float *distances, "
            "uint32_t *query_assignments_out, int32_t device_ptrs, const uint8_t *allow );") in flat
    assert ("int kmamd_knn_index_query_probe_capped(kmamd_knn_index *ix, uint32_t k, float max_distance, "
            "uint32_t nprobe, uint32_t n_queries, const void *queries, const uint32_t *probes, uint32_t *neighbors, "
            "float *distances, uint32_t *probes_out, int32_t device_ptrs, const uint8_t *allow );") in flat
    assert "min(kth, r)" in header and "index 0 at FLT_MAX" in header


def _lib_or_skip():
    from kmcuda_amd import _lib
    try:
        return _lib, _lib.lib()
    except ImportError:
        pytest.skip("the HIP library has not been built")


def test_in_lib_exports_with_argtypes():
    from kmcuda_amd import _lib
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
    _lib, L = _lib_or_skip()
    for name, nargs in SYMBOLS.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
        assert fn.argtypes[2] is _lib.f32 and fn.restype is _lib.i32


def test_dynamic_symbols():
    from kmcuda_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("the HIP library has not been built")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in SYMBOLS:
        assert name in names


def test_python_surface():
    import kmcuda_amd
    from kmcuda_amd import KnnIndex, knn_query
    for fn in (KnnIndex.query, knn_query):
        params = list(inspect.signature(fn).parameters.values())[-2:]
        assert [p.name for p in params] == ["max_distance", "return_counts"]
        assert params[0].default is None and params[1].default is False
    assert "max_distance=" in kmcuda_amd.__doc__ and "max_distance=" in kmcuda_amd.knn_index.__doc__


def _tiny(n=40, d=4, K=3, nq=5, seed=0):
    rs = numpy.random.RandomState(seed)
    x = rs.randn(n, d).astype(numpy.float32)
    c = x[:K].copy()
    a, _, _ = oracle.lloyd_assign(x, c)
    return x, c, a, rs.randn(nq, d).astype(numpy.float32)


@pytest.mark.parametrize("bad,error", [(float("nan"), ValueError), (-1, ValueError), (-1e-30, ValueError),
                                       (numpy.float32("nan"), ValueError), ("1.0", TypeError), (None, None),
                                       ([1.0], TypeError), (True, TypeError), (numpy.ones(2), TypeError)])
def test_python_refuses_a_bad_cap_before_the_index_is_built(bad, error, monkeypatch):
    import kmcuda_amd.knn_index as ki
    from kmcuda_amd import knn_query

    class Built(Exception):
        pass

    def no_library():
        raise Built()
    monkeypatch.setattr(ki._lib, "lib", no_library)
    x, c, a, q = _tiny()
    with pytest.raises(error or Built):
        knn_query(2, x, c, a, q, max_distance=bad)


def test_an_open_index_refuses_a_bad_cap_before_the_library_is_called():
    from kmcuda_amd import KnnIndex
    ix = KnnIndex.__new__(KnnIndex)
    ix.h, ix.n_rows, ix.features, ix.clusters, ix.fp16, ix.device = ctypes.c_void_p(1), 40, 4, 3, False, 0
    ix.lib = None   # (any call into the library would fail on None)
    q = numpy.zeros((5, 4), numpy.float32)
    try:
        for bad, error in ((float("nan"), ValueError), (-0.5, ValueError), ("r", TypeError)):
            with pytest.raises(error):
                ix.query(q, 2, max_distance=bad)
    finally:
        ix.h = None


def test_the_cap_as_the_library_gets_it():
    from kmcuda_amd.knn_index import _check_max_distance, _real_counts
    assert _check_max_distance(None) is None
    assert _check_max_distance(0) == 0.0 and _check_max_distance(numpy.float64(0.1)) == float(numpy.float32(0.1))
    assert _check_max_distance(numpy.array(2.5)) == 2.5 and _check_max_distance(numpy.float16(2.5)) == 2.5
    assert _check_max_distance(float("inf")) == FLT_MAX and _check_max_distance(1e300) == FLT_MAX
    dist = numpy.array([[0.5, 1.0, FLT_MAX], [numpy.nan] * 3, [FLT_MAX] * 3, [0.0, 0.25, 0.5]], numpy.float32)
    assert _real_counts(dist, 1.0).tolist() == [2, 0, 0, 3] and _real_counts(dist, 1.0).dtype == numpy.uint32
    assert _real_counts(dist, 0.25).tolist() == [0, 0, 0, 2]
    assert _real_counts(dist, None).tolist() == [2, 0, 0, 3] and _real_counts(dist, FLT_MAX).tolist() == [3, 0, 3, 3]


def test_null_handle_and_bad_caps_are_refused_without_a_device():
    _lib, L = _lib_or_skip()
    nb = (_lib.u32 * 2)(5, 6)
    q = (_lib.f32 * 4)(0.0, 0.0, 0.0, 0.0)
    vp = lambda b: ctypes.cast(b, ctypes.c_void_p)   # noqa: E731
    fake = ctypes.c_void_p(8)   # (never dereferenced: the cap is looked at first)
    for h, cap in ((None, 1.0), (None, float("inf")), (fake, float("nan")), (fake, -1.0), (fake, -0.0 - 1e-30)):
        assert L.kmamd_knn_index_query_capped(h, 1, cap, 2, vp(q), None, vp(nb), None, None, -1,
                                              None) == INVALID_ARGUMENTS, (h, cap)
        assert L.kmamd_knn_index_query_probe_capped(h, 1, cap, 1, 2, vp(q), None, vp(nb), None, None, -1,
                                                    None) == INVALID_ARGUMENTS, (h, cap)
    assert list(nb) == [5, 6]
