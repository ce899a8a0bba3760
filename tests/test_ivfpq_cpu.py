"""The refusals of IVF-PQ search, on a machine without a device: the C ABI answers InvalidArguments
with the outputs bit for bit what they were -- any answer that came after a device call would be NoSuchDevice here --
and the Python calls raise before the library is asked for anything.  Only refused or empty calls are issued."""
import numpy
import pytest

from kmcuda_amd import IvfPqIndex, ivfpq, ivfpq_search, ivfpq_train

_Q, _L, _K, _M, _DSUB, _KSUB, _TOP, _NPROBE = 3, 100, 8, 4, 8, 16, 5, 2

# (what is wrong, the arguments that differ from a valid host call)
C_TABLE = [
    ("M = 0", dict(m=0, width=0)),
    ("M = 65", dict(m=65, width=65 * _DSUB)),
    ("dsub = 0", dict(dsub=0, width=0)),
    ("dsub = 65", dict(dsub=65, width=_M * 65)),
    ("ksub = 0", dict(ksub=0)),
    ("ksub = 257", dict(ksub=257)),
    ("L = 0", dict(rows=0)),
    ("L = 2^32 - 1", dict(rows=(1 << 32) - 1)),
    ("k = 0", dict(k=0)),
    ("k = 257", dict(k=257)),
    ("K = 0", dict(clusters=0)),
    ("nprobe = 0", dict(nprobe=0)),
    ("nprobe > K", dict(nprobe=_K + 1)),
    ("nprobe = 65", dict(clusters=100, nprobe=65)),
    ("query width", dict(width=_M * _DSUB + 1)),
    ("angular", dict(metric=1)),
    ("fp16", dict(fp16=1)),
    ("device = -1", dict(device=-1)),
    ("device_ptrs != device", dict(device_ptrs=1)),
    ("no probes", dict(probes=None)),
    ("no offsets", dict(offsets=None)),
]


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from kmcuda_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("what,over", C_TABLE, ids=[row[0] for row in C_TABLE])
def test_c_abi_refuses_with_outputs_untouched(what, over):
    floats, ints = numpy.zeros(65 * 257 * 65, numpy.float32), numpy.zeros(1000, numpy.uint32)
    a = dict(rows=_L, width=_M * _DSUB, clusters=_K, m=_M, dsub=_DSUB, ksub=_KSUB, k=_TOP, nprobe=_NPROBE, metric=0,
             fp16=0, device=0, device_ptrs=-1, probes=ints.ctypes.data, offsets=ints.ctypes.data)
    a.update(over)
    idx, dist = numpy.full((_Q, 257), 0x5A5A5A5A, numpy.uint32), numpy.full((_Q, 257), -7.5, numpy.float32)
    before = idx.tobytes(), dist.tobytes()
    rc = _lib().kmamd_ivfpq_search(_Q, a["rows"], a["width"], a["clusters"], a["m"], a["dsub"], a["ksub"], a["k"],
                                   a["nprobe"], a["metric"], a["fp16"], a["device"], a["device_ptrs"], 0,
                                   floats.ctypes.data, floats.ctypes.data, floats.ctypes.data, ints.ctypes.data,
                                   ints.ctypes.data, a["offsets"], a["probes"], idx.ctypes.data, dist.ctypes.data)
    assert rc == 1, what   # kmcudaInvalidArguments
    assert (idx.tobytes(), dist.tobytes()) == before, what


def test_residuals_refusals_and_empty_calls():
    L, x, a = _lib(), numpy.zeros((4, 8), numpy.float32), numpy.zeros(4, numpy.uint32)
    out = numpy.full((4, 8), -7.5, numpy.float32)
    for n, d, k, device, ptrs, rows in [(4, 0, 2, 0, -1, x), (4, 8, 0, 0, -1, x), (1 << 32, 8, 2, 0, -1, x),
                                        (4, 8, 2, -1, -1, x), (4, 8, 2, 0, 1, x), (4, 8, 2, 0, -1, None)]:
        assert L.kmamd_ivfpq_residuals(n, d, k, device, ptrs, 0, rows.ctypes.data if rows is not None else None,
                                       x.ctypes.data, a.ctypes.data, out.ctypes.data) == 1
    assert (out == -7.5).all()
    assert L.kmamd_ivfpq_residuals(0, 8, 2, 0, -1, 0, None, x.ctypes.data, None, None) == 0
    assert L.kmamd_ivfpq_search(0, _L, _M * _DSUB, _K, _M, _DSUB, _KSUB, _TOP, _NPROBE, 0, 0, 0, -1, 0, None,
                                x.ctypes.data, x.ctypes.data, a.ctypes.data, a.ctypes.data, a.ctypes.data, None, None,
                                None) == 0


_VALID = dict(queries=numpy.zeros((_Q, _M * _DSUB), numpy.float32),
              centroids=numpy.zeros((_K, _M * _DSUB), numpy.float32),
              codebooks=numpy.zeros((_M, _KSUB, _DSUB), numpy.float32), codes=numpy.zeros((_L, _M), numpy.uint8),
              ids=numpy.arange(_L, dtype=numpy.uint32), offsets=numpy.zeros(_K + 1, numpy.uint32),
              probes=numpy.zeros((_Q, _NPROBE), numpy.uint32), k=_TOP)
PY_TABLE = [
    ("M = 65", dict(queries=numpy.zeros((_Q, 65), numpy.float32), centroids=numpy.zeros((_K, 65), numpy.float32),
                    codebooks=numpy.zeros((65, 2, 1), numpy.float32), codes=numpy.zeros((_L, 65), numpy.uint8)),
     ValueError),
    ("dsub = 65", dict(codebooks=numpy.zeros((1, 2, 65), numpy.float32)), ValueError),
    ("ksub = 257", dict(codebooks=numpy.zeros((_M, 257, _DSUB), numpy.float32)), ValueError),
    ("codebooks of another width", dict(codebooks=numpy.zeros((_M, _KSUB, _DSUB - 1), numpy.float32)), ValueError),
    ("centroids of another width", dict(centroids=numpy.zeros((_K, 3), numpy.float32)), ValueError),
    ("L = 0", dict(codes=numpy.zeros((0, _M), numpy.uint8), ids=numpy.zeros(0, numpy.uint32)), ValueError),
    ("codes of another M", dict(codes=numpy.zeros((_L, 3), numpy.uint8)), ValueError),
    ("int32 codes", dict(codes=numpy.zeros((_L, _M), numpy.int32)), TypeError),
    ("ids of another length", dict(ids=numpy.zeros(_L - 1, numpy.uint32)), ValueError),
    ("float ids", dict(ids=numpy.zeros(_L, numpy.float32)), TypeError),
    ("offsets of K entries", dict(offsets=numpy.zeros(_K, numpy.uint32)), ValueError),
    ("probes of another Q", dict(probes=numpy.zeros((_Q + 1, _NPROBE), numpy.uint32)), ValueError),
    ("nprobe > K", dict(probes=numpy.zeros((_Q, _K + 1), numpy.uint32)), ValueError),
    ("nprobe = 0", dict(probes=numpy.zeros((_Q, 0), numpy.uint32)), ValueError),
    ("k = 0", dict(k=0), ValueError),
    ("k = 257", dict(k=257), ValueError),
    ("k = 2.0", dict(k=2.0), TypeError),
    ("fp16", dict(queries=numpy.zeros((_Q, _M * _DSUB), numpy.float16)), ValueError),
    ("float64", dict(centroids=numpy.zeros((_K, _M * _DSUB), numpy.float64)), TypeError),
    ("angular", dict(metric="cos"), ValueError),
    ("device = -1", dict(device=-1), ValueError),
]


@pytest.mark.parametrize("what,over,exc", PY_TABLE, ids=[row[0] for row in PY_TABLE])
def test_python_raises_before_the_library(monkeypatch, what, over, exc):
    from kmcuda_amd import _lib

    def no_library():
        raise AssertionError("the library was asked")
    monkeypatch.setattr(_lib, "lib", no_library)
    kw = dict(_VALID)
    kw.update(over)
    args = [kw.pop(n) for n in ("queries", "centroids", "codebooks", "codes", "ids", "offsets", "probes", "k")]
    with pytest.raises(exc):
        ivfpq_search(*args, **kw)


def test_train_and_index_raise_before_the_library(monkeypatch):
    from kmcuda_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was asked")))
    rows, cen, books = numpy.zeros((50, 32), numpy.float32), _VALID["centroids"], _VALID["codebooks"]
    for bad in (dict(subspaces=0), dict(subspaces=65), dict(subspaces=5), dict(subspaces=4, ksub=257),
                dict(subspaces=4, assignments=numpy.zeros(49, numpy.uint32)), dict(subspaces=4, metric="cos")):
        with pytest.raises(ValueError):
            ivfpq_train(rows, cen, **bad)
    with pytest.raises(ValueError):
        ivfpq_train(numpy.zeros((50, 130), numpy.float32), numpy.zeros((_K, 130), numpy.float32), 2)   # dsub = 65
    for r, c, b in ((rows[:, :31], cen, books), (rows, cen[:, :31], books), (rows, cen, books[:3]),
                    (rows[:0], cen, books)):
        with pytest.raises(ValueError):
            IvfPqIndex(r, c, b, assignments=numpy.zeros(len(r), numpy.uint32))
    index = IvfPqIndex.__new__(IvfPqIndex)
    index.device, index.verbosity, index.centroids = 0, 0, cen
    for nprobe in (0, _K + 1):
        with pytest.raises(ValueError):
            index.search(_VALID["queries"], 5, nprobe=nprobe)


def test_query_tile_and_row_split_mirrors():
    L = _lib()
    for k in (0, 1, 10, 32, 33, 100, 128, 129, 256, 257):
        for m in range(0, 67):
            assert ivfpq.query_tile(m, k) == L.kmamd_ivfpq_query_tile(m, k), (m, k)
    assert [ivfpq.query_tile(m, 10) for m in (1, 4, 5, 8, 10, 16, 32, 39, 40, 64)] == [16, 16, 8, 8, 4, 4, 4, 4, 2, 2]
    for tile in (0, 2, 4, 8, 16):
        for pairs in (0, 1, 2, 7, 100, 1023, 1024, 1025, 4095, 4096, 8191, 8192, 10 ** 6, (1 << 32) - 1):
            for rows in (0, 1, 255, 256, 257, 1213, 10 ** 6, (1 << 32) - 2):
                assert ivfpq.row_split(pairs, tile, rows) == L.kmamd_ivfpq_row_split(pairs, tile, rows)
    assert [ivfpq.row_split(p, 4, 10 ** 6) for p in (1, 100, 2044, 2045, 10 ** 5)] == [512, 21, 2, 1, 1]
    assert ivfpq.row_split(1, 4, 1213) == 5
