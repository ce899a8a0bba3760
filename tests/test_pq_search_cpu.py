"""The refusals of pq_search, on a machine without a device: the C ABI answers InvalidArguments with
the outputs bit for bit what they were -- any answer that came after a device call would be NoSuchDevice here -- and
the Python call raises before the library is asked for anything.  Only refused or empty calls are issued."""
import numpy
import pytest

from kmcuda_amd import pq, pq_search

_Q, _N, _M, _DSUB, _KSUB, _K = 3, 100, 4, 8, 16, 5

# (what is wrong, the arguments that differ from a valid host call)
C_TABLE = [
    ("M = 0", dict(m=0, width=0)),
    ("M = 65", dict(m=65, width=65 * _DSUB)),
    ("dsub = 0", dict(dsub=0, width=0)),
    ("dsub = 65", dict(dsub=65, width=_M * 65)),
    ("ksub = 0", dict(ksub=0)),
    ("ksub = 257", dict(ksub=257)),
    ("N = 0", dict(n=0)),
    ("N = 2^32", dict(n=1 << 32)),
    ("k = 0", dict(k=0)),
    ("k > N", dict(n=4)),
    ("k = 257", dict(n=1000, k=257)),
    ("query width", dict(width=_M * _DSUB + 1)),
    ("angular", dict(metric=1)),
    ("fp16", dict(fp16=1)),
    ("device = -1", dict(device=-1)),
    ("device_ptrs != device", dict(device_ptrs=1)),
]


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from kmcuda_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("what,over", C_TABLE, ids=[row[0] for row in C_TABLE])
def test_c_abi_refuses_with_outputs_untouched(what, over):
    a = dict(q=_Q, n=_N, width=_M * _DSUB, m=_M, dsub=_DSUB, ksub=_KSUB, k=_K, metric=0, fp16=0, device=0,
             device_ptrs=-1)
    a.update(over)
    queries, books = numpy.zeros((_Q, 65 * 65), numpy.float32), numpy.zeros((65, 257, 65), numpy.float32)
    codes = numpy.zeros((1000, 65), numpy.uint8)
    idx, dist = numpy.full((_Q, 257), 0x5A5A5A5A, numpy.uint32), numpy.full((_Q, 257), -7.5, numpy.float32)
    before = idx.tobytes(), dist.tobytes()
    rc = _lib().kmamd_pq_search(a["q"], a["n"], a["width"], a["m"], a["dsub"], a["ksub"], a["k"], a["metric"],
                                a["fp16"], a["device"], a["device_ptrs"], 0, queries.ctypes.data, books.ctypes.data,
                                codes.ctypes.data, idx.ctypes.data, dist.ctypes.data)
    assert rc == 1, what   # kmcudaInvalidArguments
    assert (idx.tobytes(), dist.tobytes()) == before, what


_QUERIES = numpy.zeros((_Q, _M * _DSUB), numpy.float32)
_BOOKS = numpy.zeros((_M, _KSUB, _DSUB), numpy.float32)
_CODES = numpy.zeros((_N, _M), numpy.uint8)
PY_TABLE = [
    ("M = 65", dict(queries=numpy.zeros((_Q, 65), numpy.float32), codebooks=numpy.zeros((65, 2, 1), numpy.float32),
                    codes=numpy.zeros((_N, 65), numpy.uint8)), ValueError),
    ("dsub = 65", dict(queries=numpy.zeros((_Q, 65), numpy.float32), codebooks=numpy.zeros((1, 2, 65), numpy.float32),
                       codes=_CODES[:, :1]), ValueError),
    ("ksub = 257", dict(codebooks=numpy.zeros((_M, 257, _DSUB), numpy.float32)), ValueError),
    ("ksub = 0", dict(codebooks=_BOOKS[:, :0]), ValueError),
    ("N = 0", dict(codes=_CODES[:0]), ValueError),
    ("k = 0", dict(k=0), ValueError),
    ("k > N", dict(codes=_CODES[:4]), ValueError),
    ("k = 257", dict(codes=numpy.zeros((300, _M), numpy.uint8), k=257), ValueError),
    ("k = 2.0", dict(k=2.0), TypeError),
    ("query width", dict(queries=_QUERIES[:, :-1]), ValueError),
    ("codes of another M", dict(codes=_CODES[:, :3]), ValueError),
    ("codebooks of rank 2", dict(codebooks=_BOOKS[0]), ValueError),
    ("fp16", dict(queries=_QUERIES.astype(numpy.float16)), ValueError),
    ("float64", dict(codebooks=_BOOKS.astype(numpy.float64)), TypeError),
    ("int32 codes", dict(codes=_CODES.astype(numpy.int32)), TypeError),
    ("angular", dict(metric="cos"), ValueError),
    ("device = -1", dict(device=-1), ValueError),
]


@pytest.mark.parametrize("what,over,exc", PY_TABLE, ids=[row[0] for row in PY_TABLE])
def test_python_raises_before_the_library(monkeypatch, what, over, exc):
    from kmcuda_amd import _lib

    def no_library():
        raise AssertionError("the library was asked")
    monkeypatch.setattr(_lib, "lib", no_library)
    kw = dict(queries=_QUERIES, codebooks=_BOOKS, codes=_CODES, k=_K)
    kw.update(over)
    with pytest.raises(exc):
        pq_search(kw.pop("queries"), kw.pop("codebooks"), kw.pop("codes"), kw.pop("k"), **kw)


def test_no_queries_no_device():
    idx, dist = pq_search(_QUERIES[:0], _BOOKS, _CODES, _K)
    assert idx.shape == dist.shape == (0, _K) and idx.dtype == numpy.uint32 and dist.dtype == numpy.float32
    assert _lib().kmamd_pq_search(0, _N, _M * _DSUB, _M, _DSUB, _KSUB, _K, 0, 0, 0, -1, 0, None, _BOOKS.ctypes.data,
                                  _CODES.ctypes.data, None, None) == 0


def test_query_tile_mirror():
    L = _lib()
    for k in (0, 1, 10, 32, 33, 100, 128, 129, 256, 257):
        for m in range(0, 67):
            assert pq.query_tile(m, k) == L.kmamd_pq_query_tile(m, k), (m, k)
    assert [pq.query_tile(m, 10) for m in (1, 4, 5, 8, 16, 32, 39, 40, 64)] == [16, 16, 8, 8, 4, 4, 4, 2, 2]
    assert [pq.query_tile(m, 256) for m in (4, 8, 35, 36, 64)] == [8, 4, 4, 2, 2]
