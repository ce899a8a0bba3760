"""fp16 lookup tables without a device: the C ABI's and Python's refusals, which come before any
device or library call, and the query-tile rule against its C mirrors."""
import numpy
import pytest

from kmcuda_amd import IvfPqIndex, ivfpq, ivfpq_search, pq, pq_search


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from kmcuda_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("m,ksub", [(65, 256), (4, 257)])
def test_c_abi_refuses(m, ksub):
    L, f, i = _lib(), numpy.zeros(65 * 257, numpy.float32), numpy.zeros(200, numpy.uint32)
    idx, dist = numpy.full(10, 0x5A5A5A5A, numpy.uint32), numpy.full(10, -7.5, numpy.float32)
    p = [a.ctypes.data for a in (f, i, idx, dist)]
    assert L.kmamd_pq_search_f16(1, 100, m, m, 1, ksub, 5, 0, 0, 0, -1, 0, p[0], p[0], p[1], p[2], p[3]) == 1
    assert L.kmamd_ivfpq_search_f16(1, 100, m, 8, m, 1, ksub, 5, 2, 0, 0, 0, -1, 0, p[0], p[0], p[0], p[1], p[1], p[1],
                                    p[1], p[2], p[3]) == 1      # kmcudaInvalidArguments
    assert (idx == 0x5A5A5A5A).all() and (dist == -7.5).all()


def _z(*shape, t=numpy.float32):
    return numpy.zeros(shape, t)


def _flat(**kw):
    codes = _z(100, 2 if kw.get("bits") == 4 else 4, t=numpy.uint8)
    return lambda: pq_search(_z(3, 4), _z(4, 16, 1), codes, 5, **kw)


def _ivf(**kw):
    codes, u = _z(100, 2 if kw.get("bits") == 4 else 4, t=numpy.uint8), numpy.uint32
    return lambda: ivfpq_search(_z(3, 4), _z(8, 4), _z(4, 16, 1), codes, _z(100, t=u), _z(9, t=u), _z(3, 2, t=u), 5,
                                **kw)


def _index(**kw):
    return lambda: IvfPqIndex(_z(50, 4), _z(8, 4), _z(4, 16, 1), assignments=_z(50, t=numpy.uint32), **kw)


REFUSED = {
    "flat bfloat16": _flat(table_dtype="bfloat16"), "flat a numpy dtype": _flat(table_dtype=numpy.float16),
    "flat bits = 4": _flat(table_dtype="float16", bits=4),
    "ivf float64": _ivf(table_dtype="float64"), "ivf bits = 4": _ivf(table_dtype="float16", bits=4),
    "ivf terms": _ivf(table_dtype="float16", terms=_z(8, 4, 16)),
    "index half": _index(table_dtype="half"), "index bits = 4": _index(table_dtype="float16", bits=4),
    "index precomputed": _index(table_dtype="float16", precomputed=True),
    "pq.query_tile fp16": lambda: pq.query_tile(4, 10, table_dtype="fp16"),
    "pq.query_tile bits = 4": lambda: pq.query_tile(4, 10, bits=4, table_dtype="float16"),
    "ivfpq.query_tile None": lambda: ivfpq.query_tile(4, 10, table_dtype=None),
    "ivfpq.query_tile bits = 4": lambda: ivfpq.query_tile(4, 10, bits=4, table_dtype="float16"),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_python_raises_before_the_library(monkeypatch, what):
    from kmcuda_amd import _lib
    monkeypatch.setattr(_lib, "lib", None)          # asking the library would be a TypeError
    with pytest.raises(ValueError):
        REFUSED[what]()


def test_query_tile_mirrors_and_defaults():
    L = _lib()
    for k in range(0, 258):
        for m in range(0, 67):
            want = pq.query_tile(m, k, table_dtype="float16")
            assert want == L.kmamd_pq_f16_query_tile(m, k) == L.kmamd_ivfpq_f16_query_tile(m, k), (m, k)
            assert want == ivfpq.query_tile(m, k, table_dtype="float16"), (m, k)
            assert pq.query_tile(m, k) == pq.query_tile(m, k, table_dtype="float32") == L.kmamd_pq_query_tile(m, k)
            assert ivfpq.query_tile(m, k, table_dtype="float32") == L.kmamd_ivfpq_query_tile(m, k)
    # k <= 32: 16 up to M = 8, 8 up to 18, 4 beyond -- two blocks per CU up to M = 38 --, nothing past the limits
    ms = (1, 8, 9, 18, 19, 38, 39, 64, 65)
    assert [pq.query_tile(m, 10, table_dtype="float16") for m in ms] == [16, 16, 8, 8, 4, 4, 4, 4, 0]
    assert [pq.query_tile(m, 32, table_dtype="float16") for m in ms] == [16, 16, 8, 8, 4, 4, 4, 4, 0]
    assert [pq.query_tile(m, 256, table_dtype="float16") for m in (1, 2, 3, 11, 12, 64)] == [16, 8, 8, 8, 4, 4]
    assert pq._scan_lds_bytes(38, 32, 4, 256, 2) <= 80 << 10 < pq._scan_lds_bytes(39, 32, 4, 256, 2)
    assert pq._scan_lds_bytes(64, 256, 4, 256, 2) == 147536 <= 160 << 10
    assert [pq.query_tile(32, 10), ivfpq.query_tile(32, 10)] == [4, 4]      # the fp32 tiles of the README width
