"""Non-residual IVF-PQ lists without a device: the C ABI's and Python's refusals, which come before
any device or library call, and the pair-tile rule."""
import numpy
import pytest

from kmcuda_amd import IvfPqIndex, ivfpq, ivfpq_search, ivfpq_train, pq


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from kmcuda_amd import _lib
    return _lib.lib()


# (M, ksub, k, nprobe, a null pointer); K = 8
@pytest.mark.parametrize("m,ksub,k,nprobe,null", [(65, 256, 5, 2, None), (0, 256, 5, 2, None), (4, 257, 5, 2, None),
                                                  (4, 256, 0, 2, None), (4, 256, 257, 2, None), (4, 256, 5, 0, None),
                                                  (4, 256, 5, 9, None)] + [(4, 256, 5, 2, at) for at in range(9)])
@pytest.mark.parametrize("name", ["kmamd_ivfpq_search_nonresidual", "kmamd_ivfpq_search_nonresidual_f16"])
def test_c_abi_refuses(name, m, ksub, k, nprobe, null):
    f, i = numpy.zeros(65 * 257, numpy.float32), numpy.zeros(200, numpy.uint32)
    idx, dist = numpy.full(300, 0x5A5A5A5A, numpy.uint32), numpy.full(300, -7.5, numpy.float32)
    # queries, centroids, codebooks, codes, ids, offsets, probes, indices, distances
    p = [a.ctypes.data for a in (f, f, f, i, i, i, i, idx, dist)]
    if null is not None:
        p[null] = None
    assert getattr(_lib(), name)(1, 100, m, 8, m, 1, ksub, k, nprobe, 0, 0, 0, -1, 0, *p) == 1   # InvalidArguments
    assert (idx == 0x5A5A5A5A).all() and (dist == -7.5).all()


def _z(*shape, t=numpy.float32):
    return numpy.zeros(shape, t)


def _ivf(**kw):
    codes, u = _z(100, 2 if kw.get("bits") == 4 else 4, t=numpy.uint8), numpy.uint32
    return lambda: ivfpq_search(_z(3, 4), _z(8, 4), _z(4, 16, 1), codes, _z(100, t=u), _z(9, t=u), _z(3, 2, t=u), 5,
                                **kw)


def _index(**kw):
    return lambda: IvfPqIndex(_z(50, 4), _z(8, 4), _z(4, 16, 1), assignments=_z(50, t=numpy.uint32), **kw)


REFUSED = {
    "search 0": _ivf(residual=0), "search None": _ivf(residual=None), "search a string": _ivf(residual="no"),
    "search terms": _ivf(residual=False, terms=_z(8, 4, 16)), "search bits = 4": _ivf(residual=False, bits=4),
    "index 1": _index(residual=1), "index precomputed": _index(residual=False, precomputed=True),
    "index bits = 4": _index(residual=False, bits=4),
    "train 0": lambda: ivfpq_train(_z(50, 4), _z(8, 4), 4, 16, _z(50, t=numpy.uint32), residual=0),
    "query_tile None": lambda: ivfpq.query_tile(4, 10, residual=None),
    "query_tile bits = 4": lambda: ivfpq.query_tile(4, 10, bits=4, residual=False),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_python_raises_before_the_library(monkeypatch, what):
    from kmcuda_amd import _lib
    monkeypatch.setattr(_lib, "lib", None)          # asking the library would be a TypeError
    with pytest.raises(ValueError):
        REFUSED[what]()


def test_pair_tile_is_pq_search_tile():
    for table_dtype in ("float32", "float16"):
        for k in range(0, 258):
            for m in range(0, 67):
                assert ivfpq.query_tile(m, k, table_dtype=table_dtype, residual=False) == \
                    pq.query_tile(m, k, table_dtype=table_dtype), (m, k)
    assert [ivfpq.query_tile(m, 10, residual=False) for m in (4, 8, 32, 64)] == [16, 8, 4, 2]
    assert ivfpq.query_tile(8, 10) == ivfpq.query_tile(8, 10, residual=True)
