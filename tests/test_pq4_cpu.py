"""4-bit product-quantiser codes on a machine without a device: pq_pack4, the refusals -- the C ABI
answers InvalidArguments, where any answer behind a device call would be NoSuchDevice here, and the Python calls raise
ValueError before the library is asked for anything -- and the query-tile rules against their C mirrors."""
import numpy
import pytest
import torch

from kmcuda_amd import IvfPqIndex, ivfpq, ivfpq_search, pq, pq_pack4, pq_search


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from kmcuda_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("m", [1, 4, 7])
def test_pack4(m):
    codes = numpy.random.RandomState(m).randint(0, 16, (50, m)).astype(numpy.uint8)
    want = numpy.zeros((50, (m + 1) // 2), numpy.uint8)
    for col in range(m):
        want[:, col // 2] |= codes[:, col] << (4 * (col % 2))
    assert pq_pack4(codes).tobytes() == want.tobytes() and pq_pack4(codes).shape == want.shape
    assert pq_pack4(torch.from_numpy(codes)).numpy().tobytes() == want.tobytes()
    codes[3, m - 1] = 16
    with pytest.raises(ValueError):
        pq_pack4(codes)


@pytest.mark.parametrize("m,ksub", [(129, 16), (4, 17)])
def test_c_abi_refuses(m, ksub):
    L, f, i = _lib(), numpy.zeros(129 * 17, numpy.float32), numpy.zeros(200, numpy.uint32)
    idx, dist = numpy.full(10, 0x5A5A5A5A, numpy.uint32), numpy.full(10, -7.5, numpy.float32)
    p = [a.ctypes.data for a in (f, i, idx, dist)]
    assert L.kmamd_pq4_search(1, 100, m, m, 1, ksub, 5, 0, 0, 0, -1, 0, p[0], p[0], p[1], p[2], p[3]) == 1
    assert L.kmamd_ivfpq4_search(1, 100, m, 8, m, 1, ksub, 5, 2, 0, 0, 0, -1, 0, p[0], p[0], p[0], p[1], p[1], p[1],
                                 p[1], p[2], p[3]) == 1      # kmcudaInvalidArguments
    assert (idx == 0x5A5A5A5A).all() and (dist == -7.5).all()


def _flat(m=4, ksub=16, width=None, **kw):
    width = (m + 1) // 2 if width is None else width
    return lambda: pq_search(numpy.zeros((3, m), numpy.float32), numpy.zeros((m, ksub, 1), numpy.float32),
                             numpy.zeros((100, width), numpy.uint8), 5, **dict(dict(bits=4), **kw))


def _ivf(m=4, ksub=16, width=None, **kw):
    width = (m + 1) // 2 if width is None else width
    return lambda: ivfpq_search(numpy.zeros((3, m), numpy.float32), numpy.zeros((8, m), numpy.float32),
                                numpy.zeros((m, ksub, 1), numpy.float32), numpy.zeros((100, width), numpy.uint8),
                                numpy.arange(100, dtype=numpy.uint32), numpy.zeros(9, numpy.uint32),
                                numpy.zeros((3, 2), numpy.uint32), 5, **dict(dict(bits=4), **kw))


def _index(**kw):
    return lambda: IvfPqIndex(numpy.zeros((50, 4), numpy.float32), numpy.zeros((8, 4), numpy.float32),
                              numpy.zeros((4, 16, 1), numpy.float32), assignments=numpy.zeros(50, numpy.uint32), **kw)


REFUSED = {
    "flat M = 129": _flat(m=129), "flat ksub = 17": _flat(ksub=17), "flat one column per sub-space": _flat(width=4),
    "flat odd M, a column short": _flat(m=5, width=2), "flat bits = 5": _flat(bits=5), "flat bits = 1": _flat(bits=True),
    "ivf M = 129": _ivf(m=129), "ivf ksub = 17": _ivf(ksub=17), "ivf one column per sub-space": _ivf(width=4),
    "ivf bits = 2": _ivf(bits=2), "ivf terms": _ivf(terms=numpy.zeros((8, 4, 16), numpy.float32)),
    "index precomputed": _index(bits=4, precomputed=True), "index bits = 16": _index(bits=16),
    "query_tile bits = 6": lambda: pq.query_tile(4, 10, bits=6),
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
        for m in range(0, 131):
            assert pq.query_tile(m, k, bits=4) == L.kmamd_pq4_query_tile(m, k), (m, k)
            assert ivfpq.query_tile(m, k, bits=4) == L.kmamd_ivfpq4_query_tile(m, k), (m, k)
        for m in (1, 8, 33, 64, 65):
            assert pq.query_tile(m, k) == pq.query_tile(m, k, bits=8) == L.kmamd_pq_query_tile(m, k)
            assert ivfpq.query_tile(m, k) == ivfpq.query_tile(m, k, bits=8) == L.kmamd_ivfpq_query_tile(m, k)
    # 16 at every M <= 64 for small k, never below 4, nothing beyond the limits
    assert [pq.query_tile(m, 10, bits=4) for m in (1, 32, 64, 65, 71, 72, 128, 129)] == [16, 16, 16, 16, 16, 8, 8, 0]
    assert [pq.query_tile(m, 256, bits=4) for m in (1, 15, 16, 95, 96, 128)] == [16, 16, 8, 8, 4, 4]
