"""Exactly summable inputs for the weighted centroid update (tests/test_gpu_weighted_update.py, test_gpu_sharded.py,
test_weighted_cpu.py).

Rows are m / 1024 with integer m in [0, 1024); weights are j * 2^e with integer j in [1, 15] and e in [-6, 6] (about
four decades, exact in float32).  Every product w * x is then a multiple of 2^-16 below 2^10, so any sum over at most
2^16 rows is a multiple of 2^-16 below 2^26 -- 42 bits -- and any sum of weights a multiple of 2^-6 below 2^26: every
partial sum is exact in fp64 in any order and any grouping.  A float64 numpy sum and a kernel's fp64 sum of the same
rows agree bit for bit, and a wrong row, a wrong weight, a dropped or a doubled row changes the result."""
import numpy

MAX_ROWS = 1 << 16   # the argument above holds up to here


def exact_rows(rs, n, d):
    assert n <= MAX_ROWS
    return (rs.randint(0, 1024, size=(n, d)) / 1024.0).astype(numpy.float32)


def exact_weights(rs, n):
    """j * 2^e, j in [1, 15], e in [-6, 6]: drawn per row, so the weight of a row says nothing about its neighbours'."""
    assert n <= MAX_ROWS
    return (rs.randint(1, 16, size=n) * 2.0 ** rs.randint(-6, 7, size=n)).astype(numpy.float32)


def index_weights(n):
    """w[i] = 2^((i % 13) - 6): a function of the row INDEX with period 13 -- read at a list position instead of at
    the row the list names, it gives another weight unless the two differ by a multiple of 13."""
    assert n <= MAX_ROWS
    return (2.0 ** ((numpy.arange(n) % 13) - 6)).astype(numpy.float32)


def cluster_sums(x, w, labels, k, order=None):
    """Per cluster (labels in [0, k); anything else belongs to none): float64 sums of w * x and of w, the rows taken
    in `order` (a permutation of the row indices) one after the other."""
    n, d = x.shape
    sx = numpy.zeros((k, d), numpy.float64)
    sw = numpy.zeros(k, numpy.float64)
    order = numpy.arange(n) if order is None else order
    lab = labels[order]
    keep = (lab >= 0) & (lab < k)
    rows, lab = order[keep], lab[keep]
    w64 = w[rows].astype(numpy.float64)
    numpy.add.at(sx, lab, w64[:, None] * x[rows].astype(numpy.float64))   # unbuffered: strictly in `order`
    numpy.add.at(sw, lab, w64)
    return sx, sw
