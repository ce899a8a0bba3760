"""The CPU oracle's k-NN on rows without a cluster (assignment >= K, what kmeans_cuda gives NaN samples): such a row
gets an all-UINT32_MAX list, is never a candidate, and adds nothing to dists_calced -- the product's definition
(knn_job.cpp, KnnJob::gather_outputs; knn.hip, knn_exact_kernel).  Every other row's list is the one of the same search
with those rows removed."""
import numpy
import pytest

import oracle


def _corpus(seed, n, d, K):
    rs = numpy.random.RandomState(seed)
    x = rs.rand(n, d).astype(numpy.float32)
    x[: n // 2, 0] += 2.0
    c = x[rs.choice(n, K, replace=False)].copy()
    a, _, _ = oracle.lloyd_assign(x, c)
    return rs, x, c, a


@pytest.mark.parametrize("n,d,K,k", [(1500, 12, 20, 7), (300, 5, 6, 40), (60, 3, 4, 70)])
def test_rows_without_cluster_get_no_neighbours(n, d, K, k):
    rs, x, c, a = _corpus(n + k, n, d, K)
    ref, ref_calced = oracle.knn(k, x, c, a)
    # NaN rows at scattered positions (never position 0: a slot the heap never fills holds index 0), assignment K
    # and 0xFFFFFFFF
    m = 9
    nan_at = numpy.sort(1 + rs.choice(n + m - 1, m, replace=False))
    keep = numpy.ones(n + m, bool)
    keep[nan_at] = False
    xx = numpy.empty((n + m, d), numpy.float32)
    xx[keep] = x
    xx[nan_at] = numpy.nan
    aa = numpy.empty(n + m, numpy.uint32)
    aa[keep] = a
    aa[nan_at] = numpy.where(numpy.arange(m) % 2 == 0, K, 0xFFFFFFFF).astype(numpy.uint32)
    nb, calced = oracle.knn(k, xx, c, aa)
    assert (nb[nan_at] == 0xFFFFFFFF).all()
    old_index = numpy.nonzero(keep)[0]           # index in the corpus with NaN rows of row i of the plain one
    assert old_index[0] == 0
    assert (nb[keep] == old_index[ref]).all()
    assert calced == ref_calced
    if k >= n:
        assert (ref[:, n - 1:] == 0).all()       # the filler slots really are exercised
