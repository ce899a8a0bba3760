"""Mini-batch K-means restated in numpy (include/kmcuda_amd.h: kmamd_minibatch_*), on the CPU oracle's
assignment pass, with the hash draw in Python integers, and the fixtures tests/test_minibatch_cpu.py and
tests/test_gpu_minibatch.py share.

The "grid" fixtures hold rows randint(-128, 128) / 32 with integer weights in [1, 8], fewer than 2^16 rows over all
steps: every S_c, n_c and C W is then exact in fp64, so a step's result does not depend on the order of its sums.
step(..., exact=True) ASSERTS that -- math.fsum equals the forward and the reverse sum, for every cluster and feature
-- and only such steps are compared bit for bit with the device.  On other data the sums are math.fsum's (correctly
rounded) and step() also returns what the tests' error bounds need.
"""
import functools
import math

import numpy

import oracle

from _seed_parallel_ref import hash64


def draw(seed, t, batch, n):
    """The corpus rows of the batch of the step with counter t: floor(h(seed, t, j) * n / 2^64) for every slot j."""
    return numpy.array([(hash64(seed, t & 0xFFFFFFFF, j) * n) >> 64 for j in range(batch)], numpy.int64)


def _metric_id(metric):
    return oracle.COS if metric in ("angular", "cos", "cosine") else oracle.L2


def assign(x32, c32, metric):
    """kmeans_predict(x, c): one pass from "no cluster" (K)."""
    k = len(c32)
    if len(x32) == 0:
        return numpy.zeros(0, numpy.uint32)
    a, _, _ = oracle.lloyd_assign(x32, c32, assignments=numpy.full(len(x32), k, numpy.uint32),
                                  metric=_metric_id(metric))
    return a


def _column_sums(terms, exact):
    """The sum of every column of `terms` (m x D float64): math.fsum's.  exact: the forward and the reverse sum must
    equal it."""
    s = numpy.array([math.fsum(col) for col in terms.T.tolist()], numpy.float64)
    if exact:
        fwd = numpy.cumsum(terms, axis=0)[-1]
        rev = numpy.cumsum(terms[::-1], axis=0)[-1]
        assert (fwd == s).all() and (rev == s).all(), "the fixture's sums depend on their order"
    return s


def step(c, w, x, sample_weight=None, metric="L2", exact=False):
    """One step of the contract.  c: K x D float32, w: K float64, x: n x D (float32 or float16).  Returns a dict:
    centroids, weights, assignments, and per visited cluster (lists in ascending cluster order) members, abs_sums
    (sum of |w x| per feature), v (C W + S) and norm."""
    c = numpy.array(c, numpy.float32)
    w = numpy.array(w, numpy.float64)
    x32 = numpy.ascontiguousarray(x, dtype=numpy.float32)   # halves widen exactly
    k = len(c)
    a = assign(x32, c, metric)
    sw = (numpy.ones(len(x32)) if sample_weight is None else numpy.asarray(sample_weight)).astype(numpy.float64)
    out = dict(assignments=a, clusters=[], members=[], abs_sums=[], v=[], norm=[])
    angular = _metric_id(metric) == oracle.COS
    for cl in numpy.unique(a[a < k]):
        members = numpy.nonzero(a == cl)[0]   # ascending batch position
        terms = sw[members, None] * x32[members].astype(numpy.float64)   # 24 x 24 bits: exact products
        n_c = _column_sums(sw[members, None], exact)[0]
        s_c = _column_sums(terms, exact)
        cw = c[cl].astype(numpy.float64) * w[cl]
        if exact:   # C W fits: the quotient's 24 bits times a weight below 2^20
            assert w[cl] == int(w[cl]) and w[cl] < 2 ** 20
        v = cw + s_c
        w_new = w[cl] + n_c
        if angular:
            norm = math.sqrt(math.fsum((v * v).tolist()))
            new = v / norm
        else:
            norm = None
            new = v / w_new
        c[cl] = new.astype(numpy.float32)
        w[cl] = w_new
        out["clusters"].append(int(cl))
        out["members"].append(members)
        out["abs_sums"].append(numpy.abs(terms).sum(axis=0))
        out["v"].append(v)
        out["norm"].append(norm)
    out.update(centroids=c, weights=w)
    return out


def run(c, w, batches, weights=None, metric="L2", exact=False):
    """Consecutive steps; returns the list of step() results."""
    res = []
    for i, x in enumerate(batches):
        r = step(c, w, x, None if weights is None else weights[i], metric, exact)
        c, w = r["centroids"], r["weights"]
        res.append(r)
    return res


# ----------------------------------------------------------------------------------------------------------------------
# fixtures
# ----------------------------------------------------------------------------------------------------------------------
STEPS = 3


def grid_rows(rs, n, d):
    return (rs.randint(-128, 128, size=(n, d)) / 32.0).astype(numpy.float32)


@functools.lru_cache(maxsize=None)
def grid(n, d, k, weighted):
    """(centroids K x D, [STEPS batches of n x D], [STEPS weight vectors] or None); read-only arrays.  The seeds are
    grid rows too."""
    assert STEPS * n * 8 < 2 ** 20 and STEPS * n < 2 ** 16
    rs = numpy.random.RandomState(1000 * n + 10 * d + k)
    c = grid_rows(rs, k, d)
    batches = [grid_rows(rs, n, d) for _ in range(STEPS)]
    weights = [rs.randint(1, 9, size=n).astype(numpy.float32) for _ in range(STEPS)] if weighted else None
    for arr in [c] + batches + (weights or []):
        arr.setflags(write=False)
    return c, batches, weights


@functools.lru_cache(maxsize=None)
def grid_restated(n, d, k, weighted):
    """The restatement of the STEPS steps of grid(...) from cluster weights 0, with the exactness assertion."""
    c, batches, weights = grid(n, d, k, weighted)
    return run(c, numpy.zeros(k), batches, weights, "L2", exact=True)


# (n, D, K) of "three steps against the restatement": the scalar and the 16-byte row mapping, lists below and above
# 128 rows, the streamed filter (D = 320), K no multiple of 32, a one-row batch
GRID_SHAPES = [(1, 32, 2), (255, 30, 16), (257, 1, 2), (5003, 32, 16), (5003, 30, 100), (257, 256, 100),
               (5003, 320, 16)]
