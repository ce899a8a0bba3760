"""The multi-probe search of the k-NN index in executable form, and the one helper that holds the
index to it.

A probed list is what the procedure of 4.8 point 2 yields when a cluster outside the query's effective probe set is
never visited.  With the oracle as it is, that is oracle.knn_query on the corpus whose rows outside the set have lost
their cluster (assignment 0xFFFFFFFF), the query being a row of cluster P(q)[0]: a cluster without rows is walked over
without a push, and the prune test reads only radii and centroid distances of clusters that are visited."""
import numpy

import oracle
from _angular import assert_knn_only_acos_matters

NONE = 0xFFFFFFFF
FLT_MAX = numpy.finfo(numpy.float32).max
EXACT = "every candidate is evaluated with the exact arithmetic"
QUERY_HALF_RANGE = "k-NN query: a centred query leaves the half range"
INDEX_HALF_RANGE = "k-NN index: a centred row leaves the half range"


def _bits(d):
    """float32 bit patterns, every NaN mapped to one pattern."""
    d = numpy.ascontiguousarray(d, dtype=numpy.float32)
    return numpy.where(numpy.isnan(d), numpy.uint32(0x7FC00000), d.view(numpy.uint32))


def effective_set(row, K):
    """The distinct entries of a probe list that are below K, as a sorted tuple."""
    return tuple(sorted(set(int(v) for v in row if v < K)))


def probe_reference(k, x, c, a, q, probes, metric="L2", half2=False):
    """(neighbors, distances) of the probed search on the CPU oracle.  probes: Q x p, column 0 the own cluster, K a
    filler.  A query whose column 0 is K (no cluster) gets 0xFFFFFFFF / NaN, as does one with a non-finite feature
    (oracle.knn_query's own rule).  One oracle call per group of queries with the same (column 0, effective set)."""
    a = numpy.ascontiguousarray(a, dtype=numpy.uint32)
    probes = numpy.asarray(probes).astype(numpy.int64)
    K, Q = len(c), len(q)
    nb = numpy.full((Q, k), NONE, numpy.uint32)
    dist = numpy.full((Q, k), numpy.nan, numpy.float32)
    groups = {}
    for i in range(Q):
        if probes[i, 0] >= K:
            continue
        groups.setdefault((int(probes[i, 0]), effective_set(probes[i], K)), []).append(i)
    for (c_q, members), rows in groups.items():
        rows = numpy.asarray(rows)
        masked = numpy.where(numpy.isin(a, members), a, NONE).astype(numpy.uint32)
        qa = numpy.full(len(rows), c_q, numpy.uint32)
        g_nb, g_dist = oracle.knn_query(k, x, c, masked, numpy.ascontiguousarray(q[rows]), query_assignments=qa,
                                        metric=metric, half2=half2)
        nb[rows], dist[rows] = g_nb, g_dist
    return nb, dist


def run_probe(k, x, c, a, q, metric="L2", ptr="host", nprobe=None, probes=None, verbosity=1, index=None):
    """One KnnIndex build (unless `index` is given) + probed query; (neighbors, distances, probes used) as numpy arrays
    (uint32 views of the device's int32) and what the library printed."""
    import torch
    from kmcuda_amd import KnnIndex
    from test_gpu_kmeans import StdoutListener
    out = StdoutListener()
    with out:
        if ptr == "host":
            ix = index or KnnIndex(x, c, a, metric=metric, verbosity=verbosity)
            try:
                res = ix.query(q, k, nprobe=nprobe, probes=probes, return_probes=True)
            finally:
                if index is None:
                    ix.close()
        else:
            dev = torch.device("cuda", 0)
            tx, tc, tq = (torch.from_numpy(v).to(dev) for v in (x, c, q))
            ta = torch.from_numpy(numpy.ascontiguousarray(a, dtype=numpy.uint32).view(numpy.int32)).to(dev)
            tp = None if probes is None else torch.from_numpy(
                numpy.ascontiguousarray(probes, dtype=numpy.uint32).view(numpy.int32)).to(dev)
            ix = index or KnnIndex(tx, tc, ta, metric=metric, verbosity=verbosity)
            try:
                res = ix.query(tq, k, nprobe=nprobe, probes=tp, return_probes=True)
            finally:
                if index is None:
                    ix.close()
            res = tuple(r.cpu().numpy().view(numpy.uint32) if r.dtype == torch.int32 else r.cpu().numpy() for r in res)
    return res, out.text


def check_probe(k, x, c, a, q, nprobe=None, probes=None, metric="L2", env=None, ptr="host", expect=None,
                monkeypatch=None, half2=False):
    """KnnIndex(x, c, a).query(q, k, nprobe / probes) == probe_reference on the lists the index says it used.
    L2 and the half2 arithmetic: neighbours and distance bit patterns equal the reference's, NaN rows and FLT_MAX
    fillers included.  Angular: the allowance of tests/_angular.py and nothing wider.  expect: "f16" or "exact" -- the
    search that must have run, read from what verbosity 1 prints.  Returns (neighbors, distances, probes used, text)."""
    for key, v in (env or {}).items():
        monkeypatch.setenv(key, str(v))
    a = numpy.ascontiguousarray(a, dtype=numpy.uint32)
    q = numpy.ascontiguousarray(q)
    assert x.dtype == c.dtype == q.dtype
    (nb, dist, used), text = run_probe(k, x, c, a, q, metric, ptr, nprobe, probes)
    K = len(c)
    what = "%s D=%d K=%d k=%d p=%s %s %s" % (metric, x.shape[1], K, k, nprobe if probes is None else "given", ptr, env)
    if probes is not None:
        assert (used == numpy.asarray(probes).astype(numpy.uint32)).all(), what
    x32, c32, q32 = x.astype(numpy.float32), c.astype(numpy.float32), q.astype(numpy.float32)
    finite = numpy.isfinite(q32).all(axis=1)
    ref_nb, ref_dist = probe_reference(k, x if half2 else x32, c if half2 else c32, a, q if half2 else q32, used,
                                       metric=metric, half2=half2)
    assert (nb[~finite] == NONE).all() and numpy.isnan(dist[~finite]).all(), what
    if metric == "L2":
        bad = numpy.nonzero((nb != ref_nb).any(axis=1))[0]
        assert bad.size == 0, "%s: %d lists differ from the reference, first %d: %s vs %s (probes %s)" % (
            what, bad.size, bad[0], nb[bad[0]], ref_nb[bad[0]], used[bad[0]])
        bad = numpy.nonzero((_bits(dist) != _bits(ref_dist)).any(axis=1))[0]
        assert bad.size == 0, "%s: %d distance rows differ from the reference, first %d: %s vs %s" % (
            what, bad.size, bad[0], dist[bad[0]], ref_dist[bad[0]])
    else:
        has = ~numpy.isnan(ref_dist).all(axis=1)
        assert (nb[~has] == NONE).all() and numpy.isnan(dist[~has]).all(), what
        allowed = assert_knn_only_acos_matters(x32, nb[has], ref_nb[has], what, queries=q32[has])
        print("angular allowance: %d of %d rows (%s)" % (allowed, len(q), what))
        filler = ref_dist == FLT_MAX
        assert (filler == (dist == FLT_MAX)).all() and (nb[filler] == 0).all(), what
        assert (numpy.isnan(dist) == numpy.isnan(ref_dist)).all(), what
        for i, j in zip(*numpy.nonzero(~filler & ~numpy.isnan(ref_dist))):
            want = numpy.float32(oracle.distance(q32[i], x32[nb[i, j]], metric=oracle.COS))
            assert abs(dist[i, j] - want) <= 2 * numpy.spacing(max(dist[i, j], want)), (what, i, j, dist[i, j], want)
    # every neighbour is a row of a probed cluster
    for i in numpy.nonzero(finite & (used[:, 0] < K))[0][:200]:
        real = dist[i] < FLT_MAX
        assert numpy.isin(a[nb[i][real]], effective_set(used[i], K)).all(), (what, int(i))
    if expect is not None:
        assert expect in ("f16", "exact")
        assert (EXACT in text) == (expect == "exact"), text
    return nb, dist, used, text
