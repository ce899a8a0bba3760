"""Inputs and ground truth of the radius-search tests (tests/test_gpu_knn_radius.py, tests/test_radius_bound_model.py).

The corpus is the Gaussian mixture under an oracle k-means of tests/test_gpu_knn_query.py (rebuilt here; at N = 2000,
K = 16, seed 0 it leaves empty clusters and, in one case, a NaN centroid -- wanted).  The truth is the oracle's:
oracle.knn_query(k = N) returns, for every query, the exact distance to every clustered corpus row; a query's expected
hits are the rows with distance <= r in ascending (cluster id, row index) order.  Everything is computed once per
key."""
import numpy

import oracle

FLT_MAX = numpy.float32(3.402823466e+38)


def mixture(n, d, centres=12, seed=0, spread=10.0):
    rng = numpy.random.default_rng(seed)
    mu = rng.uniform(0, spread, (centres, d)).astype(numpy.float32)
    lab = rng.integers(0, centres, n)
    return (mu[lab] + rng.standard_normal((n, d)).astype(numpy.float32)).astype(numpy.float32), mu


def unit(x):
    return (x / numpy.linalg.norm(x, axis=1, keepdims=True)).astype(numpy.float32)


_CORPUS, _QUERIES, _DIST = {}, {}, {}


def clustered(n, d, metric="L2", half=False, clusters=16, seed=0):
    """(samples, centroids, assignments), read-only."""
    key = (n, d, metric, half, clusters, seed)
    if key not in _CORPUS:
        x, _ = mixture(n, d, seed=seed)
        if metric != "L2":
            x = unit(x - x.mean(axis=0))
        if half:
            x = x.astype(numpy.float16)
        c, a, _ = oracle.kmeans(x, clusters, seed=seed, metric=metric, init="random")
        for v in (x, c, a):
            v.setflags(write=False)
        _CORPUS[key] = (x, c, a)
    return _CORPUS[key]


def fresh_queries(q, n, d, metric="L2", half=False, seed=0):
    """q rows near the corpus of clustered(n, d, metric, half): corpus rows plus noise, some exact copies."""
    key = (q, n, d, metric, half, seed)
    if key not in _QUERIES:
        x = clustered(n, d, metric, half, seed=seed)[0].astype(numpy.float32)
        rng = numpy.random.default_rng(100 + seed)
        rows = x[rng.choice(len(x), q)]
        noise = rng.standard_normal((q, d)).astype(numpy.float32)
        out = rows + (0.7 if metric == "L2" else 0.03) * noise
        out[::17] = rows[::17]
        # a few rows far from every corpus row: no hits at the radii of the tests
        far = rng.uniform(-60, 80, (5, d)) if metric == "L2" else -x.mean(axis=0) + 0.05 * rng.standard_normal((5, d))
        out[-5:] = far.astype(numpy.float32)
        if metric != "L2":
            out = unit(out)
        out = numpy.ascontiguousarray(out.astype(numpy.float16 if half else numpy.float32))
        out.setflags(write=False)
        _QUERIES[key] = out
    return _QUERIES[key]


def all_distances(x, c, a, q, metric="L2", half2=False):
    """Q x N float32: the oracle's exact distance of every query to every corpus row that has a cluster, NaN elsewhere
    (rows without a cluster; every entry of a query with a NaN or inf feature).  half2: a distance that overflows the
    half range is inf in the reference's half2 arithmetic, never pushed by its search and within no radius: NaN here."""
    n, clusters = len(x), len(c)
    a = numpy.asarray(a)
    nb, dist = oracle.knn_query(n, x, c, a, q, metric=metric, half2=half2)
    members = int((a < clusters).sum())
    out = numpy.full((len(q), n), numpy.nan, numpy.float32)
    ok = nb[:, 0] != 0xFFFFFFFF
    # (the lists come out sorted: the filled slots first, then index 0 and FLT_MAX)
    rows, slots = numpy.nonzero(ok[:, None] & (dist[:, :members] != FLT_MAX))
    out[rows, nb[rows, slots].astype(numpy.int64)] = dist[rows, slots]
    assert numpy.isnan(out[:, a >= clusters]).all()
    if not half2:
        assert not numpy.isnan(out[numpy.ix_(ok, a < clusters)]).any(), "the oracle's lists are not complete"
    return out


def truth(n, d, metric="L2", half=False, q=300):
    """(x, c, a, queries, distances Q x N) of the standard case, cached."""
    key = (n, d, metric, half, q)
    if key not in _DIST:
        x, c, a = clustered(n, d, metric, half)
        qs = fresh_queries(q, n, d, metric, half)
        dm = all_distances(x, c, a, qs, metric)
        dm.setflags(write=False)
        _DIST[key] = (x, c, a, qs, dm)
    return _DIST[key]


def expected(dm, a, r):
    """(counts, offsets, neighbors, distances) of the brute-force radius search over the distance matrix dm."""
    a = numpy.asarray(a).astype(numpy.int64)
    qi, idx = numpy.nonzero(dm <= numpy.float32(r))   # (NaN compares false; row-major: ascending idx per query)
    order = numpy.lexsort((idx, a[idx], qi))
    qi, idx = qi[order], idx[order]
    counts = numpy.bincount(qi, minlength=dm.shape[0]).astype(numpy.uint32)
    offsets = numpy.zeros(dm.shape[0] + 1, numpy.int64)
    numpy.cumsum(counts, out=offsets[1:])
    return counts, offsets, idx.astype(numpy.uint32), dm[qi, idx]


def target_radius(dm, kth=21):
    """The median distance to the kth nearest clustered row."""
    finite = dm[~numpy.isnan(dm).all(axis=1)]
    return numpy.float32(numpy.median(numpy.sort(numpy.nan_to_num(finite, nan=numpy.inf), axis=1)[:, kth - 1]))


def gap_radius(dm, target, around=200):
    """The midpoint of the widest gap between consecutive distinct distances among the `around` values nearest `target`."""
    v = numpy.unique(dm[~numpy.isnan(dm)])
    near = numpy.sort(v[numpy.argsort(numpy.abs(v - target), kind="stable")[:around]])
    i = int(numpy.argmax(numpy.diff(near)))
    return numpy.float32((numpy.float64(near[i]) + numpy.float64(near[i + 1])) / 2)


def ulps_from(dm, r):
    """The smallest distance, in float32 ulps of r, between r and an entry of dm."""
    v = dm[~numpy.isnan(dm)].astype(numpy.float64)
    return float(numpy.abs(v - numpy.float64(r)).min() / numpy.spacing(numpy.float32(r)))
