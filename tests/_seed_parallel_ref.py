"""k-means|| seeding restated in numpy (include/kmcuda_amd.h: kmamd_kmeans_seed_parallel), on the CPU
oracle's distance and assignment pass, and the fixtures tests/test_seed_parallel_cpu.py and
tests/test_gpu_seed_parallel.py share.

The restatement computes phi with math.fsum and lists every row inside the margin |U * phi - l * t| <= 2^-30 * l * t: on
a fixture without such rows the drawn set does not depend on the order in which phi is summed (the device's fixed
tree differs from fsum by at most N * 2^-53 relative), so row ids, round ends and counts must be EQUAL.
"""
import functools
import math

import numpy

import oracle

_MASK = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def hash64(seed, r, s):
    """h(seed, r, s) in Python integers."""
    z = (((r << 32) | s) + (seed + 1) * _GOLDEN) & _MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _MASK
    z ^= z >> 31
    return z


def uniforms(seed, r, n):
    """U(seed, r, s) for s in [0, n) as float64 (exact: 53 bits)."""
    with numpy.errstate(over="ignore"):
        z = (numpy.arange(n, dtype=numpy.uint64) + numpy.uint64((r << 32) & _MASK)
             + numpy.uint64(((seed + 1) * _GOLDEN) & _MASK))
        z ^= z >> numpy.uint64(30)
        z *= numpy.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> numpy.uint64(27)
        z *= numpy.uint64(0x94D049BB133111EB)
        z ^= z >> numpy.uint64(31)
    return (z >> numpy.uint64(11)).astype(numpy.float64) * 2.0 ** -53


def _metric_id(metric):
    return oracle.COS if metric in ("angular", "cos", "cosine") else oracle.L2


def predict(x32, c32, metric):
    """(assignments, distances) of kmeans_predict(x, c) on the oracle; one centroid: the distance to it."""
    m, n, k = _metric_id(metric), len(x32), len(c32)
    d = numpy.full(n, numpy.nan, numpy.float32)
    if k == 1:
        a = numpy.zeros(n, numpy.uint32)
    else:
        a, _, _ = oracle.lloyd_assign(x32, c32, assignments=numpy.full(n, k, numpy.uint32), metric=m)
    for i in numpy.nonzero(a < k)[0]:
        d[i] = oracle.distance(x32[i], c32[a[i]], m)
    return a, d


def _effective(t):
    """The terms as phi and the draw see them: NaN and inf count as 0."""
    return numpy.where(numpy.isfinite(t), t, numpy.float32(0)).astype(numpy.float64)


def seed_parallel(x, clusters, rounds=5, oversampling=None, metric="L2", seed=0, full=True):
    """The restatement.  Returns a dict: rows (every candidate's row id, by round), round_ends, draw_counts (rounds
    1..R), margin_rows ((round, row) pairs inside the 2^-30 margin), and with full=True counts, live_rows, live_counts
    and fell_back.  full=False stops after the last draw (no update for it, no weights)."""
    x32 = numpy.ascontiguousarray(x, dtype=numpy.float32)   # halves widen exactly
    n = len(x32)
    ell = numpy.float32(2 * clusters if oversampling is None else oversampling)
    nan_first = numpy.isnan(x32[:, 0])
    if nan_first.all():
        raise ValueError("every row's first feature is NaN")
    first = hash64(seed, 0, 0) % n
    while nan_first[first]:
        first = (first + 1) % n
    _, d = predict(x32, x32[first:first + 1], metric)
    t = numpy.where(numpy.isnan(d), numpy.float32(numpy.inf), d).astype(numpy.float32)
    t[nan_first] = 0
    rows, ends, draws, margin = [first], [1], [], []
    for r in range(1, rounds + 1):
        eff = _effective(t)
        phi = math.fsum(eff)
        lhs = uniforms(seed, r, n) * phi
        rhs = float(ell) * eff
        drawn = numpy.nonzero(lhs < rhs)[0]
        close = numpy.nonzero((numpy.abs(lhs - rhs) <= 2.0 ** -30 * rhs) & (eff > 0))[0]
        margin += [(r, int(s)) for s in close]
        draws.append(len(drawn))
        rows += [int(s) for s in drawn]
        ends.append(len(rows))
        if len(drawn) and (full or r < rounds):
            _, d = predict(x32, x32[drawn], metric)
            better = d < t   # (a NaN d compares false)
            t[better] = d[better]
    out = dict(rows=numpy.array(rows, numpy.uint32), round_ends=numpy.array(ends, numpy.uint32), draw_counts=draws,
               margin_rows=margin, first=first)
    if not full:
        return out
    total = len(rows)
    if total >= 2:
        a, _ = predict(x32, x32[out["rows"]], metric)
        counts = numpy.bincount(a[a < total], minlength=total).astype(numpy.uint32)
    else:
        counts = numpy.array([n], numpy.uint32)
    live = counts > 0
    out.update(counts=counts, live_rows=out["rows"][live], live_counts=counts[live],
               fell_back=int(live.sum()) < clusters)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# fixtures
# ----------------------------------------------------------------------------------------------------------------------
K, ROUNDS, ELL, SEED = 16, 3, 32.0, 7


def _uniform(n, d, metric="L2", dtype=numpy.float32, rs=None):
    rs = rs or numpy.random.RandomState(n * 7 + d)
    x = rs.rand(n, d).astype(numpy.float32)
    if metric == "angular":
        x /= numpy.linalg.norm(x, axis=1)[:, None]
    return x.astype(dtype)


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(rows, metric) by name; read-only arrays."""
    if name == "l2-5003x32":        # N is no multiple of 256: the tail blocks of draw, prefix and fill
        x, metric = _uniform(5003, 32), "L2"
    elif name == "angular-5003x32":
        x, metric = _uniform(5003, 32, "angular"), "angular"
    elif name == "fp16-5003x32":
        x, metric = _uniform(5003, 32, dtype=numpy.float16), "L2"
    elif name == "l2-3000x30":
        x, metric = _uniform(3000, 30), "L2"
    elif name == "wide-2000x320":   # the streamed filter
        x, metric = _uniform(2000, 320), "L2"
    elif name == "l2-4000x256":
        x, metric = _uniform(4000, 256), "L2"
    elif name == "nan-and-duplicates":
        # 60 copies of one far row: each is drawn with probability ~ 1/2 in round 1, the first of the drawn copies
        # attracts them all and the others are candidates of count 0.  Rows with a NaN first feature (term 0, no
        # cluster) and with a NaN elsewhere (every distance NaN: the term stays inf and counts as 0).
        rs = numpy.random.RandomState(11)
        x = rs.rand(5003, 16).astype(numpy.float32)
        far = rs.choice(5003, 60, replace=False)
        x[far] = x[far[0]] + numpy.float32(1000)
        rest = numpy.setdiff1d(numpy.arange(5003), far)
        x[rs.choice(rest, 40, replace=False), 0] = numpy.nan
        x[rs.choice(rest, 5, replace=False), 3] = numpy.nan
        metric = "L2"
    elif name == "fallback-40x8":
        x, metric = _uniform(40, 8), "L2"
    elif name == "blobs-8000x8":
        # 16 blobs of 500 consecutive rows, spread 1e-3 around centres at least 20 apart
        rs = numpy.random.RandomState(3)
        centres = []
        while len(centres) < 16:
            c = rs.rand(8) * 100
            if all(numpy.linalg.norm(c - o) >= 20 for o in centres):
                centres.append(c)
        x = numpy.concatenate([c + 1e-3 * rs.standard_normal((500, 8)) for c in centres]).astype(numpy.float32)
        metric = "L2"
    else:
        raise KeyError(name)
    x.setflags(write=False)
    return x, metric


def blob_of(rows):
    """The blob (nearest of the 16 centres' first members) of every given row of the blob fixture."""
    x, _ = fixture("blobs-8000x8")
    anchors = _blob_anchors()
    d = numpy.linalg.norm(rows.astype(numpy.float64)[:, None, :] - x[anchors].astype(numpy.float64)[None], axis=2)
    assert (d.min(axis=1) < 1.0).all()
    return d.argmin(axis=1)


@functools.lru_cache(maxsize=None)
def _blob_anchors():
    x, _ = fixture("blobs-8000x8")
    anchors = []
    for i in range(len(x)):
        if all(numpy.linalg.norm(x[i].astype(numpy.float64) - x[a]) > 1.0 for a in anchors):
            anchors.append(i)
        if len(anchors) == 16:
            break
    assert len(anchors) == 16
    return numpy.array(anchors)


# the fixtures of "candidates against the restatement": each at K = 16, R = 3, l = 32
CANDIDATE_FIXTURES = ["l2-5003x32", "angular-5003x32", "fp16-5003x32", "l2-3000x30", "wide-2000x320", "l2-4000x256",
                      "nan-and-duplicates"]
# l = 1 on "l2-3000x30": the seeds whose rounds (R = 6) hold one with exactly 0 and one with exactly 1 new candidate
# (tests/test_seed_parallel_cpu.py asserts the draw counts)
SPARSE = dict(fixture="l2-3000x30", clusters=4, rounds=6, oversampling=1.0, seeds=(0, 1))
SATURATION = dict(fixture="l2-5003x32", clusters=16, rounds=1, oversampling=1e9, seed=5, duplicates=(100, 2500, 5002))
FALLBACK = dict(fixture="fallback-40x8", clusters=30, rounds=1, oversampling=1.0, seed=2)
# The blob fixture at the call's defaults.  This library's k-means++ is the reference's chooser (kmcuda.cc:300-326,
# seeding.hip): it walks the prefix sums until they reach the draw and takes the row it stops AT, the row AFTER the one
# whose term carried the sum across.  A seed is therefore the successor, in candidate order, of a draw proportional to
# weight x distance.  Candidates are ordered by round and, within a round, by row; with every blob's rows consecutive
# the successor lies in the same blob unless the drawn candidate is the last of its blob in its round (about one in
# four at 2K = 64 draws per round over 16 blobs), and then in the next blob.  So a step reaches an uncovered blob with
# probability >= 0.75 while one is left, not 1: K = 16 seeds cannot be expected to cover 16 blobs, K = 32 (15 successes
# needed in 31 steps) does with a failure probability below 1e-3.
BLOBS = dict(fixture="blobs-8000x8", clusters=32, rounds=5, oversampling=None, seed=4)


def saturation_rows():
    """The saturation fixture: "l2-5003x32" with three more copies of the row that is the first candidate."""
    x, metric = fixture(SATURATION["fixture"])
    x = x.copy()
    first = hash64(SATURATION["seed"], 0, 0) % len(x)
    dup = [d for d in SATURATION["duplicates"] if d != first]
    x[dup] = x[first]
    return x, metric, first, sorted(dup)


@functools.lru_cache(maxsize=None)
def restated(name, clusters=K, rounds=ROUNDS, oversampling=ELL, seed=SEED, full=True):
    """The restatement on a named fixture, computed once per argument set."""
    if name == "saturation":
        x, metric, _, _ = saturation_rows()
    else:
        x, metric = fixture(name)
    return seed_parallel(x, clusters, rounds, oversampling, metric, seed, full)
