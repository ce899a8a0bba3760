"""Weighted k-means++ seeding restated in numpy (DESIGN.md 4.3.1 "Seeding"), on the CPU oracle's distance, and the
fixtures tests/test_weighted_seed_ref_cpu.py and tests/test_gpu_weighted_seeding.py share.

The restatement is the reference's chooser (kmcuda.cc:262-336, as oracle/kmcuda_oracle.c: kmo_init_centroids restates
it) with the one change the design defines: where the reference sums and walks the distances d[s], the weighted
chooser sums and walks the terms t[s] = fl(w[s] * d[s]), one fp32 product rounded to nearest; d[] itself stays the
plain running minimum.  With w = 1 it IS the oracle's k-means++ (tests/test_weighted_seed_ref_cpu.py asserts the
seeds bit for bit), so nothing here is anchored on the code under test.

Beside the row ids it records, per step, what decides which path the device takes (seeding.hip): the biased-exponent
range of the non-zero finite terms (a subnormal counts as exponent 1), the number of terms under the step's exponent
cut (the outlier list), whether a term is not finite, how many are subnormal or zero, and the branch of the
reference's prefix walk that chose."""
import ctypes
import functools

import numpy

import oracle

K, SEED = 24, 3
LIST_CAP = 2048   # seeding.hip: kKmppOutCap

_libc = ctypes.CDLL(None)
_RAND_MAX = 2147483647


@functools.lru_cache(maxsize=None)
def _kmo_distance():
    """oracle.distance's C function on raw addresses: the same arithmetic, without two array conversions per call."""
    proto = ctypes.CFUNCTYPE(ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32)
    return proto(("kmo_distance", oracle.lib()))


def _metric_id(metric):
    return oracle.COS if metric in ("angular", "cos", "cosine") else oracle.L2


def distances_to_row(x32, row, metric, nan_first):
    """d[s] = oracle.distance(x[s], x[row]) in float32; 0 for a row whose first feature is NaN (kmeans.cu's plus-plus
    kernel skips such rows)."""
    fn, m, (n, dim) = _kmo_distance(), _metric_id(metric), x32.shape
    base, pitch = x32.ctypes.data, x32.strides[0]
    seed = base + row * pitch
    out = numpy.zeros(n, numpy.float32)
    for s in numpy.nonzero(~nan_first)[0].tolist():
        out[s] = fn(m, base + s * pitch, seed, dim)
    return out


def butterfly_sum(t):
    """kmcuda.cc:286-297: float sums of 32 by the warp's shuffle-down tree, accumulated in double in group order."""
    n = len(t)
    lanes = numpy.zeros((n + 31) // 32 * 32, numpy.float32)
    lanes[:n] = t
    lanes = lanes.reshape(-1, 32)
    with numpy.errstate(over="ignore", invalid="ignore"):
        for half in (16, 8, 4, 2, 1):
            lanes = lanes[:, :half] + lanes[:, half:2 * half]   # lane l += lane l + half; only lane 0 is read
        total = 0.0
        for g in lanes[:, 0].astype(numpy.float64).tolist():
            total += g
    return total


def _first_false(holds, fallback):
    """The trip at which a loop's condition first fails; `fallback` when it holds throughout."""
    stop = numpy.nonzero(~holds)[0]
    return int(stop[0]) if len(stop) else fallback


def prefix_walk(t, choice):
    """kmcuda.cc:300-326 over the terms: returns (j, branch).  Float64 and strictly sequential: numpy's accumulate is
    one running sum, element by element (the equality with the C oracle at w = 1 would show anything else)."""
    n = len(t)
    t64 = t.astype(numpy.float64)
    dist_sum = butterfly_sum(t)
    choice_approx = int(choice * n)
    with numpy.errstate(over="ignore", invalid="ignore"):
        choice_sum = choice * dist_sum

        def forward(start, total):
            # for (j = start; j < N && total < choice_sum; j++) total += t[j];
            sums = numpy.add.accumulate(numpy.concatenate([[total], t64[start:]]))
            return start + _first_false(sums < choice_sum, n - start)

        if choice_approx < 100:
            return forward(0, 0.0), "small"
        total = 0.0
        if choice_approx:
            total = float(numpy.add.accumulate(t64[:choice_approx])[-1])
        if total < choice_sum:
            return forward(choice_approx, total), "forward"
        # for (j = choice_approx; j > 1 && total >= choice_sum; j--) total -= t[j];  j++;
        assert choice_approx < n, "rand() == RAND_MAX: the reference reads past its distances"
        sums = numpy.subtract.accumulate(numpy.concatenate([[total], t64[choice_approx:1:-1]]))
        return choice_approx - _first_false(sums >= choice_sum, choice_approx - 1) + 1, "backward"


def draw_stream(seed, nan_first, clusters):
    """srand(seed); the first seed (rand() % N, redrawn while that row's feature 0 is NaN); K - 1 times
    rand() / RAND_MAX.  Drawn in one go: the stream is the process's."""
    n = len(nan_first)
    _libc.srand(ctypes.c_uint(seed))
    first = _libc.rand() % n
    while nan_first[first]:
        first = _libc.rand() % n
    return first, [(_libc.rand() + .0) / _RAND_MAX for _ in range(clusters - 1)]


def _biased_exponents(t):
    bits = numpy.ascontiguousarray(t, numpy.float32).view(numpy.uint32)
    ex = ((bits >> 23) & 0xFF).astype(numpy.int64)
    return ex, (bits & 0x7FFFFFFF) != 0


def weighted_seeds(x, w, clusters=K, seed=SEED, metric="L2", cache=None):
    """The restatement.  Returns a dict: rows (the seeds' row ids; shorter than K when a step failed), failed (None, or
    (step, j) when the walk left [1, N]: the reference's "internal bug" return), log2n, and steps: one record per step
    i = 1 .. K - 1 with emin / emax (None: no non-zero finite term), under_cut, cut, nonfinite, subnormal, zero,
    branch, choice_approx.  cache: a dict the distance columns are kept in, by row -- they depend on the rows alone."""
    x32 = numpy.ascontiguousarray(x, dtype=numpy.float32)   # halves widen exactly
    w32 = numpy.ascontiguousarray(w, dtype=numpy.float32)
    n = len(x32)
    assert w32.shape == (n,)
    nan_first = numpy.isnan(x32[:, 0])
    first, choices = draw_stream(seed, nan_first, clusters)
    log2n = (n - 1).bit_length()
    cache = {} if cache is None else cache
    rows, steps, failed = [first], [], None
    d = None
    cut = 1
    for i in range(1, clusters):
        newest = rows[-1]
        if newest not in cache:
            cache[newest] = distances_to_row(x32, newest, metric, nan_first)
        dist = cache[newest]
        if i == 1:
            d = dist.copy()
        else:
            with numpy.errstate(invalid="ignore"):
                closer = dist < d    # (a NaN on either side compares false)
            d[closer] = dist[closer]
        with numpy.errstate(over="ignore", under="ignore", invalid="ignore"):
            t = w32 * d              # float32 x float32, round to nearest
        assert t.dtype == numpy.float32
        ex, nonzero = _biased_exponents(t)
        finite = ex != 0xFF
        ee = numpy.where(ex == 0, 1, ex)
        live = finite & nonzero
        emin = int(ee[live].min()) if live.any() else None
        emax = int(ee[live].max()) if live.any() else None
        j, branch = prefix_walk(t, choices[i - 1])
        steps.append(dict(emin=emin, emax=emax, cut=cut, under_cut=int((live & (ee < cut)).sum()),
                          nonfinite=bool((~finite).any()), subnormal=int((nonzero & (ex == 0)).sum()),
                          zero=int((~nonzero).sum()), branch=branch, choice_approx=int(choices[i - 1] * n)))
        # the next step's cut (seeding.hip: kmpp_choose_kernel): this step's largest exponent + log2 N - 27
        cut = 1 if (emax is None or not finite.all()) else max(emax + log2n - 27, 1)
        if j == 0 or j > n:
            failed = (i, j)
            break
        rows.append(j - 1)
    return dict(rows=numpy.array(rows, numpy.uint32), failed=failed, steps=steps, log2n=log2n)


def outside_window(step, log2n):
    """Whether the step's terms span more binades than exact double sums allow: (emax + 1 + log2 N) - (emin - 23) > 53."""
    return step["emax"] is not None and step["emax"] - step["emin"] + log2n > 29


# ----------------------------------------------------------------------------------------------------------------------
# fixtures
# ----------------------------------------------------------------------------------------------------------------------
def _uniform(n, d, metric="L2", dtype=numpy.float32):
    x = numpy.random.RandomState(n * 7 + d).rand(n, d).astype(numpy.float32)
    if metric == "cos":
        x /= numpy.linalg.norm(x, axis=1)[:, None]
    return x.astype(dtype)


@functools.lru_cache(maxsize=None)
def rows_fixture(name):
    """(rows, metric) by name; read-only.  N = 5003 is no multiple of 32 or 256: the butterfly's tail group and the
    last 256-row block are ragged."""
    metric = "cos" if name.startswith("cos") else "L2"
    if name == "l2-5003x32":
        x = _uniform(5003, 32)
    elif name == "l2-8209x32":          # eight row shards of >= 1024 rows on 256-row boundaries, the last one ragged
        x = _uniform(8209, 32)
    elif name == "l2-5003x30":          # D % 4 != 0: the scalar chain
        x = _uniform(5003, 30)
    elif name == "cos-5003x32":
        x = _uniform(5003, 32, "cos")
    elif name == "fp16-5003x32":
        x = _uniform(5003, 32, dtype=numpy.float16)
    elif name == "wide-2000x320":       # D > 256
        x = _uniform(2000, 320)
    elif name == "dup-5003x32":         # 200 rows are copies of 200 others: zero distances inside weighted runs
        x = _uniform(5003, 32).copy()
        rs = numpy.random.RandomState(17)
        pick = rs.choice(5003, 400, replace=False)
        x[pick[:200]] = x[pick[200:]]
    elif name == "nan-5003x32":         # feature 0: the row is skipped (term 0); feature 7: its distance is NaN
        x = _uniform(5003, 32).copy()
        x[::97, 0] = numpy.nan
        x[5::101, 7] = numpy.nan
    elif name == "big-5003x32":         # every distance between two different rows exceeds 4
        x = _uniform(5003, 32) * numpy.float32(4)
    else:
        raise KeyError(name)
    x.setflags(write=False)
    return x, metric


ROWS = ["l2-5003x32", "l2-5003x30", "cos-5003x32", "fp16-5003x32", "wide-2000x320", "dup-5003x32", "nan-5003x32",
        "big-5003x32"]
FEW_LIGHT_ROWS = [0, 3, 31, 32, 100, 255, 256, 257, 2400, 2431, 2432, 2559, 2560, 2561, 4863, 4864, 4865, 4991, 4992,
                  5002]
OVERFLOW_ROWS = [150, 1200, 2500, 3800, 4900]


@functools.lru_cache(maxsize=None)
def weights_fixture(family, n):
    rs = numpy.random.RandomState(n + sum(map(ord, family)))
    w = numpy.ones(n, numpy.float32)
    if family == "ones":
        pass
    elif family == "decades":           # the ordinary case: three decades
        w = (10.0 ** rs.uniform(-1.5, 1.5, size=n)).astype(numpy.float32)
    elif family == "binades":           # eighty binades: no step's terms fit the exact window
        w = (2.0 ** rs.uniform(-40, 40, size=n)).astype(numpy.float32)
    elif family == "few-light":         # 20 rows thirty binades down, in the first, middle and last blocks
        w[FEW_LIGHT_ROWS] = 2.0 ** -30
    elif family == "many-light":        # 2500 of them: more than the outlier list holds
        w[rs.choice(n, 2500, replace=False)] = 2.0 ** -30
    elif family == "underflow":         # half the rows: their terms are subnormal (or 0 at a seed)
        w[rs.choice(n, n // 2, replace=False)] = 2.0 ** -140
    elif family == "overflow":          # 2^126 x (a distance above 4) = +inf
        w[OVERFLOW_ROWS] = 2.0 ** 126
    else:
        raise KeyError(family)
    assert numpy.isfinite(w).all() and (w > 0).all()
    w.setflags(write=False)
    return w


# the (rows, weights) pairs of the GPU tests
PAIRS = [(r, "decades") for r in ("l2-5003x32", "l2-5003x30", "cos-5003x32", "fp16-5003x32", "wide-2000x320")] + [
    ("l2-5003x32", "binades"), ("cos-5003x32", "binades"),
    ("l2-5003x32", "few-light"), ("cos-5003x32", "few-light"),
    ("l2-5003x32", "many-light"),
    ("l2-5003x32", "underflow"),
    ("dup-5003x32", "decades"),
    ("nan-5003x32", "decades"),
    ("big-5003x32", "overflow"),
]
NON_CONSTANT = ["decades", "binades", "few-light", "many-light", "underflow", "overflow"]

_columns = {}   # rows fixture -> {row: its distance column}


@functools.lru_cache(maxsize=None)
def restated(rows, weights, clusters=K, seed=SEED):
    """The restatement on a named pair, computed once per argument set.  weights: a family, or "pow2:<e>" for the
    constant 2^e."""
    x, metric = rows_fixture(rows)
    if weights.startswith("pow2:"):
        w = numpy.full(len(x), 2.0 ** int(weights[5:]), numpy.float32)
    else:
        w = weights_fixture(weights, len(x))
    return weighted_seeds(x, w, clusters, seed, metric, cache=_columns.setdefault(rows, {}))


@functools.lru_cache(maxsize=None)
def small_choice_seed(rows, clusters=K):
    """The first seed of srand() whose FIRST choice * N is below 100: the reference's `< 100` branch at step 1."""
    x, _ = rows_fixture(rows)
    nan_first = numpy.isnan(numpy.asarray(x[:, 0], numpy.float32))
    for seed in range(1, 2000):
        _, choices = draw_stream(seed, nan_first, clusters)
        if int(choices[0] * len(x)) < 100:
            return seed
    raise AssertionError("no such seed below 2000")


@functools.lru_cache(maxsize=None)
def nan_walk_seeds(clusters=K):
    """(a seed with which the NaN fixture's walk stays in range, one with which it leaves it).  A NaN term makes
    choice_sum NaN: every comparison fails, the walk ends at once, and j is 0 whenever choice * N < 100."""
    x, _ = rows_fixture("nan-5003x32")
    nan_first = numpy.isnan(x[:, 0])
    good = bad = None
    for seed in range(1, 2000):
        _, choices = draw_stream(seed, nan_first, clusters)
        small = any(int(c * len(x)) < 100 for c in choices)
        if small and bad is None:
            bad = seed
        if not small and good is None:
            good = seed
        if good is not None and bad is not None:
            return good, bad
    raise AssertionError("no such seeds below 2000")
