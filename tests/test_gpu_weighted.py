"""GPU tests of per-row sample weights: kmeans_cuda(..., sample_weight=w), kmamd_kmeans_weighted and
Engine.set_weights.  The oracle has no weighted update, so every check is built to need none: scalings that commute
with every rounding, integer weights against materialised copies on exactly summable rows, and float64 restatements
with bounds derived from the number formats."""
import ctypes

import numpy
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U = 2.0 ** -23   # one fp32 rounding, as a relative bound (half an ulp is 2^-24)


def _rows(n, d, metric, dtype, seed=0):
    x = numpy.random.RandomState(seed).rand(n, d).astype(numpy.float32)
    if metric == "cos":
        x /= numpy.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(dtype)


def _iterations():
    from kmcuda_amd import _lib
    it = ctypes.c_uint32(0)
    assert _lib.lib().kmamd_last_run_stats(ctypes.byref(it), None, None, None, None) == 0
    return it.value


# ------------------------------------------------------------------------------------------------------------------
# 1. constant power-of-two weights change nothing, bit for bit
# ------------------------------------------------------------------------------------------------------------------
_POW2_CASES = {
    # name: (n, d, k, metric, dtype, init, yinyang_t, env)
    "l2-kmpp-lloyd": (20000, 32, 50, "L2", numpy.float32, "k-means++", 0.0, {}),
    "l2-random-yy": (20000, 32, 50, "L2", numpy.float32, "random", 0.1, {}),
    "l2-import-yy": (20000, 32, 50, "L2", numpy.float32, "import", 0.1, {}),
    "cos-kmpp-lloyd": (20000, 32, 50, "cos", numpy.float32, "k-means++", 0.0, {}),
    "cos-import-yy": (20000, 32, 50, "cos", numpy.float32, "import", 0.1, {}),
    "l2-fp16-kmpp-lloyd": (20000, 32, 50, "L2", numpy.float16, "k-means++", 0.0, {}),
    "cos-fp16-random-yy": (20000, 32, 50, "cos", numpy.float16, "random", 0.1, {}),
    "l2-wide-kmpp-yy": (6000, 320, 20, "L2", numpy.float32, "k-means++", 0.1, {}),
    "l2-shards-kmpp-yy": (20000, 32, 50, "L2", numpy.float32, "k-means++", 0.1, {"KMCUDA_AMD_VIRTUAL_SHARDS": "3"}),
    "cos-shards-random-lloyd": (20000, 32, 50, "cos", numpy.float32, "random", 0.0, {"KMCUDA_AMD_VIRTUAL_SHARDS": "2"}),
    "l2-update-radix": (20000, 32, 50, "L2", numpy.float32, "random", 0.0, {"KMCUDA_AMD_UPDATE": "radix"}),
    "l2-update-sync": (20000, 32, 50, "L2", numpy.float32, "random", 0.0, {"KMCUDA_AMD_UPDATE": "sync"}),
    "l2-update-bucket": (20000, 32, 50, "L2", numpy.float32, "random", 0.0, {"KMCUDA_AMD_UPDATE": "bucket"}),
    "l2-odd-width-bucket": (8000, 30, 20, "L2", numpy.float32, "random", 0.0, {"KMCUDA_AMD_UPDATE": "bucket"}),
    "l2-odd-width-radix": (8000, 30, 20, "L2", numpy.float32, "k-means++", 0.0, {"KMCUDA_AMD_UPDATE": "radix"}),
    "l2-yy-reference": (20000, 32, 50, "L2", numpy.float32, "k-means++", 0.1, {"KMCUDA_AMD_YY": "reference"}),
}


@pytest.mark.parametrize("case", sorted(_POW2_CASES))
def test_constant_power_of_two_weights_change_nothing(case, monkeypatch):
    """w = 1, 2 and 0.5 for every row: scaling by a power of two commutes with every rounding of the sums, the
    seeding's terms and thresholds and the stop test, so centroids, assignments and the average distance are those of
    the unweighted call, bit for bit.  (w = 2 cannot be met by ignoring the weights: the cluster weights are twice the
    counts and every sum is doubled.)  KMCUDA_AMD_YY=reference shares the default update and works with weights."""
    from kmcuda_amd import kmeans_cuda
    n, d, k, metric, dtype, init, yy, env = _POW2_CASES[case]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    x = _rows(n, d, metric, dtype)
    if init == "import":
        init = x[numpy.random.RandomState(5).choice(n, k, replace=False)].copy()
    kw = dict(init=init, device=1, seed=3, tolerance=0.01, yinyang_t=yy, metric=metric, average_distance=True)
    c0, a0, d0 = kmeans_cuda(x, k, **kw)
    it0 = _iterations()
    assert it0 > 2
    for w in (1.0, 2.0, 0.5):
        c1, a1, d1 = kmeans_cuda(x, k, sample_weight=numpy.full(n, w, numpy.float32), **kw)
        assert _iterations() == it0, w
        assert numpy.array_equal(a0, a1), w
        assert numpy.array_equal(c0.view(numpy.uint16 if dtype == numpy.float16 else numpy.uint32),
                                 c1.view(numpy.uint16 if dtype == numpy.float16 else numpy.uint32)), w
        assert numpy.float32(d0).tobytes() == numpy.float32(d1).tobytes(), w


@pytest.mark.parametrize("init", ["k-means++", "random"])
def test_constant_weights_through_device_pointers(init):
    """The same invariance with every buffer a raw device pointer, the weights included."""
    from kmcuda_amd import kmeans_cuda
    from kmcuda_amd.api import free_device_ptr, _DEVICE_ALLOCS
    n, d, k = 20000, 32, 50
    x = _rows(n, d, "L2", numpy.float32)
    dev = torch.device("cuda", 0)
    xt = torch.from_numpy(x).to(dev)
    kw = dict(init=init, device=1, seed=3, tolerance=0.01, yinyang_t=0.1, average_distance=True)
    c0, a0, d0 = kmeans_cuda(x, k, **kw)
    for w in (None, 2.0, 0.5):
        wt = torch.full((n,), w, dtype=torch.float32, device=dev) if w is not None else None
        cp, ap, d1 = kmeans_cuda((xt.data_ptr(), 0, x.shape), k, sample_weight=wt.data_ptr() if w is not None else None,
                                 **kw)
        c1 = _DEVICE_ALLOCS[cp].cpu().numpy()
        a1 = _DEVICE_ALLOCS[ap].cpu().numpy().view(numpy.uint32)
        free_device_ptr(cp)
        free_device_ptr(ap)
        assert numpy.array_equal(a0, a1), w
        assert numpy.array_equal(c0.view(numpy.uint32), c1.view(numpy.uint32)), w
        assert numpy.float32(d0).tobytes() == numpy.float32(d1).tobytes(), w
    assert torch.equal(xt.cpu(), torch.from_numpy(x))


def test_native_module_takes_the_keyword():
    """libKMCUDA (the CPython module inside the library) has the same trailing keyword."""
    import libKMCUDA
    n, d, k = 8000, 16, 20
    x = _rows(n, d, "L2", numpy.float32)
    kw = dict(init="k-means++", device=1, seed=3, tolerance=0.01, yinyang_t=0)
    c0, a0 = libKMCUDA.kmeans_cuda(x, k, **kw)
    c1, a1 = libKMCUDA.kmeans_cuda(x, k, sample_weight=numpy.full(n, 2, numpy.float32), **kw)
    c2, a2 = libKMCUDA.kmeans_cuda(x, k, sample_weight=None, **kw)
    assert numpy.array_equal(a0, a1) and numpy.array_equal(c0.view(numpy.uint32), c1.view(numpy.uint32))
    assert numpy.array_equal(a0, a2) and numpy.array_equal(c0.view(numpy.uint32), c2.view(numpy.uint32))


# ------------------------------------------------------------------------------------------------------------------
# 2. integer weights equal materialised copies, bit for bit (L2)
# ------------------------------------------------------------------------------------------------------------------
_COPIES_LAYOUTS = {
    # name: (d, dtype, KMCUDA_AMD_UPDATE)
    "d16": (16, numpy.float32, None),
    "d15": (15, numpy.float32, None),          # D % 4 != 0: the scalar cluster_sums_w kernels
    "d258": (258, numpy.float32, None),        # ... with two feature trips
    "fp16-d16": (16, numpy.float16, None),     # m / 1024 is exact in half; the centroids are rounded to half after the update
    "bucket-d16": (16, numpy.float32, "bucket"),
    "radix-d16": (16, numpy.float32, "radix"),
}


@pytest.mark.parametrize("tolerance,yinyang_t,shards,layout", [
    pytest.param(tol, yy, shards, "d16", id="%s-%s-%s" % (tol, yy, shards))
    for tol, yy in [(0.0, 0.0), (0.01, 0.0), (0.01, 0.1)] for shards in [None, "3"]
] + [pytest.param(0.01, 0.0, None, layout, id=layout) for layout in ("d15", "d258", "fp16-d16", "bucket-d16", "radix-d16")])
def test_integer_weights_equal_copies(tolerance, yinyang_t, shards, layout, monkeypatch):
    """Rows are multiples of 2^-10 in [0, 1), weights in {1, 2, 3, 4}, at most 2^20 expanded rows: every partial sum of
    w x is a multiple of 2^-10 below 2^22, exact in fp64 in any order and any partition into shards, buckets or move
    lists, and both runs apply the identical (c W_old + delta) / W_new.  The weighted call on the distinct rows and the
    unweighted call on the expanded rows return identical centroids, iteration counts and assignments.  tolerance =
    0.01 is the stop-rule check (the reassigned weight against the total weight).  The layouts beside d = 16 put
    non-constant weights through the scalar kernels (d = 15, d = 258), float16 rows (exact here; both runs round the
    same centroids to half) and the forced direct and radix paths: the argument is the same for each."""
    from kmcuda_amd import kmeans_cuda
    if shards:
        monkeypatch.setenv("KMCUDA_AMD_VIRTUAL_SHARDS", shards)
    d, dtype, update = _COPIES_LAYOUTS[layout]
    if update:
        monkeypatch.setenv("KMCUDA_AMD_UPDATE", update)
    rs = numpy.random.RandomState(11)
    n, k = 30000, 32
    x = (rs.randint(0, 1024, size=(n, d)) / 1024.0).astype(numpy.float32).astype(dtype)
    assert (x.astype(numpy.float64) * 1024 == numpy.round(x.astype(numpy.float64) * 1024)).all()
    w = rs.randint(1, 5, size=n)
    big = numpy.repeat(x, w, axis=0)
    first = numpy.concatenate([[0], numpy.cumsum(w)[:-1]])
    assert len(big) <= 2 ** 20 and (big[first] == x).all()
    init = x[rs.choice(n, k, replace=False)].copy()
    kw = dict(init=init, device=1, seed=3, tolerance=tolerance, yinyang_t=yinyang_t)
    cw, aw = kmeans_cuda(x, k, sample_weight=w.astype(numpy.float32), **kw)
    itw = _iterations()
    cb, ab = kmeans_cuda(big, k, **kw)
    itb = _iterations()
    assert itw == itb and itw > 3
    bits = numpy.uint16 if dtype == numpy.float16 else numpy.uint32
    assert cw.dtype == dtype and numpy.array_equal(cw.view(bits), cb.view(bits))
    assert numpy.array_equal(aw, ab[first])
    assert (ab == numpy.repeat(aw, w)).all()


# ------------------------------------------------------------------------------------------------------------------
# 3. fractional weights against a float64 restatement
# ------------------------------------------------------------------------------------------------------------------
def _log_uniform(rs, n):
    return (10.0 ** rs.uniform(-1.5, 1.5, size=n)).astype(numpy.float32)   # three decades


def _restate(metric, c_prev, w_prev, x64, w64, prev, cur, k):
    """One update in float64 from the GPU's own fp32 centroids of the step before: (c W_old + sum_in w x - sum_out
    w x), divided by W_new (L2) or normalised (angular).  Returns (centroids, cluster weights)."""
    v = c_prev.astype(numpy.float64) * w_prev[:, None]
    wn = w_prev.copy()
    moved = prev != cur
    for s in numpy.nonzero(moved)[0]:
        if cur[s] < k:
            v[cur[s]] += w64[s] * x64[s]
            wn[cur[s]] += w64[s]
        if prev[s] < k:
            v[prev[s]] -= w64[s] * x64[s]
            wn[prev[s]] -= w64[s]
    if metric == "L2":
        return v / wn[:, None], wn
    return v / numpy.linalg.norm(v, axis=1, keepdims=True), wn


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("metric", ["L2", "cos"])
def test_step_level_fractional_weights(metric, fused):
    """Engine.set_weights, then three steps of lloyd_assign + (move_deltas, apply_delta) or the fused (reduce_fill,
    reduce_apply), with the GPU's own assignments.  Rows uniform in [0, 1) (unit length for the angular metric),
    weights log-uniform over three decades.

    L2, against the float64 weighted MEAN of the current members: the first step from zero counts computes sum(w x) /
    sum(w) in fp64 and rounds once to fp32, relative error <= 2^-23; every later incremental step starts from an
    fp32-rounded centroid and adds at most another 2^-23 on positive data: (s + 1) 2^-23 after step s.
    Angular: the update is incremental by design (normalize(c_old W_old + delta), update.hip), so the restatement is
    that formula in float64 from the GPU's own fp32 centroids of the step before; what separates the two is the fp64
    arithmetic (~1e-16 K-fold, negligible) and ONE rounding to fp32 of a positive value: relative error <= 2^-23 at
    every step.  The first step from zero counts is the normalised weighted sum of the members.
    Cluster weights (the sum of the steps' dweight, which is what the engine adds up): 1e-12 relative against the
    float64 sum over the members.  Fused buffer: its last word is the weight of the rows that changed cluster."""
    from kmcuda_amd.engine import Engine
    rs = numpy.random.RandomState(21)
    n, d, k = 8192, 64, 16
    x = _rows(n, d, metric, numpy.float32, seed=21)
    w = _log_uniform(rs, n)
    x64, w64 = x.astype(numpy.float64), w.astype(numpy.float64)
    dev = torch.device("cuda", 0)
    xs, ws = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    cen = torch.from_numpy(x[rs.choice(n, k, replace=False)].copy()).to(dev)
    asg = torch.full((n,), -1, dtype=torch.int32, device=dev)
    prev = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ccounts = torch.zeros(k, dtype=torch.int32, device=dev)
    eng = Engine(n, d, k, metric, device=0)
    plain_len = eng.reduce_len()
    eng.set_weights(ws)
    assert plain_len == k * d + k + 4 and eng.reduce_len() == plain_len + k + 1
    delta = torch.zeros(k * d, dtype=torch.float64, device=dev)
    dcount = torch.zeros(k, dtype=torch.int32, device=dev)
    buf = torch.zeros(eng.reduce_len(), dtype=torch.float64, device=dev)
    cw_run = numpy.zeros(k)        # the steps' dweight, added up as the engine adds them
    cw_prev = numpy.zeros(k)
    for step in range(3):
        c_before = cen.cpu().numpy()
        eng.reset_counters()
        eng.lloyd_assign(xs, cen, asg, prev)
        if fused:
            eng.reduce_fill(xs, prev, asg, buf)
            eng.reduce_apply(buf, cen, ccounts)
        else:
            eng.move_deltas(xs, prev, asg, delta, dcount)
            eng.apply_delta(delta, dcount, cen, ccounts)
        eng.sync()
        cur = asg.cpu().numpy().view(numpy.uint32)
        prv = prev.cpu().numpy().view(numpy.uint32)
        got = cen.cpu().numpy().astype(numpy.float64)
        counts = numpy.bincount(cur, minlength=k)
        assert (ccounts.cpu().numpy() == counts).all() and counts.min() > 0
        wsum = numpy.bincount(cur, weights=w64, minlength=k)
        ref_inc, w_inc = _restate(metric, c_before, cw_prev, x64, w64, prv, cur, k)
        if metric == "L2":
            mean = numpy.stack([(w64[cur == c, None] * x64[cur == c]).sum(0) / wsum[c] for c in range(k)])
            err = numpy.abs(got - mean) / numpy.abs(mean)
            print("step %d: max relative error against the float64 weighted mean %.3g (bound %.3g)"
                  % (step, err.max(), (step + 1) * U))
            assert err.max() <= (step + 1) * U
        else:
            if step == 0:   # from zero counts: the normalised weighted sum of the members
                s = numpy.stack([(w64[cur == c, None] * x64[cur == c]).sum(0) for c in range(k)])
                numpy.testing.assert_allclose(ref_inc, s / numpy.linalg.norm(s, axis=1, keepdims=True), rtol=1e-13)
            err = numpy.abs(got - ref_inc) / numpy.abs(ref_inc)
            print("step %d: max relative error against the float64 restatement %.3g (bound %.3g)" % (step, err.max(), U))
            assert err.max() <= U   # one fp32 rounding of a positive value (docstring)
        numpy.testing.assert_allclose(w_inc, wsum, rtol=1e-12)
        if fused:
            tail = buf.cpu().numpy()
            assert (tail[k * d:k * d + k] == counts - numpy.bincount(prv[prv < k], minlength=k)).all()
            cw_run += tail[plain_len:plain_len + k]
            numpy.testing.assert_allclose(cw_run, wsum, rtol=1e-12)
            numpy.testing.assert_allclose(tail[-1], w64[prv != cur].sum(), rtol=1e-12)
        cw_prev = wsum
    # a weight the engine refuses leaves it unweighted; None switches back
    bad = ws.clone()
    bad[17] = 0.0
    with pytest.raises(ValueError):
        eng.set_weights(bad)
    assert eng.reduce_len() == plain_len
    eng.set_weights(ws)
    eng.set_weights(None)
    assert eng.reduce_len() == plain_len
    eng.close()


def test_step_level_stop_rule_is_weighted():
    """reduce_apply_stop with weights: the update happens iff (float)changed_weight > threshold -- with a threshold
    between the reassigned weight and the reassigned row count's would-be verdict the two rules differ."""
    from kmcuda_amd.engine import Engine
    rs = numpy.random.RandomState(4)
    n, d, k = 4096, 32, 8
    x = _rows(n, d, "L2", numpy.float32, seed=4)
    w = numpy.full(n, 0.25, numpy.float32)
    dev = torch.device("cuda", 0)
    xs, ws = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    cen = torch.from_numpy(x[rs.choice(n, k, replace=False)].copy()).to(dev)
    asg = torch.full((n,), -1, dtype=torch.int32, device=dev)
    prev = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ccounts = torch.zeros(k, dtype=torch.int32, device=dev)
    eng = Engine(n, d, k, "L2", device=0)
    eng.set_weights(ws)
    buf = torch.zeros(eng.reduce_len(), dtype=torch.float64, device=dev)
    eng.stop_clear()
    eng.reset_counters()
    eng.lloyd_assign(xs, cen, asg, prev)
    eng.reduce_fill(xs, prev, asg, buf)
    before = cen.clone()
    # every row joined a cluster: changed weight = n / 4, changed rows = n.  Threshold n / 2: the weighted rule stops
    eng.reduce_apply_stop(buf, cen, ccounts, n / 2.0, 1)
    counters, stopped = eng.stop_report(1)
    assert counters[0] == n and stopped                # the report keeps counting rows
    assert torch.equal(cen, before) and int(ccounts.sum()) == 0
    assert buf[-1].item() == n / 4.0
    eng.stop_clear()
    eng.reduce_apply_stop(buf, cen, ccounts, n / 8.0, 2)
    counters, stopped = eng.stop_report(2)
    assert not stopped and int(ccounts.sum()) == n and not torch.equal(cen, before)
    eng.close()


@pytest.mark.parametrize("shards", [None, "2"])
def test_whole_call_fractional_weights(shards, monkeypatch):
    """tolerance = 0: the returned centroids are the weighted means of the returned assignments within (iterations +
    1) 2^-23 (one fp32 rounding per incremental step, positive data), and average_distance is sum(w d) / sum(w) to
    1e-6, the bar tests/test_gpu_kmeans.py holds the unweighted value to."""
    from kmcuda_amd import kmeans_cuda
    if shards:
        monkeypatch.setenv("KMCUDA_AMD_VIRTUAL_SHARDS", shards)
    rs = numpy.random.RandomState(8)
    n, d, k = 20000, 8, 20
    x = rs.rand(n, d).astype(numpy.float32)
    w = _log_uniform(rs, n)
    cen, asg, avg = kmeans_cuda(x, k, init="k-means++", device=1, seed=3, tolerance=0, yinyang_t=0,
                                average_distance=True, sample_weight=w)
    its = _iterations()
    x64, w64 = x.astype(numpy.float64), w.astype(numpy.float64)
    wsum = numpy.bincount(asg, weights=w64, minlength=k)
    assert wsum.min() > 0
    mean = numpy.stack([(w64[asg == c, None] * x64[asg == c]).sum(0) / wsum[c] for c in range(k)])
    err = (numpy.abs(cen - mean) / numpy.abs(mean)).max()
    print("%d iterations: max relative error %.3g (bound %.3g)" % (its, err, (its + 1) * U))
    assert err <= (its + 1) * U
    dist = numpy.linalg.norm(x64 - cen.astype(numpy.float64)[asg], axis=1)
    valid = (w64 * dist).sum() / w64.sum()
    print("average distance %.9g, float64 %.9g" % (avg, valid))
    assert abs(valid - avg) < 1e-6
    # the weights matter: the unweighted run ends elsewhere
    c_plain, _ = kmeans_cuda(x, k, init="k-means++", device=1, seed=3, tolerance=0, yinyang_t=0)
    assert not numpy.array_equal(c_plain, cen)


# ------------------------------------------------------------------------------------------------------------------
# 4. weighted k-means++ uses the weights
# ------------------------------------------------------------------------------------------------------------------
def test_weighted_kmeanspp_uses_the_weights():
    """Two blobs 100 apart; the far one weighs 2^-60 per row, the near one 1.  tolerance = 1 stops the run at the first
    stop test, before any update: the returned centroids ARE the seeds.  The first seed is the reference's uniform
    rand() % N draw -- excluded by construction: only seeds of srand() whose first draw lands in the near blob are
    used.  No weighted run draws a seed from the far blob; every unweighted run on the same rows does (its rows carry
    ~99 % of the distance mass), so the check cannot pass vacuously.  (The far rows come last: the reference's
    sequential prefix sum then never ends on one of them by its own off-by-one.)"""
    from kmcuda_amd import kmeans_cuda
    rs = numpy.random.RandomState(2)
    n_near, n_far, d, k = 3000, 3000, 4, 4
    x = rs.rand(n_near + n_far, d).astype(numpy.float32)
    x[n_near:] += 100.0
    w = numpy.ones(n_near + n_far, numpy.float32)
    w[n_near:] = 2.0 ** -60
    libc = ctypes.CDLL(None)
    seeds = []
    for seed in range(1, 200):
        libc.srand(seed)
        if libc.rand() % len(x) < n_near:
            seeds.append(seed)
        if len(seeds) == 6:
            break
    assert len(seeds) == 6
    for seed in seeds:
        kw = dict(init="k-means++", device=1, seed=seed, tolerance=1.0, yinyang_t=0)
        cw, _ = kmeans_cuda(x, k, sample_weight=w, **kw)
        assert _iterations() == 1
        assert (cw[:, 0] < 50).all(), (seed, cw[:, 0])
        assert all((x == row).all(axis=1).any() for row in cw)      # seeds are rows
        cp, _ = kmeans_cuda(x, k, **kw)
        assert (cp[0] == cw[0]).all()                                # the same uniform first seed
        assert (cp[:, 0] > 50).any(), (seed, cp[:, 0])


# ------------------------------------------------------------------------------------------------------------------
# 5. refusals that need a device; emptied clusters
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), 0.0, -1.0, -0.0])
@pytest.mark.parametrize("shards", [None, "3"])
def test_invalid_weight_values_are_refused(bad, shards, monkeypatch):
    """A NaN, an inf, a zero or a negative weight anywhere: InvalidArguments (ValueError in Python) before any
    clustering work, outputs untouched."""
    from kmcuda_amd import kmeans_cuda, _lib
    if shards:
        monkeypatch.setenv("KMCUDA_AMD_VIRTUAL_SHARDS", shards)
    L = _lib.lib()
    n, d, k = 5000, 8, 10
    x = _rows(n, d, "L2", numpy.float32)
    w = numpy.ones(n, numpy.float32)
    w[n - 7] = bad
    with pytest.raises(ValueError):
        kmeans_cuda(x, k, device=1, seed=3, sample_weight=w)
    cen = numpy.full((k, d), 7, numpy.float32)
    asg = numpy.full(n, 0x5A5A5A5A, numpy.uint32)
    avg = ctypes.c_float(-3.0)
    rc = L.kmamd_kmeans_weighted(1, None, 0.01, 0.1, 0, n, d, k, 3, 1, -1, 0, 0, x.ctypes.data, cen.ctypes.data,
                                 asg.ctypes.data, ctypes.cast(ctypes.byref(avg), ctypes.c_void_p), w.ctypes.data)
    assert rc == 1
    assert (cen == 7).all() and (asg == 0x5A5A5A5A).all() and avg.value == -3.0
    # ... and a null weight pointer is kmeans_cuda itself
    rc = L.kmamd_kmeans_weighted(1, None, 0.01, 0.1, 0, n, d, k, 3, 1, -1, 0, 0, x.ctypes.data, cen.ctypes.data,
                                 asg.ctypes.data, None, None)
    assert rc == 0
    c0, a0 = kmeans_cuda(x, k, device=1, seed=3)
    assert numpy.array_equal(c0.view(numpy.uint32), cen.view(numpy.uint32)) and numpy.array_equal(a0, asg)


def test_reference_arithmetic_modes_refuse_weights_on_the_gpu(monkeypatch):
    from kmcuda_amd import kmeans_cuda
    x = _rows(5000, 8, "L2", numpy.float32)
    w = numpy.ones(5000, numpy.float32)
    with pytest.raises(ValueError):
        kmeans_cuda(x, 10, init="afkmc2", device=1, seed=3, sample_weight=w)
    with pytest.raises(ValueError):
        kmeans_cuda(x, 10, init=("afkmc2", 50), device=1, seed=3, sample_weight=w)
    monkeypatch.setenv("KMCUDA_AMD_EXACT_UPDATE", "1")
    with pytest.raises(ValueError):
        kmeans_cuda(x, 10, device=1, seed=3, sample_weight=w)
    kmeans_cuda(x, 10, device=1, seed=3)                      # without weights the mode is what it was
    monkeypatch.delenv("KMCUDA_AMD_EXACT_UPDATE")
    monkeypatch.setenv("KMCUDA_AMD_FP16_STRICT", "1")
    with pytest.raises(ValueError):
        kmeans_cuda(x.astype(numpy.float16), 10, device=1, seed=3, sample_weight=w)
    kmeans_cuda(x, 10, device=1, seed=3, sample_weight=w)    # fp32 rows: the switch does not apply


def test_cluster_emptied_during_a_weighted_run():
    """Centroid 1 holds two rows after the first pass and loses both in the second: its member COUNT is 0, so it gets
    NaN centroids -- whatever rounding residue its running weight would have -- and is never chosen again."""
    from kmcuda_amd import kmeans_cuda
    rs = numpy.random.RandomState(0)
    x = numpy.zeros((102, 2), numpy.float32)
    x[:50, 0] = 3.0
    x[50, 0] = 4.0
    x[51, 0] = 8.2
    x[52:, 0] = 9.2
    w = _log_uniform(rs, 102)
    w[50] = w[51] = 0.7          # (equal: centroid 1 moves to their midpoint, 6.1, and both are nearer to a neighbour)
    init = numpy.array([[0, 0], [6.1, 0], [12.2, 0]], numpy.float32)
    cen, asg = kmeans_cuda(x, 3, init=init, device=1, seed=3, tolerance=0, yinyang_t=0, sample_weight=w)
    assert _iterations() >= 3
    assert numpy.isnan(cen[1]).all() and not (asg == 1).any()
    assert (asg[:51] == 0).all() and (asg[51:] == 2).all()
    w64 = w.astype(numpy.float64)
    for c, rows in ((0, slice(0, 51)), (2, slice(51, 102))):
        mean = (w64[rows] * x[rows, 0]).sum() / w64[rows].sum()
        assert abs(cen[c, 0] - mean) <= 4 * U * mean and cen[c, 1] == 0


def test_identical_calls_give_identical_bits():
    """The weight sums are taken in a fixed order (no floating-point atomics): two identical calls agree bit for bit."""
    from kmcuda_amd import kmeans_cuda
    rs = numpy.random.RandomState(3)
    x = rs.rand(30000, 24).astype(numpy.float32)
    w = _log_uniform(rs, 30000)
    kw = dict(init="k-means++", device=1, seed=5, tolerance=0.003, yinyang_t=0.1, average_distance=True, sample_weight=w)
    c0, a0, d0 = kmeans_cuda(x, 40, **kw)
    it0 = _iterations()
    c1, a1, d1 = kmeans_cuda(x, 40, **kw)
    assert _iterations() == it0
    assert numpy.array_equal(c0.view(numpy.uint32), c1.view(numpy.uint32)) and numpy.array_equal(a0, a1) and d0 == d1
