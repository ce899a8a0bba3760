"""Mini-batch K-means on the GPU (kmcuda_amd.MiniBatchKMeans, kmeans_minibatch; C ABI kmamd_minibatch_*) against the
numpy restatement of tests/_minibatch_ref.py: bit for bit on the grid fixtures, whose sums do not depend on their
order (tests/test_minibatch_cpu.py asserts that), within a bound derived from the data elsewhere."""
import ctypes

import numpy
import pytest

import _minibatch_ref as ref
import _seed_parallel_ref as spref

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _same_bits(a, b):
    a, b = numpy.ascontiguousarray(a), numpy.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _model(c, **kw):
    from kmcuda_amd import MiniBatchKMeans
    return MiniBatchKMeans(c, **kw)


# ---- 1. three steps against the restatement on a grid fixture --------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("shape", ref.GRID_SHAPES, ids=["%dx%d-k%d" % s for s in ref.GRID_SHAPES])
def test_three_steps_equal_the_restatement_bit_for_bit(shape, weighted):
    c, batches, weights = ref.grid(*shape, weighted)
    want = ref.grid_restated(*shape, weighted)
    with _model(c) as m:
        for i, x in enumerate(batches):
            a = m.partial_fit(x, sample_weight=weights[i] if weighted else None, return_assignments=True)
            assert (a == want[i]["assignments"]).all(), i
            assert _same_bits(m.centroids, want[i]["centroids"]), i
            assert _same_bits(m.cluster_weights, want[i]["weights"]), i
            assert m.steps_done == i + 1


# ---- 2. weights and copies ---------------------------------------------------------------------------------------------
def test_integer_weights_equal_materialised_copies():
    c, batches, weights = ref.grid(255, 30, 16, True)
    with _model(c) as mw, _model(c) as mc:
        for x, w in zip(batches, weights):
            mw.partial_fit(x, sample_weight=w)
            mc.partial_fit(numpy.repeat(x, w.astype(numpy.int64), axis=0))
            assert _same_bits(mw.centroids, mc.centroids)
            assert _same_bits(mw.cluster_weights, mc.cluster_weights)


@pytest.mark.parametrize("d", [30, 32])
def test_constant_weight_one_equals_no_weights(d):
    rs = numpy.random.RandomState(d)
    x = rs.standard_normal((5003, d)).astype(numpy.float32)
    c = x[rs.choice(len(x), 16, replace=False)]
    with _model(c) as m1, _model(c) as m0:
        for lo in (0, 2000):
            m1.partial_fit(x[lo:lo + 3003], sample_weight=numpy.ones(3003, numpy.float32))
            m0.partial_fit(x[lo:lo + 3003])
        assert _same_bits(m1.centroids, m0.centroids)
        assert _same_bits(m1.cluster_weights, m0.cluster_weights)


# ---- 3. skew -----------------------------------------------------------------------------------------------------------
def _skewed():
    """K = 8, D = 32 on the grid: 4500 of 5003 rows in cluster 0, one row in cluster 1, the rest in cluster 2, a NaN
    centroid (3), four far centroids without a member (4..7), 12 rows with a NaN first feature."""
    rs = numpy.random.RandomState(42)
    d = 32
    c = numpy.zeros((8, d), numpy.float32)
    c[1], c[2], c[3] = 3.0, -3.0, numpy.nan
    for k in range(4, 8):
        c[k] = 3.5 * numpy.where((numpy.arange(d) >> (k - 4)) & 1, 1.0, -1.0)
    near = lambda n, at: (at + rs.randint(-16, 17, size=(n, d)) / 32.0).astype(numpy.float32)
    x = numpy.concatenate([near(4500, 0.0), near(1, 3.0), near(490, -3.0), near(12, 0.0)])
    x[-12:, 0] = numpy.nan
    x = x[rs.permutation(len(x))]
    w0 = numpy.array([5, 0, 2, 7, 3, 0, 1, 4], numpy.float64)
    return c, w0, x


def test_skewed_batch_nan_centroid_nan_rows_and_an_empty_step():
    c, w0, x = _skewed()
    want = ref.step(c, w0, x, exact=True)
    counts = numpy.bincount(want["assignments"], minlength=9)
    assert counts[0] > 4096 and counts[1] == 1 and counts[2] == 490 and not counts[3:8].any() and counts[8] == 12
    with _model(c, cluster_weights=w0) as m:
        a = m.partial_fit(x, return_assignments=True)
        got_c, got_w = m.centroids, m.cluster_weights
        assert (a == want["assignments"]).all()
        assert (a[numpy.isnan(x[:, 0])] == 8).all()
        assert _same_bits(got_c, want["centroids"]) and _same_bits(got_w, want["weights"])
        # the clusters without a member: byte-identical to before, the NaN centroid among them
        assert got_c[3:].tobytes() == c[3:].tobytes() and got_w[3:].tobytes() == w0[3:].tobytes()
        assert numpy.isnan(got_c[3]).all()
        # rows that take no part change nothing; an empty batch changes nothing but the counter
        nan_rows = x[numpy.isnan(x[:, 0])]
        assert (m.partial_fit(nan_rows, return_assignments=True) == 8).all()
        m.partial_fit(numpy.zeros((0, 32), numpy.float32))
        assert m.steps_done == 3
        assert _same_bits(m.centroids, got_c) and _same_bits(m.cluster_weights, got_w)


# ---- 4. general data and the angular metric --------------------------------------------------------------------------------
def _general(metric, d):
    rs = numpy.random.RandomState(17 + d)
    x = rs.standard_normal((3 * 5003, d)).astype(numpy.float32)
    if metric == "angular":
        x /= numpy.linalg.norm(x, axis=1)[:, None]
    c = x[rs.choice(len(x), 16, replace=False)].copy()
    # weights with few bits: their fp64 sums are exact in any order, so W must be EQUAL
    w = (rs.randint(1, 9, size=len(x)) / 4.0).astype(numpy.float32)
    return c, x.reshape(3, 5003, d), w.reshape(3, 5003)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("metric,d", [("L2", 32), ("L2", 30), ("angular", 32), ("angular", 30)])
def test_one_step_from_an_exported_state_within_the_summation_bound(metric, d, weighted):
    """|C' - restated C'| <= one float32 ulp of the restated value + the fp64 order-dependent error of S_c carried through
    the step: m 2^-52 sum|w x_f| / W' under L2 (m members; any association of m terms errs by at most (m - 1) 2^-53 times
    the sum of their magnitudes).  Angular, v = C W + S, r = |v|: dv_f = m 2^-52 sum|w x_f| + 2^-52 |v_f| (the sum and
    the rounding of the addition), d(r^2) <= 2 sum_f |v_f| dv_f + D 2^-52 r^2 (the squares and their sum in any order),
    dr = d(r^2) / (2 r) + 2^-52 r (the root), and |d(v_f / r)| <= dv_f / r + |v_f| dr / r^2."""
    c, xs, ws = _general(metric, d)
    with _model(c, metric=metric) as m:
        for i in range(2):
            m.partial_fit(xs[i], sample_weight=ws[i] if weighted else None)
        c0, w0 = m.centroids, m.cluster_weights   # the state exported from the GPU
        a = m.partial_fit(xs[2], sample_weight=ws[2] if weighted else None, return_assignments=True)
        got_c, got_w = m.centroids, m.cluster_weights
    want = ref.step(c0, w0, xs[2], ws[2] if weighted else None, metric)
    assert (a == want["assignments"]).all()
    assert _same_bits(got_w, want["weights"])
    eps, worst = 2.0 ** -52, 0.0
    visited = numpy.zeros(len(c), bool)
    for j, cl in enumerate(want["clusters"]):
        visited[cl] = True
        members, abs_sums, v = len(want["members"][j]), want["abs_sums"][j], want["v"][j]
        restated = want["centroids"][cl]
        ulp = numpy.spacing(numpy.abs(restated)).astype(numpy.float64)
        if metric == "L2":
            bound = ulp + members * eps * abs_sums / want["weights"][cl]
        else:
            r = want["norm"][j]
            dv = members * eps * abs_sums + eps * numpy.abs(v)
            dr = (2.0 * (numpy.abs(v) * dv).sum() + d * eps * r * r) / (2.0 * r) + eps * r
            bound = ulp + dv / r + numpy.abs(v) * dr / (r * r)
        err = numpy.abs(got_c[cl].astype(numpy.float64) - restated.astype(numpy.float64))
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), cl
    print("largest error / bound over %d clusters: %.3g" % (len(want["clusters"]), worst))
    assert got_c[~visited].tobytes() == c0[~visited].tobytes()


@pytest.mark.parametrize("metric", ["L2", "angular"])
def test_two_identical_runs_of_five_steps_are_bit_identical(metric):
    c, xs, ws = _general(metric, 32)
    batches = [xs[i % 3][(i * 400):(i * 400) + 3000] for i in range(5)]
    wts = [ws[i % 3][(i * 400):(i * 400) + 3000] for i in range(5)]
    runs = []
    for _ in range(2):
        with _model(c, metric=metric) as m:
            for x, w in zip(batches, wts):
                m.partial_fit(x, sample_weight=w)
            runs.append((m.centroids, m.cluster_weights))
    assert _same_bits(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1])


# ---- 5. fit and partial_fit ------------------------------------------------------------------------------------------------
def _corpus(dtype):
    rs = numpy.random.RandomState(23)
    x = rs.standard_normal((5003, 32)).astype(dtype)
    c = x[rs.choice(len(x), 16, replace=False)].astype(numpy.float32)
    w = (0.25 + rs.rand(len(x))).astype(numpy.float32)
    return c, x, w


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("dtype", [numpy.float32, numpy.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("kind", ["numpy", "tensor"])
def test_fit_is_partial_fit_on_the_drawn_rows(kind, dtype, weighted):
    torch = _torch()
    c, x, w = _corpus(dtype)
    with _model(c) as m:
        for t in range(4):
            idx = ref.draw(7, t, 1000, len(x))
            m.partial_fit(x[idx], sample_weight=w[idx] if weighted else None)
        want_c, want_w = m.centroids, m.cluster_weights
    if kind == "tensor":
        dev = torch.device("cuda", 0)
        corpus, cw, seeds = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev), torch.from_numpy(c).to(dev)
    else:
        corpus, cw, seeds = x, w, c
    results = []
    for plan in ((4,), (2, 2)):   # fit twice with 2 steps is fit once with 4
        with _model(seeds) as m:
            for steps in plan:
                m.fit(corpus, steps, 1000, seed=7, sample_weight=cw if weighted else None)
            assert m.steps_done == 4
            got_c, got_w = m.centroids, m.cluster_weights
        if kind == "tensor":
            assert got_c.is_cuda and got_c.dtype == torch.float32 and got_w.dtype == torch.float64
            got_c, got_w = got_c.cpu().numpy(), got_w.cpu().numpy()
        results.append((got_c, got_w))
    for got_c, got_w in results:
        assert _same_bits(got_c, want_c) and _same_bits(got_w, want_w)


def test_partial_fit_of_a_device_tensor_is_partial_fit_of_its_host_copy():
    torch = _torch()
    c, x, w = _corpus(numpy.float32)
    dev = torch.device("cuda", 0)
    with _model(c) as mh, _model(torch.from_numpy(c).to(dev)) as md:
        ah = mh.partial_fit(x, sample_weight=w, return_assignments=True)
        ad = md.partial_fit(torch.from_numpy(x).to(dev), sample_weight=torch.from_numpy(w).to(dev),
                            return_assignments=True)
        assert ad.is_cuda and ad.dtype == torch.int32
        assert (ad.cpu().numpy().view(numpy.uint32) == ah).all()
        assert _same_bits(md.centroids.cpu().numpy(), mh.centroids)
        assert _same_bits(md.cluster_weights.cpu().numpy(), mh.cluster_weights)


def test_a_step_beyond_the_chunk_is_refused(monkeypatch):
    c, x, _ = _corpus(numpy.float32)
    monkeypatch.setenv("KMCUDA_AMD_ASSIGN_CHUNK", "100")
    with _model(c) as m:
        m.partial_fit(x[:100])
        before = (m.centroids, m.cluster_weights)
        with pytest.raises(ValueError):
            m.partial_fit(x[:101])
        with pytest.raises(ValueError):
            m.fit(x, 2, 1000)
        assert m.steps_done == 1
        assert _same_bits(m.centroids, before[0]) and _same_bits(m.cluster_weights, before[1])
        m.fit(x, 2, 100)
        assert m.steps_done == 3


def test_refusals_on_a_live_model_leave_the_state_alone(monkeypatch):
    from kmcuda_amd import _lib
    c, x, _ = _corpus(numpy.float32)
    odd = numpy.zeros((4, 7), numpy.float32)
    with _model(c) as m, _model(odd) as mo:
        before = (m.centroids, m.cluster_weights)
        for bad in (numpy.nan, numpy.inf, 0.0, -1.0):
            w = numpy.ones(len(x), numpy.float32)
            w[4001] = bad
            with pytest.raises(ValueError):
                m.partial_fit(x, sample_weight=w)
            with pytest.raises(ValueError):
                m.fit(x, 2, 500, sample_weight=w)
        L = _lib.lib()
        assert L.kmamd_minibatch_step(m.h, 10, 0, None, None, None, -1) == 1            # null rows
        assert L.kmamd_minibatch_step(m.h, 10, 0, x.ctypes.data, None, None, 1) == 1    # another device
        assert L.kmamd_minibatch_fit(m.h, 0, 0, x.ctypes.data, None, 10, 1, 0, -1) == 1   # N = 0
        assert L.kmamd_minibatch_fit(m.h, 100, 0, x.ctypes.data, None, 0, 1, 0, -1) == 1   # batch = 0
        assert L.kmamd_minibatch_fit(m.h, 100, 0, None, None, 10, 1, 0, -1) == 1         # null samples
        h16 = numpy.zeros((10, 8), numpy.float16)
        assert L.kmamd_minibatch_step(mo.h, 10, 1, h16.ctypes.data, None, None, -1) == 1   # odd D with fp16x2
        monkeypatch.setenv("KMCUDA_AMD_FP16_STRICT", "1")
        x16 = x.astype(numpy.float16)
        assert L.kmamd_minibatch_step(m.h, 10, 1, x16.ctypes.data, None, None, -1) == 1
        with pytest.raises(ValueError):
            m.partial_fit(x16)
        monkeypatch.delenv("KMCUDA_AMD_FP16_STRICT")
        assert m.steps_done == 0 and mo.steps_done == 0
        assert _same_bits(m.centroids, before[0]) and _same_bits(m.cluster_weights, before[1])
    bad_cw = _torch().tensor([1.0, -1.0] + [0.0] * 14, dtype=_torch().float64, device="cuda:0")
    h = ctypes.c_void_p()
    dc = _torch().from_numpy(c).to("cuda:0")
    rc = _lib.lib().kmamd_minibatch_create(ctypes.byref(h), 0, 32, 16, 0, 0, 0, ctypes.c_void_p(dc.data_ptr()),
                                           ctypes.c_void_p(bad_cw.data_ptr()))
    assert rc == 1 and not h.value


# ---- 6. against the existing update ---------------------------------------------------------------------------------------
def test_one_step_from_weight_zero_equals_lloyd_assign_move_deltas_apply_delta():
    torch = _torch()
    from kmcuda_amd.engine import Engine
    n, d, k = 5003, 32, 16
    c, batches, _ = ref.grid(n, d, k, False)
    x = batches[0]
    with _model(c) as m:
        a = m.partial_fit(x, return_assignments=True)
        got_c, got_w = m.centroids, m.cluster_weights
    dev = torch.device("cuda", 0)
    xs, cs = torch.from_numpy(x.copy()).to(dev), torch.from_numpy(c.copy()).to(dev)
    asg = torch.full((n,), k, dtype=torch.int32, device=dev)
    prev = torch.full((n,), k, dtype=torch.int32, device=dev)
    none = torch.full((n,), k, dtype=torch.int32, device=dev)
    delta = torch.zeros((k * d,), dtype=torch.float64, device=dev)
    dcount = torch.zeros((k,), dtype=torch.int32, device=dev)
    ccounts = torch.zeros((k,), dtype=torch.int32, device=dev)
    eng = Engine(n, d, k, "L2", device=0)
    eng.lloyd_assign(xs, cs, asg, prev)
    eng.move_deltas(xs, none, asg, delta, dcount)
    eng.apply_delta(delta, dcount, cs, ccounts)
    eng.sync()
    lloyd_c, counts = cs.cpu().numpy(), ccounts.cpu().numpy()
    eng.close()
    assert (asg.cpu().numpy().view(numpy.uint32) == a).all()
    assert (counts > 0).sum() >= 2
    visited = counts > 0
    assert _same_bits(got_c[visited], lloyd_c[visited])
    assert (got_w == counts).all()
    assert got_c[~visited].tobytes() == c[~visited].tobytes()   # where the Lloyd update writes NaN


# ---- 7. blobs ----------------------------------------------------------------------------------------------------------------
def test_blobs_every_centroid_ends_inside_its_blob():
    x, _ = spref.fixture("blobs-8000x8")
    anchors = spref._blob_anchors()   # one row per blob
    seeds = x[anchors]
    with _model(seeds) as m:
        m.fit(x, 20, 512, seed=5)
        c, w = m.centroids, m.cluster_weights
    assert w.sum() == 20 * 512 and (w > 0).all()
    x64 = x.astype(numpy.float64)
    # a centre is a convex combination of drawn members of its blob (W started at 0), rounded to float32
    rounding = numpy.sqrt(x.shape[1]) * float(numpy.spacing(numpy.abs(x).max()))
    for j, row in enumerate(anchors):
        blob = x64[row // 500 * 500:(row // 500 + 1) * 500]
        mean = blob.mean(axis=0)
        radius = numpy.linalg.norm(blob - mean, axis=1).max()
        assert numpy.linalg.norm(c[j].astype(numpy.float64) - mean) <= radius + rounding, j


# ---- 8. the one-shot call ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["numpy", "tensor"])
@pytest.mark.parametrize("init", ["array", "k-means||"])
def test_kmeans_minibatch_one_shot(init, kind):
    torch = _torch()
    from kmcuda_amd import kmeans_minibatch
    c, x, _ = _corpus(numpy.float32)
    if kind == "tensor":
        dev = torch.device("cuda", 0)
        x, c = torch.from_numpy(x).to(dev), torch.from_numpy(c).to(dev)
    start = c if init == "array" else "k-means||"
    outs = [kmeans_minibatch(x, 16, 500, 3, init=start, seed=11) for _ in range(2)]
    for cen, w in outs:
        if kind == "tensor":
            assert cen.is_cuda and w.is_cuda and cen.dtype == torch.float32 and w.dtype == torch.float64
            assert tuple(cen.shape) == (16, 32) and tuple(w.shape) == (16,)
        else:
            assert isinstance(cen, numpy.ndarray) and cen.dtype == numpy.float32 and cen.shape == (16, 32)
            assert isinstance(w, numpy.ndarray) and w.dtype == numpy.float64 and w.shape == (16,)
    host = [(cen.cpu().numpy(), w.cpu().numpy()) if kind == "tensor" else (cen, w) for cen, w in outs]
    assert _same_bits(host[0][0], host[1][0]) and _same_bits(host[0][1], host[1][1])
    assert host[0][1].sum() == 3 * 500
