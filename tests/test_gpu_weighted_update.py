"""The weighted centroid update (update.hip: cluster_sums_w_kernel<DIRECT, VEC4>, the weighted apply_delta) with
PER-ROW weights on every host path and both feature mappings, driven with synthetic (prev, cur) pairs as
tests/test_gpu_kmeans.py::test_update_host_logic drives the unweighted one.

The inputs are exactly summable (tests/_weighted_inputs.py): every partial sum of w * x and of w is exact in fp64 in
any order, so the move sums are compared with a float64 numpy reference BIT FOR BIT -- no tolerance.  A weight read at
the list position instead of at the row the list names, a dropped tail row or a doubled row changes the result."""
import numpy
import pytest

from _weighted_inputs import exact_rows, exact_weights, index_weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U = 2.0 ** -23   # one fp32 rounding, as a relative bound (half an ulp is 2^-24)
NONE = -1        # 0xFFFFFFFF: the row has no cluster


def bucket_cap(n, k):
    """move_bucket_cap() of update.hip, restated: the rows a direct-path bucket holds."""
    cap = 32
    while cap < 4096 and cap * 2 * k <= n:
        cap <<= 1
    return cap


def sum_groups(d, vec4):
    """Row groups of cluster_sums_body's two mappings at width d (1024 threads / lanes per row)."""
    if vec4:
        fl = 16
        while fl < 256 and fl * 4 < d:
            fl <<= 1
    else:
        fl = 256 if d > 128 else (128 if d > 64 else 64)
    return 1024 // fl


# name: (n, d, k, rows in a view one float past a 16-byte boundary, VEC4 kernels expected, cap expected)
_LAYOUTS = {
    "d24-vec4": (20000, 24, 8, False, True, 2048),                # one trip, lanes beyond D idle
    "d30-scalar": (20000, 30, 8, False, False, 2048),             # D % 4 != 0, fl = 64
    "d7-scalar": (20000, 7, 8, False, False, 2048),
    "d258-scalar-two-trips": (20000, 258, 8, False, False, 2048),  # two feature trips of 256
    "d1032-vec4-two-trips": (6144, 1032, 8, False, True, 512),    # two trips of 1024 features
    "d32-offset-view-scalar": (20000, 32, 8, True, False, 2048),  # scalar kernels chosen by alignment, not width
}


def _lists(prev, cur, k):
    """Lengths of the (in, out) move lists per centroid, by move_flags()'s rule."""
    moved = prev != cur
    ein = moved & (cur >= 0) & (cur < k)
    eout = moved & (prev >= 0) & (prev < k)
    return (numpy.bincount(cur[ein], minlength=k), numpy.bincount(prev[eout], minlength=k))


def _moved(rs, prev, moves):
    """cur = prev with `count` rows of cluster src sent to dst, for every (src, dst, count); count None = all."""
    cur = prev.copy()
    assert len({m[0] for m in moves}) == len(moves)   # one move per source: no row moves twice
    for src, dst, count in moves:
        rows = numpy.nonzero(prev == src)[0]
        count = len(rows) if count is None else count
        assert len(rows) >= count > 0, (src, len(rows), count)
        cur[rs.choice(rows, count, replace=False)] = dst
    return cur


def _sequence(n, d, k, vec4):
    """The synthetic (prev, cur) pairs.  Every intended list length is asserted against the bucket capacity and the
    mappings' thresholds, so a later change of move_bucket_cap() or of the 128-row switch fails here instead of
    silently skipping a branch of cluster_sums_body."""
    rs = numpy.random.RandomState(1234)
    cap = bucket_cap(n, k)
    groups = sum_groups(d, vec4)
    assert k == 8 and n % k == 0
    seq = []
    base = rs.permutation(numpy.arange(n, dtype=numpy.int32) % k).astype(numpy.int32)

    # 0. all-join: every row comes from "no cluster"; every list is far beyond the capacity
    none = numpy.full(n, NONE, numpy.int32)
    nin, nout = _lists(none, base, k)
    assert (nin == n // k).all() and (nout == 0).all() and n // k > cap
    seq.append(("all-join", none, base))

    # 1. short lists (1..127 rows: the scalar mapping inside the VEC4 kernels), lengths no multiples of 8; a single-row
    #    list; empty in-list with a non-empty out-list (0, 4, 6) and the reverse (1, 5); no event at all (7); rows that
    #    leave and join none (cur = K)
    a1 = _moved(rs, base, [(0, 1, 1), (2, 3, 127), (3, 2, 61), (4, k, 13), (6, 5, 7)])
    nin, nout = _lists(base, a1, k)
    assert list(nin) == [0, 1, 61, 127, 0, 7, 0, 0] and list(nout) == [1, 0, 127, 61, 13, 0, 7, 0]
    assert all(0 < v < 128 and v % 8 for v in list(nin) + list(nout) if v)
    assert nin.sum() == nout.sum() - 13                      # the 13 rows count as leaves only
    seq.append(("short", base, a1))

    # 2. mid lists (128..1024 rows and within the capacity: rank sort, four-feature mapping in the VEC4 kernels), lengths
    #    no multiples of 4 and no multiples of the group count; rows that leave for cur > K; a short pair beside them
    big = min(1023, cap - 1)
    a2 = _moved(rs, a1, [(0, 1, 443), (1, 0, 130), (2, 3, big), (3, 4, 257), (5, k + 5, 131), (7, 6, 5)])
    nin, nout = _lists(a1, a2, k)
    assert list(nin) == [130, 443, 0, big, 257, 0, 5, 0] and list(nout) == [443, 130, big, 257, 0, 131, 0, 5]
    for v in (443, 130, big, 257, 131):
        assert 128 <= v <= min(1024, cap) and v % 4 and v % groups, (v, cap, groups)
    seq.append(("mid", a1, a2))

    # 3. long lists, 1025..cap rows: the bitonic sort of the direct path (only where the capacity leaves room)
    a3 = a2
    if cap >= 2048:
        a3 = _moved(rs, a2, [(1, 0, 1025), (3, 2, cap), (4, 5, 1500)])
        nin, nout = _lists(a2, a3, k)
        assert list(nin) == [1025, 0, cap, 0, 0, 1500, 0, 0] and list(nout) == [0, 1025, 0, cap, 1500, 0, 0, 0]
        assert all(1024 < v <= cap for v in (1025, cap, 1500))
        seq.append(("long", a2, a3))
    else:
        assert cap == 512 and d == 1032   # the narrow layouts all have the bitonic branch

    # 4. beyond the capacity: the overflow rebuild from (prev, cur), four overflowing buckets in one call -- one of
    #    them by a single row -- beside a short pair; cluster 6 loses every row
    sizes = numpy.bincount(a3[(a3 >= 0) & (a3 < k)], minlength=k)
    src = max((0, 1, 4, 5), key=lambda c: sizes[c])
    dst = src ^ 1
    a4 = _moved(rs, a3, [(6, 7, None), (src, dst, cap + 1), (2, 3, 9)])
    nin, nout = _lists(a3, a4, k)
    assert nout[6] == sizes[6] > cap and nin[7] == sizes[6] and nout[src] == cap + 1 == nin[dst]
    assert nin[3] == 9 == nout[2] and nin.sum() == nout.sum() == sizes[6] + cap + 1 + 9
    seq.append(("overflow", a3, a4))

    # 5., 6. small calls behind the big one (auto: the host's stale counts pick the path, as in the unweighted test)
    a5 = _moved(rs, a4, [(0, 2, 37), (1, 3, 41), (7, 6, 3)])
    seq.append(("after-37-41-3", a4, a5))
    a6 = _moved(rs, a5, [(4, 0, 60)])
    seq.append(("after-60", a5, a6))
    return seq


def _reference(x, w, prev, cur, k):
    """float64: delta = sum_in(w x) - sum_out(w x), the count change, sum_in(w) - sum_out(w) per centroid, and the
    weight of the rows that joined a cluster.  Exact for these inputs whatever order numpy adds in."""
    wx = w.astype(numpy.float64)[:, None] * x.astype(numpy.float64)
    w64 = w.astype(numpy.float64)
    moved = prev != cur
    ein = moved & (cur >= 0) & (cur < k)
    eout = moved & (prev >= 0) & (prev < k)
    delta = numpy.zeros((k, x.shape[1]), numpy.float64)
    dcount = numpy.zeros(k, numpy.int64)
    dweight = numpy.zeros(k, numpy.float64)
    for c in range(k):
        i, o = ein & (cur == c), eout & (prev == c)
        delta[c] = wx[i].sum(0) - wx[o].sum(0)
        dcount[c] = int(i.sum()) - int(o.sum())
        dweight[c] = w64[i].sum() - w64[o].sum()
    return delta, dcount, dweight, w64[ein].sum()


_CASES = {}    # (layout, weights) -> inputs, sequence and float64 references, computed once
_RECORD = {}   # (layout, weights, call pair) -> the first mode's buffers: every other mode must reproduce them


def _case(layout, weights):
    key = (layout, weights)
    if key not in _CASES:
        n, d, k, offset, vec4, cap = _LAYOUTS[layout]
        assert bucket_cap(n, k) == cap
        rs = numpy.random.RandomState(len(layout) * 31 + d)
        x = exact_rows(rs, n, d)
        w = exact_weights(rs, n) if weights == "drawn" else index_weights(n)
        seq = _sequence(n, d, k, vec4)
        _CASES[key] = (x, w, seq, [_reference(x, w, p, c, k) for _, p, c in seq])
    return _CASES[key]


def _upload_rows(x, offset, dev):
    """The rows on the device: contiguous, or in a view one float past a 16-byte boundary."""
    if not offset:
        xs = torch.from_numpy(x).to(dev)
        assert xs.data_ptr() % 16 == 0
        return xs, xs
    n, d = x.shape
    store = torch.zeros(n * d + 4, dtype=torch.float32, device=dev)
    xs = store[1:1 + n * d].view(n, d)
    xs.copy_(torch.from_numpy(x).to(dev))
    assert xs.data_ptr() % 16 == 4 and xs.is_contiguous()
    return xs, store


def _same_bits(got, want, what):
    got, want = numpy.ascontiguousarray(got, numpy.float64), numpy.ascontiguousarray(want, numpy.float64)
    assert got.shape == want.shape, what
    bad = numpy.argwhere(got.view(numpy.uint64) != want.view(numpy.uint64))
    if len(bad):
        at = tuple(bad[0])
        raise AssertionError("%s: %d of %d words differ, first at %s: got %r, float64 reference %r"
                             % (what, len(bad), got.size, at, got[at], want[at]))


@pytest.mark.parametrize("weights", ["drawn", "index13"])
@pytest.mark.parametrize("layout", sorted(_LAYOUTS))
@pytest.mark.parametrize("mode", ["auto", "sync", "bucket", "radix"])
def test_weighted_move_sums(mode, layout, weights):
    """Engine.set_weights, set_update_mode, then the synthetic sequence -- once through reduce_fill (the tail is
    visible) and once through move_deltas, each on a fresh engine.  After every call: delta, the count change, the
    K + 1 weight words and the four counter words against the float64 reference, bit for bit; the sequence of buffers
    bit-identical across the four modes.  bucket: always the direct path (rank sort, bitonic sort, overflow rebuild);
    radix: always the sorted path; auto and sync: whichever the host's figures pick.  weights: drawn per row (j 2^e),
    or 2^((i % 13) - 6) by row index."""
    from kmcuda_amd.engine import Engine
    n, d, k, offset, vec4, cap = _LAYOUTS[layout]
    x, w, seq, refs = _case(layout, weights)
    dev = torch.device("cuda", 0)
    xs, _keep = _upload_rows(x, offset, dev)
    assert ((d % 4 == 0) and xs.data_ptr() % 16 == 0) == vec4
    ws = torch.from_numpy(w).to(dev)
    kd = k * d
    for via in ("fill", "deltas"):
        eng = Engine(n, d, k, "L2", device=0)
        eng.set_weights(ws)
        eng.set_update_mode(mode)
        assert eng.reduce_len() == kd + k + 4 + k + 1
        if not offset:
            # one assignment pass first: the counter words the tail copies are then not all zero
            asg = torch.full((n,), -1, dtype=torch.int32, device=dev)
            prv = torch.full((n,), -1, dtype=torch.int32, device=dev)
            eng.reset_counters()
            eng.lloyd_assign(xs, xs[:k].clone(), asg, prv)
            eng.sync()
            assert eng.counters()[0] == n
        counters = eng.counters()
        buf = torch.zeros(eng.reduce_len(), dtype=torch.float64, device=dev)
        delta = torch.zeros(kd, dtype=torch.float64, device=dev)
        dcount = torch.zeros(k, dtype=torch.int32, device=dev)
        record = []
        for (name, prev, cur), (want, wcount, wweight, wjoined) in zip(seq, refs):
            what = "%s, %s, call %r" % (mode, via, name)
            pt, ct = torch.from_numpy(prev).to(dev), torch.from_numpy(cur).to(dev)
            if via == "fill":
                buf.fill_(float("nan"))          # a word the kernel leaves out stays NaN
                eng.reduce_fill(xs, pt, ct, buf)
                eng.sync()
                got = buf.cpu().numpy().copy()
                _same_bits(got[:kd].reshape(k, d), want, what + ": delta")
                assert (got[kd:kd + k] == wcount).all(), what
                assert list(got[kd + k:kd + k + 4]) == counters, what   # where the unweighted layout has them
                _same_bits(got[kd + k + 4:kd + k + 4 + k], wweight, what + ": dweight")
                _same_bits(got[-1:], numpy.array([wjoined]), what + ": weight of the rows that joined")
            else:
                delta.fill_(float("nan"))
                dcount.fill_(-12345)
                eng.move_deltas(xs, pt, ct, delta, dcount)
                eng.sync()
                got = delta.cpu().numpy().copy()
                _same_bits(got.reshape(k, d), want, what + ": delta")
                assert (dcount.cpu().numpy() == wcount).all(), what
            record.append(got)
        eng.close()
        first = _RECORD.setdefault((layout, weights, via), record)
        for i, (a, b) in enumerate(zip(first, record)):
            assert a.tobytes() == b.tobytes(), "%s call %d differs between update modes" % (via, i)


@pytest.mark.parametrize("layout", ["d24-vec4", "d30-scalar"])
@pytest.mark.parametrize("mode", ["bucket", "radix"])
def test_unset_weights_leave_no_trace(mode, layout):
    """set_weights(w), one weighted call, set_weights(None): the next move_deltas and reduce_fill reproduce, bit for
    bit, those of an engine that never had weights (and the float64 sums of the plain rows, exact as well)."""
    from kmcuda_amd.engine import Engine
    n, d, k, offset, vec4, cap = _LAYOUTS[layout]
    x, w, seq, refs = _case(layout, "drawn")
    dev = torch.device("cuda", 0)
    xs = torch.from_numpy(x).to(dev)
    ws = torch.from_numpy(w).to(dev)
    kd = k * d
    ones = numpy.ones(n, numpy.float32)
    out = []
    for weighted_first in (True, False):
        eng = Engine(n, d, k, "L2", device=0)
        eng.set_update_mode(mode)
        plain_len = eng.reduce_len()
        assert plain_len == kd + k + 4
        delta = torch.zeros(kd, dtype=torch.float64, device=dev)
        dcount = torch.zeros(k, dtype=torch.int32, device=dev)
        if weighted_first:
            eng.set_weights(ws)
            _, prev, cur = seq[1]
            eng.move_deltas(xs, torch.from_numpy(prev).to(dev), torch.from_numpy(cur).to(dev), delta, dcount)
            eng.sync()
            _same_bits(delta.cpu().numpy().reshape(k, d), refs[1][0], "weighted call")
            eng.set_weights(None)
            assert eng.reduce_len() == plain_len
        got = []
        for name, prev, cur in seq[2:5]:
            pt, ct = torch.from_numpy(prev).to(dev), torch.from_numpy(cur).to(dev)
            delta.fill_(float("nan"))
            eng.move_deltas(xs, pt, ct, delta, dcount)
            buf = torch.full((plain_len,), float("nan"), dtype=torch.float64, device=dev)
            eng.reduce_fill(xs, pt, ct, buf)
            eng.sync()
            want, wcount, _, _ = _reference(x, ones, prev, cur, k)
            _same_bits(delta.cpu().numpy().reshape(k, d), want, "unweighted again, call %r" % name)
            assert (dcount.cpu().numpy() == wcount).all()
            got.append((delta.cpu().numpy().copy(), buf.cpu().numpy().copy()))
        eng.close()
        out.append(got)
    for (da, ba), (db, bb) in zip(*out):
        assert da.tobytes() == db.tobytes() and ba.tobytes() == bb.tobytes()


# ------------------------------------------------------------------------------------------------------------------
# the weighted apply from known state
# ------------------------------------------------------------------------------------------------------------------
_APPLY = {}


def _apply_case(metric):
    """n = 6000 rows, K = 6 centroids of 1000 rows each, then four steps in which every surviving cluster keeps at least
    half its weight (asserted by the test); step 2 empties cluster 2 by count and nothing refills it."""
    if metric not in _APPLY:
        from test_gpu_weighted import _log_uniform
        n, d, k = 6000, 30, 6
        rs = numpy.random.RandomState(77)
        if metric == "L2":
            x, w = exact_rows(rs, n, d), exact_weights(rs, n)
        else:   # unit-length rows are not exactly summable: the existing file's log-uniform weights
            x = rs.rand(n, d).astype(numpy.float32)
            x /= numpy.linalg.norm(x, axis=1, keepdims=True)
            w = _log_uniform(rs, n)
        none = numpy.full(n, NONE, numpy.int32)
        a0 = rs.permutation(numpy.arange(n, dtype=numpy.int32) % k).astype(numpy.int32)
        a1 = _moved(rs, a0, [(0, 1, 300), (1, 2, 200), (3, k, 100), (4, 0, 350)])
        a2 = _moved(rs, a1, [(2, 3, None), (0, 4, 100)])
        a3 = _moved(rs, a2, [(1, 0, 150), (3, 5, 400)])
        a4 = _moved(rs, a3, [(5, 1, 200)])
        _APPLY[metric] = (x, w, [(none, a0), (a0, a1), (a1, a2), (a2, a3), (a3, a4)])
    return _APPLY[metric]


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("metric", ["L2", "cos"])
def test_weighted_apply_from_known_state(metric, fused):
    """(move_deltas, apply_delta) and (reduce_fill, reduce_apply) over synthetic steps, against the restatement of
    tests/test_gpu_weighted.py: (c W_old + delta) / W_new (L2) or the normalised vector (angular) in float64, from the
    GPU's own fp32 centroids of the step before and the exact float64 cluster weights.

    Bound: the fp64 evaluation differs from the kernel's by fp64 roundings only (~1e-16 relative, at most doubled by
    the subtraction because every surviving cluster keeps at least half its weight -- asserted), and the result, a
    positive value, is rounded ONCE to fp32: relative error <= 2^-23 (half an ulp is 2^-24; the other half covers the
    fp64 residue).  Step 2 empties cluster 2 by count: its centroid is NaN from then on, its running weight 0 -- the
    later steps' dweight for it is exactly 0 and the surviving clusters' centroids, which divide by their own running
    weights, keep the bound."""
    from kmcuda_amd.engine import Engine
    from test_gpu_weighted import _restate
    x, w, steps = _apply_case(metric)
    n, d = x.shape
    k, kd = 6, 6 * d
    x64, w64 = x.astype(numpy.float64), w.astype(numpy.float64)
    dev = torch.device("cuda", 0)
    xs, ws = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    eng = Engine(n, d, k, metric, device=0)
    eng.set_weights(ws)
    cen = torch.from_numpy(x[:k].copy()).to(dev)
    ccounts = torch.zeros(k, dtype=torch.int32, device=dev)
    buf = torch.zeros(eng.reduce_len(), dtype=torch.float64, device=dev)
    delta = torch.zeros(kd, dtype=torch.float64, device=dev)
    dcount = torch.zeros(k, dtype=torch.int32, device=dev)
    cw = numpy.zeros(k)
    emptied = False
    for step, (prev, cur) in enumerate(steps):
        c_before = cen.cpu().numpy()
        pt, ct = torch.from_numpy(prev).to(dev), torch.from_numpy(cur).to(dev)
        if fused:
            buf.fill_(float("nan"))
            eng.reduce_fill(xs, pt, ct, buf)
            eng.reduce_apply(buf, cen, ccounts)
        else:
            eng.move_deltas(xs, pt, ct, delta, dcount)
            eng.apply_delta(delta, dcount, cen, ccounts)
        eng.sync()
        members = (cur >= 0) & (cur < k)
        counts = numpy.bincount(cur[members], minlength=k)
        wsum = numpy.bincount(cur[members], weights=w64[members], minlength=k)
        assert (ccounts.cpu().numpy() == counts).all()
        left = (prev != cur) & (prev >= 0) & (prev < k)
        w_out = numpy.bincount(prev[left], weights=w64[left], minlength=k)
        live = counts > 0
        assert (w_out[live] <= cw[live] / 2).all(), "a surviving cluster lost more than half its weight"
        with numpy.errstate(invalid="ignore", divide="ignore"):
            ref, w_new = _restate(metric, c_before, cw, x64, w64, prev.view(numpy.uint32), cur.view(numpy.uint32), k)
        got = cen.cpu().numpy().astype(numpy.float64)
        if step >= 2:
            emptied = True
            assert not live[2] and live.sum() == k - 1
            assert numpy.isnan(got[2]).all()                  # by COUNT, whatever residue the weight would have
        else:
            assert live.all()
        err = numpy.abs(got[live] - ref[live]) / numpy.abs(ref[live])
        print("%s step %d: max relative error against the float64 restatement %.3g (bound %.3g)"
              % (metric, step, err.max(), U))
        assert err.max() <= U
        if metric == "L2":
            assert (w_new[live] == wsum[live]).all()          # exact weights: the running weights are exact
        else:
            numpy.testing.assert_allclose(w_new[live], wsum[live], rtol=1e-12)
        if fused:
            tail = buf.cpu().numpy()
            dw = wsum - cw
            if metric == "L2":
                _same_bits(tail[kd + k + 4:kd + k + 4 + k][live], dw[live], "dweight, step %d" % step)
                if step == 2:
                    assert tail[kd + k + 4 + 2] == -cw[2]     # the emptied cluster gives back exactly what it had
            else:   # two float64 sums of at most n positive terms each: 1e-12 of their magnitudes covers both orders
                joined = (prev != cur) & members
                w_in = numpy.bincount(cur[joined], weights=w64[joined], minlength=k)
                assert (numpy.abs(tail[kd + k + 4:kd + k + 4 + k] - (w_in - w_out)) <= 1e-12 * (w_in + w_out)).all()
            if step > 2:
                assert tail[kd + k + 4 + 2] == 0.0 and tail[kd + 2] == 0.0   # no event: no weight, no count
        cw = wsum.copy()
        if emptied:
            cw[2] = 0.0
    assert emptied
    eng.close()
