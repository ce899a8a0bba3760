"""The multi-probe search's definition on the CPU: tests/_probe_ref.probe_reference against a float64
brute force over the probed rows, against the unrestricted oracle at p = K, its filler tail, the entries a probe list
may carry without changing anything -- and the argument checks of knn_query(nprobe=, probes=), which all happen before
the device is touched (no GPU here)."""
import numpy
import pytest

import oracle
from _probe_ref import FLT_MAX, NONE, probe_reference

K, D, N, Q = 12, 16, 600, 40


@pytest.fixture(scope="module")
def data():
    rng = numpy.random.default_rng(5)
    cent = (rng.normal(size=(K, D)) * 3).astype(numpy.float32)
    lab = rng.integers(0, K, N)
    x = (cent[lab] + rng.normal(size=(N, D))).astype(numpy.float32)
    a, _, _ = oracle.lloyd_assign(x, cent)
    q = (cent[rng.integers(0, K, Q)] + rng.normal(size=(Q, D))).astype(numpy.float32)
    d2 = ((q[:, None, :].astype(numpy.float64) - cent[None].astype(numpy.float64)) ** 2).sum(-1)
    order = numpy.argsort(d2, axis=1, kind="stable").astype(numpy.uint32)
    return x, cent, a.astype(numpy.uint32), q, order


def _brute(x, a, q, members, k):
    rows = numpy.nonzero(numpy.isin(a, members))[0]
    d = numpy.sqrt(((x[rows].astype(numpy.float64) - q.astype(numpy.float64)) ** 2).sum(-1))
    o = numpy.argsort(d, kind="stable")
    gaps = numpy.diff(d[o][:k + 1])
    # (the oracle's fp32 distances are off by less than 1e-6 relative)
    assert gaps.size == 0 or gaps.min() > 1e-6 * d[o][min(k, len(o) - 1)], "the data are not tie-free"
    return rows[o][:k]


@pytest.mark.parametrize("p", [1, 3, K])
def test_reference_is_brute_force_over_the_probed_rows(data, p):
    x, c, a, q, order = data
    k = 7
    probes = order[:, :p]
    nb, dist = probe_reference(k, x, c, a, q, probes)
    for i in range(Q):
        want = _brute(x, a, q[i], probes[i], k)
        filled = dist[i] < FLT_MAX
        assert filled.sum() == len(want), i
        assert (nb[i][filled] == want).all(), (i, nb[i], want)
        assert (nb[i][~filled] == 0).all()
        assert (numpy.diff(dist[i]) >= 0).all()


def test_all_clusters_probed_is_the_exact_query(data):
    x, c, a, q, order = data
    nb, dist = probe_reference(7, x, c, a, q, order)
    full_nb, full_dist = oracle.knn_query(7, x, c, a, q, query_assignments=order[:, 0].copy())
    assert (nb == full_nb).all()
    assert (dist.view(numpy.uint32) == full_dist.view(numpy.uint32)).all()


def test_filler_tail_when_k_exceeds_the_probed_rows(data):
    x, c, a, q, order = data
    k = 200
    probes = order[:, :2]
    nb, dist = probe_reference(k, x, c, a, q, probes)
    for i in range(Q):
        n = int(numpy.isin(a, probes[i]).sum())
        assert n < k
        assert (dist[i, :n] < FLT_MAX).all() and (dist[i, n:] == FLT_MAX).all() and (nb[i, n:] == 0).all()
        assert sorted(nb[i, :n]) == sorted(numpy.nonzero(numpy.isin(a, probes[i]))[0])


def test_fillers_duplicates_and_order_change_nothing(data):
    x, c, a, q, order = data
    base = order[:, :4]
    nb, dist = probe_reference(7, x, c, a, q, base)
    rng = numpy.random.default_rng(1)
    wide = numpy.full((Q, 9), K, numpy.uint32)
    wide[:, 0] = base[:, 0]
    for i in range(Q):
        tail = numpy.concatenate([base[i, 1:], base[i, 1:3], [base[i, 0]], [K]])   # 3 ids, 2 repeats, the own one, K
        wide[i, 1:1 + len(tail)] = rng.permutation(tail)
    nb2, dist2 = probe_reference(7, x, c, a, q, wide)
    assert (nb == nb2).all() and (dist.view(numpy.uint32) == dist2.view(numpy.uint32)).all()


def test_queries_without_a_list(data):
    x, c, a, q, order = data
    probes = order[:, :3].copy()
    probes[5] = K                       # the ranking found no centroid
    qq = q.copy()
    qq[9, 3] = numpy.nan
    nb, dist = probe_reference(7, x, c, a, qq, probes)
    for i in (5, 9):
        assert (nb[i] == NONE).all() and numpy.isnan(dist[i]).all()


# ---- knn_query's argument checks: every one of them before a device call -------------------------------------------
def _call(data, **kw):
    from kmcuda_amd import knn_query
    x, c, a, q, order = data
    return knn_query(5, x, c, a, q, device=10 ** 6, **kw)   # (a device that does not exist: reaching it is an error)


@pytest.mark.parametrize("kw,exc", [
    (dict(nprobe=0), ValueError),
    (dict(nprobe=65), ValueError),
    (dict(nprobe=K + 1), ValueError),
    (dict(nprobe=2.0), TypeError),
    (dict(nprobe=3, probes="width2"), ValueError),
    (dict(probes="1d"), ValueError),
    (dict(probes="float"), TypeError),
    (dict(probes="too_big"), ValueError),
    (dict(probes="column0_K"), ValueError),
    (dict(probes="rows"), ValueError),
    (dict(nprobe=2, query_assignments="qa"), ValueError),
    (dict(probes="ok", query_assignments="qa"), ValueError),
    (dict(return_probes=True), ValueError),
])
def test_arguments_are_refused_before_the_device(data, kw, exc):
    order = data[4]
    named = {
        "width2": order[:, :2], "1d": order[:, 0].copy(), "float": order[:, :2].astype(numpy.float32),
        "too_big": numpy.where(numpy.arange(2)[None] == 1, K + 1, order[:, :2]).astype(numpy.uint32),
        "column0_K": numpy.full((Q, 2), K, numpy.uint32), "rows": order[:-1, :2], "ok": order[:, :2],
        "qa": order[:, 0].copy(),
    }
    kw = {key: (named[v] if isinstance(v, str) else v) for key, v in kw.items()}
    with pytest.raises(exc) as info:
        _call(data, **kw)
    assert "unexpected keyword" not in str(info.value) and "No such" not in str(info.value), info.value


def test_half2_arithmetic_has_no_ranking(data, monkeypatch):
    """KMCUDA_AMD_FP16_STRICT with half rows: computed probes are refused (as kmeans_predict_top refuses the mode), and
    a caller's lists are not -- that call gets as far as the device."""
    from kmcuda_amd import knn_query
    x, c, a, q, order = data
    x, c, q = (v.astype(numpy.float16) for v in (x, c, q))
    monkeypatch.setenv("KMCUDA_AMD_FP16_STRICT", "1")
    with pytest.raises(ValueError, match="FP16_STRICT"):
        knn_query(5, x, c, a, q, device=10 ** 6, nprobe=3)
    with pytest.raises(ValueError, match="No such"):
        knn_query(5, x, c, a, q, device=10 ** 6, probes=order[:, :3])
