"""Batched K-means (kmeans_batched, kmeans_predict_batched) against the CPU oracle, slice by slice:
for every problem the assignments are oracle.lloyd_assign's on that problem's N x D slice bit for bit, the distances
oracle.distance's, and the update is the float64 mean of the members rounded to fp32."""
import numpy
import pytest

import oracle
from kmcuda_amd import kmeans_batched, kmeans_predict_batched
from kmcuda_amd.batched import max_clusters

pytestmark = pytest.mark.gpu
U32 = numpy.uint32


def _columns(x):
    """(B, N, D) -> the (N, B * D) layout: problem b in the column block [b * D, (b + 1) * D)."""
    return numpy.ascontiguousarray(x.transpose(1, 0, 2)).reshape(x.shape[1], -1)


def _slice_reference(x, c):
    """Per problem: oracle.lloyd_assign on the slice (k for a NaN row) and oracle.distance to that centroid."""
    k = c.shape[1]
    asg = numpy.stack([oracle.lloyd_assign(x[b], c[b])[0] for b in range(len(x))])
    dist = numpy.array([[oracle.distance(x[b, i], c[b, a]) if a < k else numpy.nan for i, a in enumerate(asg[b])]
                        for b in range(len(x))], numpy.float32).reshape(asg.shape)
    return asg, dist


def _means(x, asg, c):
    """The float64 mean of every cluster's members rounded to fp32; a cluster without members keeps c's bits."""
    out = c.copy()
    for j in range(len(c)):
        if (asg == j).any():
            out[j] = x[asg == j].astype(numpy.float64).mean(axis=0).astype(numpy.float32)
    return out


def _within_one_ulp(got, ref):
    # a cluster's sum: fp64 additions of at most N fp32 values (relative error <= N 2^-53, far below half an fp32
    # place), one fp64 division and ONE rounding to fp32: at most one last place from the float64 mean's rounding
    return (numpy.abs(got.astype(numpy.float64) - ref) <= numpy.spacing(numpy.abs(ref))).all()


@pytest.mark.parametrize("n,b", [(1, 1), (255, 3), (256, 1), (257, 3), (1000, 3)])
@pytest.mark.parametrize("k", [1, 2, 255, 256, "max"])
@pytest.mark.parametrize("d", [1, 3, 4, 8, 12, 16, 17, 32, 64])
def test_one_assignment_pass_is_the_oracles_on_every_slice(d, k, n, b):
    k = max_clusters(d) if k == "max" else k
    rs = numpy.random.default_rng(1000 * d + k + n)
    x = rs.standard_normal((b, n, d)).astype(numpy.float32)
    c = rs.standard_normal((b, k, d)).astype(numpy.float32)
    c[:, :min(k, n):3] = x[:, :min(k, n):3]           # centroids that are rows: distances of exactly zero
    if k >= 3:
        c[:, 0] = numpy.round(c[:, 0] * 8) / 8        # (eighths: the steps of 1 and 2 below are exact)
        c[:, 1] = c[:, 0]                             # two identical centroids: the lower index wins
        c[:, 2] = c[:, 0]
        c[:, 2, 0] += 2
        if n >= 3:
            x[:, 1] = c[:, 0]
            x[:, 1, 0] += 1                           # a row half way between centroids 0 (= 1) and 2
    if n >= 3:
        x[:, 2, 0] = numpy.nan                        # no cluster: k
    ref, ref_dist = _slice_reference(x, c)
    asg, dist = kmeans_predict_batched(x, c, return_distances=True)
    assert asg.dtype == U32 and (asg == ref).all()
    assert (dist.view(U32) == ref_dist.view(U32)).all()
    if n >= 3:
        assert (asg[:, 2] == k).all() and numpy.isnan(dist[:, 2]).all()
    asg_c, dist_c = kmeans_predict_batched(_columns(x), c, layout="columns", return_distances=True)
    assert (asg_c.T == ref).all() and (dist_c.T.view(U32) == ref_dist.view(U32)).all()
    if k <= 256:
        codes = kmeans_predict_batched(_columns(x), c, layout="columns", dtype=numpy.uint8)
        assert codes.dtype == numpy.uint8 and (codes.T == (ref & 0xFF).astype(numpy.uint8)).all()


@pytest.mark.parametrize("layout", ["problems", "columns"])
@pytest.mark.parametrize("d,integers", [(3, False), (16, False), (33, False), (8, True)])
def test_one_full_iteration_moves_to_the_float64_means(d, integers, layout):
    b, n, k = 2, 700, 6
    rs = numpy.random.default_rng(d)
    x = rs.integers(-8, 9, (b, n, d)).astype(numpy.float32) if integers else \
        rs.standard_normal((b, n, d)).astype(numpy.float32)
    init = x[:, :k].copy()
    init[:, k - 1] = 1000.0                            # nobody's nearest: it keeps its bits
    cen, asg, its = kmeans_batched(_columns(x) if layout == "columns" else x, k, init=init, max_iter=1,
                                   layout=layout, problems=b)
    asg = asg.T if layout == "columns" else asg
    assert (its == 1).all()
    for p in range(b):
        ref_asg = oracle.lloyd_assign(x[p], init[p])[0]
        assert (asg[p] == ref_asg).all()
        ref = _means(x[p], ref_asg, init[p])
        assert cen[p, k - 1].tobytes() == init[p, k - 1].tobytes()
        if integers:   # every sum is exact in fp64: the same quotient, the same rounding
            assert cen[p].tobytes() == ref.tobytes()
        else:
            assert _within_one_ulp(cen[p], ref)


@pytest.mark.parametrize("d", [4, 64])
def test_the_largest_panel_runs_a_full_iteration(d):
    k, n = max_clusters(d), 5000                       # the update's fp64 cells at the LDS bound
    x = numpy.random.default_rng(d).integers(-8, 9, (1, n, d)).astype(numpy.float32)
    init = x[:, :k] + numpy.float32(0.25)
    cen, asg, _ = kmeans_batched(x, k, init=init, max_iter=1)
    ref_asg = oracle.lloyd_assign(x[0], init[0])[0]
    assert (asg[0] == ref_asg).all() and cen[0].tobytes() == _means(x[0], ref_asg, init[0]).tobytes()


def _blobs(d=6, n=900, k=5):
    """Three problems of k well-separated blobs (spacing 20, noise 0.5: a last-place difference of a centroid moves
    no row across a boundary) from different starts: the blob centres, the first k rows, k shifted rows."""
    rs = numpy.random.default_rng(11)
    centres = (20 * rs.permutation(k * d).reshape(k, d) % 100).astype(numpy.float32)
    x = numpy.stack([centres[rs.integers(0, k, n)] + 0.5 * rs.standard_normal((n, d)).astype(numpy.float32)
                     for _ in range(3)]).astype(numpy.float32)
    init = numpy.stack([centres, x[1, :k], x[2, ::n // k][:k] + 3])
    return x, init.astype(numpy.float32)


def test_whole_runs_stop_per_problem_and_follow_the_plain_loop():
    x, init = _blobs()
    k = init.shape[1]
    cen, asg, its = kmeans_batched(x, k, init=init, max_iter=50, tolerance=0.0)
    assert len(set(its.tolist())) > 1 and its.max() < 50
    for p in range(3):
        c, a, changed = init[p], numpy.full(x.shape[1], -1), []
        for _ in range(int(its[p])):                   # the plain loop of that problem alone, as many passes
            prev, a = a, oracle.lloyd_assign(x[p], c)[0]
            changed.append(int((a != prev).sum()))
            c = _means(x[p], a, c)
        assert changed[-1] == 0 and all(changed[:-1])  # ... it stops there too, and not earlier
        assert (asg[p] == a).all() and _within_one_ulp(cen[p], c)
    again = kmeans_batched(x, k, init=init, max_iter=50, tolerance=0.0)
    assert all(u.tobytes() == v.tobytes() for u, v in zip((cen, asg, its), again))
    cols = kmeans_batched(_columns(x), k, init=init, max_iter=50, tolerance=0.0, layout="columns")
    assert cols[0].tobytes() == cen.tobytes() and (cols[1].T == asg).all() and (cols[2] == its).all()


def _hash_draw(seed, r, s):
    m = (1 << 64) - 1
    z = (((r << 32) | s) + (seed + 1) * 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


@pytest.mark.parametrize("n,k", [(900, 5), (40, 40)])
def test_random_init_is_the_hash_draw(n, k):
    x, _ = _blobs(n=n)
    picks = []
    for p in range(3):                                 # the first draws t = 0, 1, ... that give k distinct rows
        rows, t = [], 0
        while len(rows) < k:
            row = (_hash_draw(9, p, t) * n) >> 64
            rows += [row] if row not in rows else []
            t += 1
        picks.append(x[p, rows])
    got = kmeans_batched(x, k, init="random", seed=9, max_iter=3)
    want = kmeans_batched(x, k, init=numpy.stack(picks), max_iter=3)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(got, want))


def test_device_tensors_in_device_tensors_out_with_the_same_bits():
    import torch
    x, init = _blobs()
    dev = torch.device("cuda", 0)
    xc = torch.from_numpy(_columns(x)).to(dev)
    host = kmeans_batched(_columns(x), init.shape[1], init=init, max_iter=50, layout="columns")
    got = kmeans_batched(xc, init.shape[1], init=torch.from_numpy(init).to(dev), max_iter=50, layout="columns")
    assert all(t.is_cuda for t in got)
    assert all(t.cpu().numpy().tobytes() == h.tobytes() for t, h in zip(got, host))
    asg, dist = kmeans_predict_batched(xc, got[0], layout="columns", return_distances=True)
    h_asg, h_dist = kmeans_predict_batched(_columns(x), host[0], layout="columns", return_distances=True)
    assert asg.is_cuda and dist.is_cuda
    assert asg.cpu().numpy().tobytes() == h_asg.tobytes() and dist.cpu().numpy().tobytes() == h_dist.tobytes()
    assert (asg.cpu().numpy().view(U32) == host[1]).all()   # the run's last pass moved nothing
