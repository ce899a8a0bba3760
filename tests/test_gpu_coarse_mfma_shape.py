"""Stage 1 of the default Lloyd filter on either MFMA shape (kmcuda_amd/csrc/lloyd_coarse.hpp, SHAPE: 16x16x32 by
default where it applies, KMCUDA_AMD_COARSE_MFMA=32 for 32x32x16 everywhere; reference: the assignment of
src/kmeans.cu:293-364 that every path must reproduce).

The two shapes differ in which lane holds which score, how the packed index decodes to a centroid and which scores
form the four quarters the duo list is built from.  Whatever the shape: assignments, previous assignments and the
reassignment counter are the oracle's, bit for bit -- at every padded width (16 and 512 keep 32x32x16 under either
setting), with rows as fp32 or halves, with and without the row cache, in plain and carried passes, with the duo list
off and always on.  Near-tie rows send most rows through the undecided / duo paths; duplicate centroids put exact ties
between lane groups, half tiles and tiles (the lowest index wins)."""
import numpy
import pytest

import oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SHAPES = ["16", "32"]


def _assign(x, c, cached=False, half=False):
    from kmcuda_amd.engine import Engine
    dev = torch.device("cuda", 0)
    n, d = x.shape
    xs = torch.from_numpy(x).to(dev)
    cs = torch.from_numpy(c.astype(numpy.float32)).to(dev)
    asg = torch.full((n,), -1, dtype=torch.int32, device=dev)
    prev = torch.full((n,), -1, dtype=torch.int32, device=dev)
    eng = Engine(n, d, c.shape[0], "L2", device=0)
    h = None
    if half:
        h = xs.to(torch.float16)
        eng.set_half_rows(h)
    if cached:
        eng.set_row_cache(True)
    eng.lloyd_assign(xs, cs, asg, prev)
    counters = eng.counters()
    eng.close()
    return asg.cpu().numpy().view(numpy.uint32), prev.cpu().numpy().view(numpy.uint32), counters


def _near_ties(rs, n, d, k, spread):
    """Rows between pairs of centroids: most rows have exactly two contenders."""
    c = rs.rand(k, d).astype(numpy.float32)
    a, b = rs.randint(0, k, n), rs.randint(0, k, n)
    t = (0.5 + spread * rs.randn(n, 1)).astype(numpy.float32)
    x = (t * c[a] + (1 - t) * c[b] + 1e-3 * rs.randn(n, d)).astype(numpy.float32)
    return x, c


def _check(x, c, cached, half):
    if half:
        x = x.astype(numpy.float16).astype(numpy.float32)
    got, prev, counters = _assign(x, c, cached=cached, half=half)
    ref, ref_prev, ref_changed = oracle.lloyd_assign(x, c)
    bad = numpy.nonzero(got != ref)[0]
    assert bad.size == 0, (bad[:10], got[bad[:10]], ref[bad[:10]])
    assert (prev == ref_prev).all()
    assert counters[0] == ref_changed


# (d, k): padded widths 16, 32, 64, 128 (100: not a multiple of 16), 256, 512 (300); K not a multiple of 32
@pytest.mark.parametrize("duo", ["0", "2"])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("cached", [False, True])
@pytest.mark.parametrize("d,k", [(16, 45), (32, 130), (64, 77), (100, 257), (256, 96), (300, 70)])
@pytest.mark.parametrize("shape", SHAPES)
def test_near_ties_equal_the_oracle(shape, d, k, cached, half, duo, monkeypatch):
    monkeypatch.setenv("KMCUDA_AMD_COARSE_MFMA", shape)
    monkeypatch.setenv("KMCUDA_AMD_DUO", duo)
    rs = numpy.random.RandomState(d + k)
    n = 3001   # (not a multiple of the 256 rows of a block)
    x, c = _near_ties(rs, n, d, k, 1e-4)
    x[5] = numpy.nan                      # kmeans.cu:312
    x[17, 3 % d] = numpy.inf
    _check(x, c, cached, half)


@pytest.mark.parametrize("cached", [False, True])
@pytest.mark.parametrize("d", [32, 256])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_tile_position_and_ties_across_lane_groups(shape, d, cached, monkeypatch):
    """Rows at every centroid of K = 77 (every one of the 32 positions of a tile wins somewhere, the last tile is
    partial), and exact ties: centroid a duplicated at a + 1 (same lane group), a + 4 (next lane group), a + 16 (other
    half tile) and a + 32 (next tile) -- the lowest index wins."""
    monkeypatch.setenv("KMCUDA_AMD_COARSE_MFMA", shape)
    monkeypatch.setenv("KMCUDA_AMD_DUO", "2")
    rs = numpy.random.RandomState(d)
    k = 77
    c = rs.rand(k, d).astype(numpy.float32)
    for a, off in ((2, 1), (9, 4), (20, 16), (5, 32), (40, 4), (44, 16), (64, 4)):
        c[a + off] = c[a]
    lab = numpy.repeat(numpy.arange(k), 40)
    x = (c[lab] + 1e-3 * rs.randn(len(lab), d)).astype(numpy.float32)
    # and rows half way between two centroids of different lane groups / half tiles
    a, b = rs.randint(0, k, 1500), rs.randint(0, k, 1500)
    x = numpy.concatenate([x, (0.5 * (c[a] + c[b]) + 1e-5 * rs.randn(1500, d)).astype(numpy.float32)])
    _check(x, c, cached, False)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("shape", SHAPES)
def test_carried_passes(shape, d, half, monkeypatch):
    """Bounds carried from pass to pass (every row, then the listed rows): states equal to plain passes and to the
    oracle's replay of every pass (test_gpu_carry._run_pair)."""
    monkeypatch.setenv("KMCUDA_AMD_COARSE_MFMA", shape)
    from test_gpu_carry import _run_pair
    rs = numpy.random.RandomState(d + 3)
    cen = rs.rand(24, d) * 6.0
    x = (cen[rs.randint(0, 24, 20000)] + rs.randn(20000, d)).astype(numpy.float32)
    _run_pair(x, 40, iters=8, carry_from=2, fused=False, half=half, list_max=1.0)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("d", [12, 32, 128, 256])
@pytest.mark.parametrize("shape", SHAPES)
def test_angular_near_ties(shape, d, half, monkeypatch):
    """The angular metric, plain and row-cache passes, duo list always on: products at 1 with a centroid and its
    duplicate at a lower index (the lowest index wins) among rows between two centroids."""
    monkeypatch.setenv("KMCUDA_AMD_COARSE_MFMA", shape)
    monkeypatch.setenv("KMCUDA_AMD_DUO", "2")
    from test_gpu_angular_clamp import _check as _check_cos
    rs = numpy.random.RandomState(d + 7 * half)
    x, c = _near_ties(rs, 4000, d, 90, 1e-3)
    x /= numpy.linalg.norm(x, axis=1, keepdims=True)
    c /= numpy.linalg.norm(c, axis=1, keepdims=True)
    x[100:140] = c[7]
    c[3] = c[7]
    if half:
        x = x.astype(numpy.float16).astype(numpy.float32)
    for variant in ("f16", "f16-cached"):
        _check_cos(x, [c], variant, half, monkeypatch, exact_rows=numpy.arange(100, 140))
