"""knn_cuda() at the edges where a filtered search goes wrong: data far from unit scale (half subnormals, the half
range and beyond it once centred, fp32 subnormal squared distances), NaN / inf rows and centroids, empty and one-row
clusters, cluster sizes around the kernels' tiles, assignments that are not the nearest centroid, k around the heap's
sizes and beyond N, K around the query-order key's 32 bits, and every KMCUDA_AMD_KNN_* switch.

One helper checks every case: the neighbour lists equal the CPU oracle's bit for bit (indices and order, the
all-UINT32_MAX rows of samples without a cluster and the oracle's index-0 filler slots when k >= N included); on finite
L2 inputs the j-th returned neighbour's float64 distance also equals the j-th smallest float64 distance (1e-5
relative), which the oracle and the kernels cannot both get wrong the same way; and where it matters the search that
actually ran is read back from what the library prints (the `k-NN filter:` statistics line of KMCUDA_AMD_KNN_STATS=1
exists only for the f16 matrix-core filter), so that a guard cannot pass by switching the filter off everywhere."""
import numpy
import pytest

import oracle
from _angular import assert_knn_only_acos_matters
from test_gpu_kmeans import StdoutListener

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NONE = 0xFFFFFFFF
F16 = "k-NN filter:"                                   # the f16 filter's statistics line (KMCUDA_AMD_KNN_STATS=1)
EXACT = "every candidate is evaluated with the exact arithmetic"
HALF_RANGE = "leaves the half range"


def _f64_check(x, a, K, k, nb, rows):
    """The float64 distances of the returned lists are the k smallest float64 distances, in order."""
    x64 = x.astype(numpy.float64)
    cand = numpy.nonzero(a < K)[0]
    for i in rows:
        d = numpy.sqrt(((x64[cand] - x64[i]) ** 2).sum(axis=1))
        d = d[cand != i]
        m = min(k, d.size)
        want = numpy.partition(d, m - 1)[:m] if m < d.size else d
        want = numpy.sort(want)[:m]
        got = numpy.sqrt(((x64[nb[i, :m].astype(numpy.int64)] - x64[i]) ** 2).sum(axis=1))
        assert numpy.allclose(got, want, rtol=1e-5, atol=0), (int(i), got, want)


def check(k, x, c, a, metric="L2", ptr="host", env=None, monkeypatch=None, expect=None, f64=None, rows=160, seed=0):
    """knn_cuda == oracle.knn bit for bit; float64 order check on finite L2 inputs; `expect` in
    {"f16", "f32", "exact", "half_range_f32", "half_range_exact"}: the search that must have run."""
    from kmcuda_amd import knn_cuda
    from kmcuda_amd.api import _DEVICE_ALLOCS, free_device_ptr
    for key, v in (env or {}).items():
        monkeypatch.setenv(key, str(v))
    if expect is not None:
        monkeypatch.setenv("KMCUDA_AMD_KNN_STATS", "1")
    a = numpy.ascontiguousarray(a, dtype=numpy.uint32)
    out = StdoutListener()
    with out:
        if ptr == "host":
            nb = knn_cuda(k, x, c, a, metric=metric, device=1, verbosity=1)
        else:
            assert x.dtype == numpy.float32
            dev = torch.device("cuda", 0)
            xs, cs = torch.from_numpy(x).to(dev), torch.from_numpy(c).to(dev)
            at = torch.from_numpy(a.view(numpy.int32)).to(dev)
            p = knn_cuda(k, (xs.data_ptr(), 0, x.shape), (cs.data_ptr(), len(c)), at.data_ptr(), metric=metric,
                         device=1, verbosity=1)
            nb = _DEVICE_ALLOCS[p].cpu().numpy().view(numpy.uint32)
            free_device_ptr(p)
    x32, c32 = x.astype(numpy.float32), c.astype(numpy.float32)
    ref, _ = oracle.knn(k, x32, c32, a, metric=metric)
    bad = numpy.nonzero((nb != ref).any(axis=1))[0]
    assert bad.size == 0, "%d rows differ from the oracle, first %d: %s vs %s" % (
        bad.size, bad[0], nb[bad[0]], ref[bad[0]])
    if expect is not None:
        text = out.text
        if expect == "f16":
            assert F16 in text and HALF_RANGE not in text, text
        elif expect in ("f32", "exact"):
            assert F16 not in text and HALF_RANGE not in text, text
        else:
            assert F16 not in text and HALF_RANGE in text, text
        if expect in ("exact", "half_range_exact"):
            assert EXACT in text, text
        elif expect != "f16":
            assert EXACT not in text, text
    if f64 is None:
        f64 = metric == "L2" and bool(numpy.isfinite(x32).all()) and bool(numpy.isfinite(c32).all())
    if f64:
        rs = numpy.random.RandomState(seed)
        sel = numpy.nonzero(a < len(c))[0]
        if sel.size > rows:
            sel = rs.choice(sel, rows, replace=False)
        _f64_check(x32, a, len(c), k, nb, sel)
    return nb, out.text


def blobs(n, d, K, scale, seed, offset=0.0, spread=0.15):
    """n rows in K Gaussian blobs of a cube of side `scale` (+ offset), the oracle's nearest-centroid assignments to
    the blob centres."""
    rs = numpy.random.RandomState(seed)
    centres = rs.rand(K, d) * scale + offset
    lab = rs.randint(0, K, n)
    x = (centres[lab] + rs.randn(n, d) * (spread * scale)).astype(numpy.float32)
    c = centres.astype(numpy.float32)
    a, _, _ = oracle.lloyd_assign(x, c)
    return x, c, a


# ----------------------------------------------------------------------------------------------------------------
# data range
# ----------------------------------------------------------------------------------------------------------------
RANGE = [(s, d, f) for s in (1e-6, 1.0, 6e4, 2e5) for d in (16, 64, 256, 512, 1024) for f in ("f16", "f32")
         if not (f == "f32" and d > 256)]


@pytest.mark.parametrize("scale,d,filt", RANGE)
def test_data_range(scale, d, filt, monkeypatch):
    n = 2500 if d <= 256 else 1200
    x, c, a = blobs(n, d, 24, scale, seed=d + int(numpy.log10(scale) * 7) + 100, spread=0.05)
    if scale == 6e4:
        assert numpy.abs(x - c.mean(axis=0)).max() < 65504   # just inside the half range once centred
    if scale == 2e5:
        assert numpy.abs(x - c.mean(axis=0)).max() > 65520   # beyond it
    expect = filt if scale < 1e5 or filt == "f32" else ("half_range_f32" if d <= 256 else "half_range_exact")
    check(10, x, c, a, env={"KMCUDA_AMD_FILTER": filt}, monkeypatch=monkeypatch, expect=expect, seed=d)


@pytest.mark.parametrize("d", [16, 64])
def test_uniform_beyond_the_half_range(d, monkeypatch):
    """Uniform rows at 2e5: true neighbours need not share the signs of their overflowing centred values (in blobs
    they do, and +inf scores still reach the exact chain), so hi.hi scores of neighbours come out NaN."""
    rs = numpy.random.RandomState(d)
    x = (rs.rand(3000, d) * 2e5).astype(numpy.float32)
    c = x[rs.choice(3000, 20, replace=False)].copy()
    a, _, _ = oracle.lloyd_assign(x, c)
    check(10, x, c, a, monkeypatch=monkeypatch, expect="half_range_f32", seed=d)


@pytest.mark.parametrize("filt", ["f16", "f32"])
def test_one_outlier_row(filt, monkeypatch):
    """A unit-scale corpus with ONE row at 1e6: that finite row alone takes the call off the f16 filter."""
    x, c, a = blobs(3000, 64, 30, 1.0, seed=31)
    x[1234] = 1e6
    a, _, _ = oracle.lloyd_assign(x, c)
    check(10, x, c, a, env={"KMCUDA_AMD_FILTER": filt}, monkeypatch=monkeypatch,
          expect="f32" if filt == "f32" else "half_range_f32")


@pytest.mark.parametrize("d", [64, 512])
def test_offset_rows(d, monkeypatch):
    """Unit spread at offset 1e4: the centred rows are unit-scale, the f16 filter stays on."""
    x, c, a = blobs(2500, d, 24, 1.0, seed=41, offset=1e4)
    check(10, x, c, a, monkeypatch=monkeypatch, expect="f16")


@pytest.mark.parametrize("d,skew", [(64, False), (64, True), (512, True)])
def test_fp16x2_across_the_half_range(d, skew, monkeypatch):
    """Half inputs spanning +-6e4.  Centred by the mean of the centroids, a value can reach twice 65504: with most
    centroids on one side (skew) the rows on the other leave the half range."""
    rs = numpy.random.RandomState(d + skew)
    n, K = 2400 if d == 64 else 1200, 20
    x = rs.uniform(-6e4, 6e4, (n, d))
    if skew:
        x[: int(0.9 * n)] = rs.uniform(3e4, 6e4, (int(0.9 * n), d))
    x16 = x.astype(numpy.float16)
    c16 = x16[rs.choice(int(0.9 * n) if skew else n, K, replace=False)].copy()
    a, _, _ = oracle.lloyd_assign(x16.astype(numpy.float32), c16.astype(numpy.float32))
    over = numpy.abs(x16.astype(numpy.float32) - c16.astype(numpy.float32).mean(axis=0)).max() >= 65520
    assert over or not skew
    expect = "f16" if not over else ("half_range_f32" if d <= 256 else "half_range_exact")
    check(10, x16, c16, a, monkeypatch=monkeypatch, expect=expect)


@pytest.mark.parametrize("filt", ["f16", "f32"])
def test_fp32_subnormal_squared_distances(filt, monkeypatch):
    """Rows at 1e-19: every squared difference is an fp32 subnormal (the slack of knn_centroid_bounds_kernel)."""
    x, c, a = blobs(2500, 16, 24, 1e-19, seed=51)
    assert (x - c[a]).max() ** 2 < 1.2e-38
    check(10, x, c, a, env={"KMCUDA_AMD_FILTER": filt}, monkeypatch=monkeypatch, expect=filt)


# ----------------------------------------------------------------------------------------------------------------
# non-finite and degenerate inputs
# ----------------------------------------------------------------------------------------------------------------
def degenerate(d, seed=61):
    """NaN rows (assignment K and 0xFFFFFFFF), one row with an inf feature, NaN centroids of empty clusters and one
    NaN centroid with members, an empty cluster with a finite centroid, a one-row cluster, duplicate rows in different
    clusters."""
    x, c, a = blobs(2000, d, 30, 1.0, seed=seed + d)
    rs = numpy.random.RandomState(seed)
    a = a.astype(numpy.uint32)
    nan_rows = rs.choice(2000, 12, replace=False)
    x[nan_rows] = numpy.nan
    a[nan_rows] = numpy.where(numpy.arange(12) % 3 == 0, NONE, 30).astype(numpy.uint32)
    rest = numpy.setdiff1d(numpy.arange(2000), nan_rows)
    x[rest[5], 3] = numpy.inf                      # one inf feature (its cluster keeps it)
    a[a == 4] = 9                                  # cluster 4: empty, NaN centroid
    c[4] = numpy.nan
    a[a == 5] = 10                                 # cluster 5: empty, finite centroid
    c[6, 0] = numpy.nan                            # cluster 6: NaN centroid with members
    one = numpy.nonzero(a == 7)[0]
    a[one[1:]] = 11                                # cluster 7: one row
    dup, twin = rest[100:110], rest[200:210]
    x[twin] = x[dup]                               # duplicates ...
    other = (a[dup] + 1) % 30                      # ... assigned to other clusters (not the empty or one-row ones)
    other[numpy.isin(other, [4, 5, 7])] = 12
    other[other == a[dup]] = 13
    a[twin] = other
    assert (a[twin] != a[dup]).all() and (a == 7).sum() == 1 and not numpy.isin(a, [4, 5]).any()
    return x, c, a


@pytest.mark.parametrize("ptr", ["host", "device"])
@pytest.mark.parametrize("path", ["f16", "f32", "exact_env", "exact_wide"])
def test_non_finite_and_degenerate(path, ptr, monkeypatch):
    d = 1100 if path == "exact_wide" else 64
    x, c, a = degenerate(d)
    env = {"f16": {}, "f32": {"KMCUDA_AMD_FILTER": "f32"}, "exact_env": {"KMCUDA_AMD_KNN_EXACT": 1},
           "exact_wide": {}}[path]
    expect = {"f16": "f16", "f32": "f32", "exact_env": "exact", "exact_wide": "exact"}[path]
    nb, _ = check(10, x, c, a, ptr=ptr, env=env, monkeypatch=monkeypatch, expect=expect)
    assert (nb[a >= 30] == NONE).all() and (a >= 30).sum() == 12


# ----------------------------------------------------------------------------------------------------------------
# shapes
# ----------------------------------------------------------------------------------------------------------------
def sized(sizes, d, seed, scale=1.0):
    """Clusters of exactly the given sizes (blobs), centroids = the blob centres."""
    rs = numpy.random.RandomState(seed)
    K = len(sizes)
    centres = (rs.rand(K, d) * scale).astype(numpy.float32)
    a = numpy.repeat(numpy.arange(K), sizes).astype(numpy.uint32)
    perm = rs.permutation(len(a))
    a = a[perm]
    x = (centres[a] + rs.randn(len(a), d) * 0.12 * scale).astype(numpy.float32)
    return x, centres, a


@pytest.mark.parametrize("d", [16, 64, 512])
def test_cluster_sizes_around_the_tiles(d, monkeypatch):
    sizes = [1, 31, 32, 33, 511, 512, 513, 1023, 1025, 2, 64, 96]
    x, c, a = sized(sizes, d, seed=71 + d)
    check(10, x, c, a, monkeypatch=monkeypatch, expect="f16")


def test_one_cluster_holds_ninety_percent(monkeypatch):
    sizes = [5400] + [30] * 20
    x, c, a = sized(sizes, 64, seed=81)
    check(10, x, c, a, monkeypatch=monkeypatch, expect="f16")


@pytest.mark.parametrize("filt", ["f16", "f32"])
def test_assignments_not_the_nearest_centroid(filt, monkeypatch):
    """Legal inputs: 30 % of the rows in a random other cluster (the radii grow, the prune rule stays sound)."""
    x, c, a = blobs(3000, 64, 30, 1.0, seed=91)
    rs = numpy.random.RandomState(91)
    moved = rs.choice(3000, 900, replace=False)
    a = a.copy()
    a[moved] = (a[moved] + rs.randint(1, 30, 900)) % 30
    check(10, x, c, a, env={"KMCUDA_AMD_FILTER": filt}, monkeypatch=monkeypatch, expect=filt)


@pytest.mark.parametrize("k", [1, 2, 32, 64, 65, 200])
def test_k(k, monkeypatch):
    x, c, a = blobs(3000, 64, 30, 1.0, seed=101)
    check(k, x, c, a, monkeypatch=monkeypatch, expect="f16", rows=60)


@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.parametrize("k", [39, 40, 57])
def test_k_at_and_beyond_n(k, d, monkeypatch):
    """k = N - 1 fills every list; beyond it the slots no row fills hold the oracle's index 0."""
    x, c, a = blobs(40, d, 4, 1.0, seed=111)
    nb, _ = check(k, x, c, a, monkeypatch=monkeypatch)
    if k > 39:
        assert (nb[1:, 39:] == 0).all()


@pytest.mark.parametrize("K", [8000, 8200])
def test_many_clusters(K, monkeypatch):
    """Above 8192 clusters the query-order key of mode 3 has no 32 bits left: identity order."""
    x, c, a = blobs(3 * K, 16, K, 1.0, seed=121, spread=0.02)
    check(5, x, c, a, monkeypatch=monkeypatch, expect="f16", rows=40)


# ----------------------------------------------------------------------------------------------------------------
# every switch gives the oracle's lists
# ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def skewed():
    sizes = [3000, 1200, 600] + [40] * 40 + [1, 2, 3]
    return sized(sizes, 64, seed=131)


@pytest.mark.parametrize("order", [0, 1, 2, 3])
@pytest.mark.parametrize("tight", [0, 1])
def test_order_and_tight(skewed, order, tight, monkeypatch):
    x, c, a = skewed
    check(10, x, c, a, env={"KMCUDA_AMD_KNN_ORDER": order, "KMCUDA_AMD_KNN_TIGHT": tight}, monkeypatch=monkeypatch,
          expect="f16")


@pytest.mark.parametrize("shards", [2, 3, 5])
def test_virtual_shards(skewed, shards, monkeypatch):
    x, c, a = skewed
    check(10, x, c, a, env={"KMCUDA_AMD_VIRTUAL_SHARDS": shards}, monkeypatch=monkeypatch, expect="f16")


def test_xcd_dispatch(monkeypatch):
    x, c, a = blobs(40000, 64, 200, 1.0, seed=141, spread=0.03)
    check(10, x, c, a, env={"KMCUDA_AMD_KNN_XCD": 1}, monkeypatch=monkeypatch, expect="f16", rows=60)


@pytest.mark.parametrize("d", [64, 1100])
def test_shares_cover_the_answer(d, monkeypatch):
    """KMCUDA_AMD_KNN_SHARD=i/3 runs one share; the three shares, each into a sentinel-filled buffer, write disjoint
    row sets whose union is the whole answer (rows without a cluster included)."""
    from kmcuda_amd import knn_cuda
    x, c, a = degenerate(d, seed=151)
    k = 10
    ref, _ = oracle.knn(k, x, c, a)
    dev = torch.device("cuda", 0)
    xs, cs = torch.from_numpy(x).to(dev), torch.from_numpy(c).to(dev)
    at = torch.from_numpy(a.view(numpy.int32)).to(dev)
    sentinel = 0x5A5A5A5A
    written = numpy.zeros(len(x), int)
    got = numpy.full((len(x), k), sentinel, numpy.uint32)
    for i in range(3):
        monkeypatch.setenv("KMCUDA_AMD_KNN_SHARD", "%d/3" % i)
        out = torch.full((len(x), k), sentinel, dtype=torch.int32, device=dev)
        knn_cuda(k, (xs.data_ptr(), 0, x.shape, out.data_ptr()), (cs.data_ptr(), len(c)), at.data_ptr(), device=1)
        nb = out.cpu().numpy().view(numpy.uint32)
        mine = (nb != sentinel).any(axis=1)
        assert (nb[~mine] == sentinel).all()
        written += mine
        got[mine] = nb[mine]
    assert (written == 1).all(), numpy.bincount(written)
    assert (got == ref).all()


# ----------------------------------------------------------------------------------------------------------------
# angular
# ----------------------------------------------------------------------------------------------------------------
def unit_corpus(n, d, seed):
    """Unit rows with exact duplicates, near duplicates (products >= 1 clamp to distance 0) and antipodal rows."""
    rs = numpy.random.RandomState(seed)
    x = rs.randn(n, d)
    x /= numpy.linalg.norm(x, axis=1, keepdims=True)
    m = n // 10
    x[m:2 * m] = x[:m]                                             # duplicates
    near = x[:m] + rs.randn(m, d) * 1e-7
    x[2 * m:3 * m] = near / numpy.linalg.norm(near, axis=1, keepdims=True)
    x[3 * m:4 * m] = -x[:m]                                        # antipodal
    return x.astype(numpy.float32)


@pytest.mark.parametrize("d", [16, 256, 768])
@pytest.mark.parametrize("half", [False, True])
def test_angular_clamp(d, half, monkeypatch):
    n, K = 2000, 20
    x = unit_corpus(n, d, seed=d + half)
    if half:
        x = x.astype(numpy.float16)
    rs = numpy.random.RandomState(d)
    c = x[rs.choice(n, K, replace=False)].copy()
    a, _, _ = oracle.lloyd_assign(x.astype(numpy.float32), c.astype(numpy.float32), metric=oracle.COS)
    from kmcuda_amd import knn_cuda
    nb = knn_cuda(10, x, c, a, metric="cos", device=1)
    ref, _ = oracle.knn(10, x.astype(numpy.float32), c.astype(numpy.float32), a, metric="cos")
    assert_knn_only_acos_matters(x, nb, ref, "D=%d half=%s" % (d, half))
