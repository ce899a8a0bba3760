"""k-means|| seeding on the device (kmeans_seed_parallel, kmeans_cuda(init="k-means||")) against the numpy restatement
of tests/_seed_parallel_ref.py: candidates, round ends and counts EQUAL (tests/test_seed_parallel_cpu.py asserts that
no fixture has a row inside the margin in which the order of phi's summation could decide a draw), the seeds against
the public weighted k-means++ call, the fallback, the init inside kmeans_cuda, and repeatability."""
import numpy
import pytest

import _seed_parallel_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch.device("cuda", 0)


def _bits(a):
    a = numpy.ascontiguousarray(a)
    return a.view(numpy.uint16 if a.dtype == numpy.float16 else numpy.uint32)


def _run(x, metric, clusters=ref.K, rounds=ref.ROUNDS, oversampling=ref.ELL, seed=ref.SEED):
    from kmcuda_amd import kmeans_seed_parallel
    return kmeans_seed_parallel(x, clusters, rounds=rounds, oversampling=oversampling, metric=metric, seed=seed,
                                return_candidates=True)


def _check_candidates(info, want):
    assert list(info["round_ends"]) == list(want["round_ends"])
    assert numpy.array_equal(info["rows"], want["rows"])
    assert numpy.array_equal(info["counts"], want["counts"])
    assert info["fell_back"] == want["fell_back"]


def _public_seeds(x, metric, rows, counts, clusters, seed):
    """What the issue defines the seeds as: the public weighted k-means++ call over the live candidates."""
    from kmcuda_amd import kmeans_cuda
    live = counts > 0
    cen, _ = kmeans_cuda(x[rows[live]], clusters, sample_weight=counts[live].astype(numpy.float32), init="k-means++",
                         tolerance=1.0, yinyang_t=0, metric=metric, seed=seed, device=1)
    return cen


def _are_rows(cen, x):
    have = {r.tobytes() for r in numpy.ascontiguousarray(x)}
    return all(c.tobytes() in have for c in numpy.ascontiguousarray(cen))


# 1 + 4. candidates against the restatement, centroids against the public call
@pytest.mark.parametrize("name", ref.CANDIDATE_FIXTURES)
def test_candidates_and_seeds(name):
    x, metric = ref.fixture(name)
    want = ref.restated(name)
    cen, info = _run(x, metric)
    _check_candidates(info, want)
    assert cen.dtype == x.dtype and cen.shape == (ref.K, x.shape[1])
    assert _are_rows(cen, x)
    assert numpy.array_equal(_bits(cen), _bits(_public_seeds(x, metric, info["rows"], info["counts"], ref.K, ref.SEED)))


# 2. rounds with 0 or 1 new candidate: no engine, and the single-centroid distance pass
@pytest.mark.parametrize("seed", ref.SPARSE["seeds"])
def test_rounds_with_no_or_one_candidate(seed):
    s = ref.SPARSE
    x, metric = ref.fixture(s["fixture"])
    want = ref.restated(s["fixture"], s["clusters"], s["rounds"], s["oversampling"], seed)
    assert 0 in want["draw_counts"] and 1 in want["draw_counts"]
    cen, info = _run(x, metric, s["clusters"], s["rounds"], s["oversampling"], seed)
    _check_candidates(info, want)
    assert _are_rows(cen, x)
    assert numpy.array_equal(_bits(cen), _bits(_public_seeds(x, metric, info["rows"], info["counts"], s["clusters"],
                                                             seed)))


# 3. saturation: round 1 draws every row with a non-zero term; the ordered fill across all blocks
def test_saturation_draws_every_row_in_order():
    s = ref.SATURATION
    x, metric, first, dup = ref.saturation_rows()
    cen, info = _run(x, metric, s["clusters"], s["rounds"], s["oversampling"], s["seed"])
    assert info["rows"][0] == first
    assert numpy.array_equal(info["rows"][1:], numpy.setdiff1d(numpy.arange(len(x)), [first] + dup))
    assert list(info["round_ends"]) == [1, len(x) - len(dup)]
    assert not info["fell_back"] and _are_rows(cen, x)
    # every row is its own nearest candidate; the first candidate also attracts its copies
    assert info["counts"][0] == 1 + len(dup) and (info["counts"][1:] == 1).all()


# 5. fallback: fewer live candidates than clusters
def test_fallback_is_plain_kmeanspp():
    from kmcuda_amd import kmeans_cuda
    f = ref.FALLBACK
    x, metric = ref.fixture(f["fixture"])
    want = ref.restated(f["fixture"], f["clusters"], f["rounds"], f["oversampling"], f["seed"])
    cen, info = _run(x, metric, f["clusters"], f["rounds"], f["oversampling"], f["seed"])
    _check_candidates(info, want)
    assert info["fell_back"] is True
    plain, _ = kmeans_cuda(x, f["clusters"], init="k-means++", tolerance=1.0, yinyang_t=0, seed=f["seed"], device=1)
    assert numpy.array_equal(_bits(cen), _bits(plain))


# 6. kmeans_cuda(init="k-means||") against the stand-alone seeds
@pytest.mark.parametrize("name", ["l2-5003x32", "fp16-5003x32", "angular-5003x32"])
def test_kmeans_cuda_init_equals_imported_seeds(name):
    import libKMCUDA
    from kmcuda_amd import api, kmeans_seed_parallel
    x, metric = ref.fixture(name)
    kw = dict(tolerance=0.01, yinyang_t=0, metric=metric, seed=9, device=1)
    seeds = kmeans_seed_parallel(x, ref.K, metric=metric, seed=9)
    c0, a0 = api.kmeans_cuda(x, ref.K, init=seeds, **kw)
    for mod in (api, libKMCUDA):
        for init in ("k-means||", "kmeans||", "scalable-k-means++", ("k-means||",), ("k-means||", 5),
                     ("k-means||", 5, 2.0 * ref.K)):
            c1, a1 = mod.kmeans_cuda(x, ref.K, init=init, **kw)
            assert numpy.array_equal(a0, a1), (mod.__name__, init)
            assert numpy.array_equal(_bits(c0), _bits(c1)), (mod.__name__, init)
    # the tuple's parameters reach the seeding
    seeds3 = kmeans_seed_parallel(x, ref.K, rounds=ref.ROUNDS, oversampling=ref.ELL, metric=metric, seed=9)
    assert not numpy.array_equal(_bits(seeds3), _bits(seeds))
    c2, a2 = api.kmeans_cuda(x, ref.K, init=seeds3, **kw)
    for mod in (api, libKMCUDA):
        c3, a3 = mod.kmeans_cuda(x, ref.K, init=("k-means||", ref.ROUNDS, ref.ELL), **kw)
        assert numpy.array_equal(a2, a3) and numpy.array_equal(_bits(c2), _bits(c3)), mod.__name__


def test_kmeans_cuda_init_on_device_tensors():
    from kmcuda_amd import api, kmeans_seed_parallel
    x, metric = ref.fixture("l2-5003x32")
    xt = torch.from_numpy(x.copy()).to(_dev())
    kw = dict(tolerance=0.01, yinyang_t=0.1, metric=metric, seed=9, device=1)
    seeds_t = kmeans_seed_parallel(xt, ref.K, metric=metric, seed=9)
    assert seeds_t.is_cuda and seeds_t.dtype == torch.float32
    seeds = kmeans_seed_parallel(x, ref.K, metric=metric, seed=9)
    assert numpy.array_equal(_bits(seeds_t.cpu().numpy()), _bits(seeds))
    c0, a0 = api.kmeans_cuda(x, ref.K, init=seeds, **kw)
    cp, ap = api.kmeans_cuda((xt.data_ptr(), 0, x.shape), ref.K, init="k-means||", **kw)
    c1 = api._DEVICE_ALLOCS[cp].cpu().numpy()
    a1 = api._DEVICE_ALLOCS[ap].cpu().numpy().view(numpy.uint32)
    api.free_device_ptr(cp)
    api.free_device_ptr(ap)
    assert numpy.array_equal(a0, a1) and numpy.array_equal(_bits(c0), _bits(c1))
    assert torch.equal(xt.cpu(), torch.from_numpy(x.copy()))


def test_sample_weight_with_this_init_raises():
    import libKMCUDA
    from kmcuda_amd import api
    x, _ = ref.fixture("l2-3000x30")
    w = numpy.ones(len(x), numpy.float32)
    for mod in (api, libKMCUDA):
        with pytest.raises(ValueError):
            mod.kmeans_cuda(x, ref.K, init="k-means||", sample_weight=w, seed=1, device=1)


# 7. repeatability; host and device buffers
@pytest.mark.parametrize("name", ["l2-5003x32", "fp16-5003x32"])
def test_repeatable_and_host_equals_device(name):
    x, metric = ref.fixture(name)
    c0, i0 = _run(x, metric)
    c1, i1 = _run(x, metric)
    ct, it = _run(torch.from_numpy(x.copy()).to(_dev()), metric)
    assert ct.is_cuda
    for c, i in ((c1, i1), (ct.cpu().numpy(), it)):
        assert numpy.array_equal(_bits(c0), _bits(c))
        assert numpy.array_equal(i0["rows"], i["rows"]) and numpy.array_equal(i0["counts"], i["counts"])
        assert list(i0["round_ends"]) == list(i["round_ends"]) and i0["fell_back"] == i["fell_back"]


# 7b. half rows on the device that do not lie 16-byte aligned: the engine's filter gets no halves, the same result
def test_misaligned_half_device_view():
    name = "fp16-5003x32"
    x, metric = ref.fixture(name)
    want = ref.restated(name)
    buf = torch.empty(x.size + 2, dtype=torch.float16, device=_dev())
    xs = buf[2:].view(x.shape)   # one half2 pair into the buffer
    xs.copy_(torch.from_numpy(x.copy()))
    assert xs.data_ptr() % 16 != 0 and xs.is_contiguous()
    cen, info = _run(xs, metric)
    _check_candidates(info, want)
    cen = cen.cpu().numpy()
    assert cen.dtype == x.dtype and cen.shape == (ref.K, x.shape[1])
    assert _are_rows(cen, x)
    assert numpy.array_equal(_bits(cen), _bits(_public_seeds(x, metric, info["rows"], info["counts"], ref.K, ref.SEED)))


# 8. the blob fixture: every blob holds a seed
def test_every_blob_holds_a_seed():
    """16 blobs, the call's defaults, K = 32: why not K = 16 is written at tests/_seed_parallel_ref.py: BLOBS (this
    library's k-means++ takes the row AFTER the proportional draw, as the reference's chooser does)."""
    b = ref.BLOBS
    x, metric = ref.fixture(b["fixture"])
    want = ref.restated(b["fixture"], b["clusters"], b["rounds"], b["oversampling"], b["seed"])
    cen, info = _run(x, metric, b["clusters"], b["rounds"], b["oversampling"], b["seed"])
    _check_candidates(info, want)
    assert _are_rows(cen, x)
    assert set(ref.blob_of(cen)) == set(range(16))
