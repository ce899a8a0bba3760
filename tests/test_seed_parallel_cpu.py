"""k-means|| seeding (kmcuda_amd/seed.py, C ABI kmamd_kmeans_seed_parallel): the surface, every refusal that is decided
before a device is touched, the hash, and the conditions the GPU tests' fixtures have to meet -- checked on the numpy
restatement (tests/_seed_parallel_ref.py)."""
import ctypes
import fnmatch
import os
import re
import subprocess

import numpy
import pytest

import _seed_parallel_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "kmamd_kmeans_seed_parallel"
_SENTINEL = 0x5A5A5A5A


def _built():
    import __graft_entry__
    __graft_entry__.build()
    from kmcuda_amd import _lib
    return _lib


# ----------------------------------------------------------------------------------------------------------------------
# the surface
# ----------------------------------------------------------------------------------------------------------------------
def test_importable_declared_and_listed():
    import kmcuda_amd
    from kmcuda_amd import kmeans_seed_parallel, _lib  # noqa: F401
    assert callable(kmcuda_amd.kmeans_seed_parallel)
    assert NAME in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "kmcuda_amd.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, header)
    with open(os.path.join(ROOT, "kmcuda_amd", "csrc", "exports.map")) as f:
        patterns = re.findall(r"^\s*([\w*]+);", f.read().split("local:")[0], flags=re.M)
    assert any(fnmatch.fnmatchcase(NAME, p) for p in patterns)


def test_library_exports_the_symbol_with_argtypes():
    _l = _built()
    L = _l.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _l.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert NAME in exported
    fn = getattr(L, NAME)
    assert fn.restype is _l.i32 and len(fn.argtypes) == 19
    assert fn.argtypes[2] is ctypes.c_uint16 and fn.argtypes[5] is _l.f32 and fn.argtypes[7] is _l.i32


def test_the_init_is_appended_to_the_enum_and_named():
    with open(os.path.join(ROOT, "include", "kmcuda.h")) as f:
        text = f.read()
    enum = re.search(r"Centroid seeding.*?typedef enum \{(.*?)\} KMCUDAInitMethod;", text, flags=re.S).group(1)
    names = re.findall(r"\b(kmcudaInitMethod\w+)\b\s*(?:=\s*\d+)?\s*,?\s*/\*", enum)
    assert names == ["kmcudaInitMethodRandom", "kmcudaInitMethodPlusPlus", "kmcudaInitMethodAFKMC2",
                     "kmcudaInitMethodImport", "kmcudaInitMethodParallel"]
    for name in ("k-means||", "kmeans||", "scalable-k-means++"):
        assert '{"%s", kmcudaInitMethodParallel}' % name in text
    from kmcuda_amd import api
    assert api._INIT["k-means||"] == api._INIT["kmeans||"] == api._INIT["scalable-k-means++"] == 4
    assert api._INIT["k-means++"] == 1   # and the default init stays k-means++
    import inspect
    assert inspect.signature(api.kmeans_cuda).parameters["init"].default == "k-means++"


# ----------------------------------------------------------------------------------------------------------------------
# refusals, before the library is loaded
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Fails the test if the library is loaded at all: validation must come first."""
    from kmcuda_amd import _lib

    def boom():
        raise AssertionError("the device library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", boom)


def _x(n=64, d=8, dtype=numpy.float32):
    return numpy.random.default_rng(5).standard_normal((n, d)).astype(dtype)


@pytest.mark.parametrize("kw, exc", [
    (dict(clusters=1), ValueError), (dict(clusters=0), ValueError), (dict(clusters=65), ValueError),
    (dict(clusters=4.0), TypeError), (dict(clusters=True), TypeError),
    (dict(rounds=0), ValueError), (dict(rounds=65), ValueError), (dict(rounds=2.5), TypeError),
    (dict(oversampling=0), ValueError), (dict(oversampling=-1.0), ValueError),
    (dict(oversampling=float("nan")), ValueError), (dict(oversampling=float("inf")), ValueError),
    (dict(oversampling=1e39), ValueError),   # inf as a float32
    (dict(oversampling="many"), TypeError),
    (dict(metric="manhattan"), ValueError), (dict(metric=3), TypeError),
    (dict(device=-1), ValueError), (dict(device="0"), TypeError), (dict(seed=1.5), TypeError),
])
def test_python_refusals(no_device, kw, exc):
    from kmcuda_amd import kmeans_seed_parallel
    args = dict(clusters=4)
    args.update(kw)
    with pytest.raises(exc):
        kmeans_seed_parallel(_x(), **args)


def test_python_refuses_bad_rows(no_device, monkeypatch):
    torch = pytest.importorskip("torch")
    from kmcuda_amd import kmeans_seed_parallel
    with pytest.raises(TypeError):
        kmeans_seed_parallel(_x(dtype=numpy.float64), 4)
    with pytest.raises(TypeError):
        kmeans_seed_parallel(_x().astype(numpy.int32), 4)
    with pytest.raises(ValueError):
        kmeans_seed_parallel(_x()[0], 4)
    with pytest.raises(ValueError):
        kmeans_seed_parallel(_x()[:, :, None], 4)
    with pytest.raises(ValueError):
        kmeans_seed_parallel(_x(d=7, dtype=numpy.float16), 4)
    with pytest.raises(ValueError):   # a host tensor is neither kind
        kmeans_seed_parallel(torch.from_numpy(_x()), 4)
    monkeypatch.setenv("KMCUDA_AMD_FP16_STRICT", "1")
    with pytest.raises(ValueError):
        kmeans_seed_parallel(_x(dtype=numpy.float16), 4)


def test_kmeans_cuda_refuses_bad_parameters_and_weights():
    """init="k-means||": the tuple's rounds and oversampling, and sample weights, through the mirror module and the
    native one (both check before the device is asked for anything)."""
    _built()
    import libKMCUDA
    from kmcuda_amd import api
    x = _x()
    for mod in (api, libKMCUDA):
        for init in (("k-means||", 0), ("k-means||", 65), ("k-means||", 3, -1.0), ("k-means||", 3, float("nan")),
                     ("k-means||", 3, float("inf")), "k-means|||"):
            with pytest.raises(ValueError):
                mod.kmeans_cuda(x, 4, init=init, device=1 << 20)
    with pytest.raises(ValueError):
        api.kmeans_cuda(x, 4, init="k-means||", sample_weight=numpy.ones(64, numpy.float32), device=1 << 20)


def _raw_call(L, x, fp16, **over):
    n, d = x.shape
    a = dict(metric=0, n=n, d=d, k=4, rounds=3, ell=8.0, device=0, device_ptrs=-1, samples=x.ctypes.data)
    a.update(over)
    k = max(int(a["k"]), 1)
    cen = numpy.full((k, d), -7.5, x.dtype)
    rows = numpy.full(16, _SENTINEL, numpy.uint32)
    counts = numpy.full(16, _SENTINEL, numpy.uint32)
    total = numpy.full(1, _SENTINEL, numpy.uint32)
    ends = numpy.full(65, _SENTINEL, numpy.uint32)
    fell = numpy.full(1, 77, numpy.int32)
    a.setdefault("centroids", cen.ctypes.data)
    rc = L.kmamd_kmeans_seed_parallel(a["metric"], a["n"], a["d"], a["k"], a["rounds"], a["ell"], 0, a["device"],
                                      a["device_ptrs"], int(fp16), 0, a["samples"], a["centroids"], rows.ctypes.data,
                                      counts.ctypes.data, 16, total.ctypes.data, ends.ctypes.data, fell.ctypes.data)
    untouched = ((cen == x.dtype.type(-7.5)).all() and (rows == _SENTINEL).all() and (counts == _SENTINEL).all()
                 and total[0] == _SENTINEL and (ends == _SENTINEL).all() and fell[0] == 77)
    return rc, untouched


@pytest.mark.parametrize("over", [dict(metric=2), dict(d=0), dict(n=0), dict(k=1), dict(k=0), dict(k=65),
                                  dict(rounds=65), dict(ell=-1.0), dict(ell=float("nan")), dict(ell=float("inf")),
                                  dict(samples=None), dict(centroids=None), dict(device=-1),
                                  dict(device=0, device_ptrs=1)])
def test_c_call_refuses_with_outputs_untouched(over):
    L = _built().lib()
    rc, untouched = _raw_call(L, _x(), False, **over)
    assert rc == 1 and untouched


def test_c_call_refuses_strict_half2_and_odd_half_features(monkeypatch):
    L = _built().lib()
    rc, untouched = _raw_call(L, _x(d=7, dtype=numpy.float16), True)
    assert rc == 1 and untouched
    monkeypatch.setenv("KMCUDA_AMD_FP16_STRICT", "1")
    rc, untouched = _raw_call(L, _x(dtype=numpy.float16), True)
    assert rc == 1 and untouched
    # the switch concerns half rows only: fp32 rows get past the checks (to the device, or to "no such device")
    rc, _ = _raw_call(L, _x(), False, device=31)
    assert rc in (0, 2)


def test_kmeans_weighted_refuses_weights_with_this_init():
    """kmamd_kmeans_weighted(init = 4, weights): InvalidArguments before any device is touched."""
    L = _built().lib()
    x = _x()
    cen = numpy.full((4, 8), -7.5, numpy.float32)
    asg = numpy.full(64, _SENTINEL, numpy.uint32)
    w = numpy.ones(64, numpy.float32)
    rc = L.kmamd_kmeans_weighted(4, None, 0.01, 0.0, 0, 64, 8, 4, 0, 1, -1, 0, 0, x.ctypes.data, cen.ctypes.data,
                                 asg.ctypes.data, None, w.ctypes.data)
    assert rc == 1 and (cen == -7.5).all() and (asg == _SENTINEL).all()


# ----------------------------------------------------------------------------------------------------------------------
# the hash
# ----------------------------------------------------------------------------------------------------------------------
def test_hash_values_computed_by_hand():
    """splitmix64's finaliser of ((r << 32) | s) + (seed + 1) * 0x9E3779B97F4A7C15, step by step in Python integers
    (the values below were computed once, with the five steps written out, and are pinned); the vectorised form the
    restatement draws with agrees, also for a row index >= 2^31."""
    # (seed 0, r 0, s 0) is splitmix64's first output for the state 0, the published test vector.  seed 0xFFFFFFFF:
    # (seed + 1) * 0x9E3779B97F4A7C15 mod 2^64 = 0x7F4A7C1500000000, + (64 << 32 | 0x80000001) = 0x7F4A7C5580000001.
    pinned = {(0, 0, 0): 0xE220A8397B1DCDAF, (7, 3, 12345): 0x9F70C87C2B896690,
              (0xFFFFFFFF, 64, 0x80000001): 0x24B5B3164C0C94EA}
    for (seed, r, s), want in pinned.items():
        assert _by_hand(seed, r, s) == want
        assert ref.hash64(seed, r, s) == want
    # the vectorised form at s >= 2^31: rows 0x80000000 .. 0x80000003 of round 64, seed 0xFFFFFFFF
    u = _uniforms_at(0xFFFFFFFF, 64, 0x80000000, 4)
    assert u[1] == (pinned[(0xFFFFFFFF, 64, 0x80000001)] >> 11) * 2.0 ** -53
    assert (ref.uniforms(7, 3, 12346)[12345] == (pinned[(7, 3, 12345)] >> 11) * 2.0 ** -53)


def _by_hand(seed, r, s):
    m = (1 << 64) - 1
    z = ((r * (1 << 32) + s) + (seed + 1) * 0x9E3779B97F4A7C15) % (1 << 64)
    z = z ^ (z >> 30)
    z = (z * 0xBF58476D1CE4E5B9) & m
    z = z ^ (z >> 27)
    z = (z * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def _uniforms_at(seed, r, s0, n):
    return numpy.array([(ref.hash64(seed, r, s0 + i) >> 11) * 2.0 ** -53 for i in range(n)])


# ----------------------------------------------------------------------------------------------------------------------
# the fixtures of the GPU tests, on the restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.CANDIDATE_FIXTURES)
def test_candidate_fixtures_have_no_margin_rows(name):
    r = ref.restated(name)
    assert r["margin_rows"] == []
    assert len(r["round_ends"]) == ref.ROUNDS + 1 and r["round_ends"][-1] == len(r["rows"])
    assert min(r["draw_counts"]) >= 2          # every round takes the engine's path
    assert not r["fell_back"]
    for lo, hi in zip(r["round_ends"][:-1], r["round_ends"][1:]):   # ascending within a round
        assert (numpy.diff(r["rows"][lo:hi].astype(numpy.int64)) > 0).all()
    assert r["counts"].sum() == _rows_with_a_cluster(name)


def _rows_with_a_cluster(name):
    x, _ = ref.fixture(name)
    return int((~numpy.isnan(x.astype(numpy.float32)).any(axis=1)).sum())


def test_duplicate_fixture_drops_candidates():
    r = ref.restated("nan-and-duplicates")
    x, _ = ref.fixture("nan-and-duplicates")
    dropped = r["rows"][r["counts"] == 0]
    assert len(dropped) >= 5
    live = {x[i].tobytes() for i in r["live_rows"]}
    assert all(x[i].tobytes() in live for i in dropped)        # each is a copy of a live candidate
    assert len(live) == len(r["live_rows"])
    assert not numpy.isnan(x[r["rows"], 0]).any()               # a NaN first feature is never drawn
    assert not numpy.isnan(x[r["rows"]]).any()


def test_sparse_fixture_has_rounds_with_no_and_with_one_candidate():
    s = ref.SPARSE
    seen = set()
    for seed in s["seeds"]:
        r = ref.restated(s["fixture"], s["clusters"], s["rounds"], s["oversampling"], seed)
        assert r["margin_rows"] == [] and not r["fell_back"]
        assert 0 in r["draw_counts"] and 1 in r["draw_counts"]
        seen.add(tuple(r["draw_counts"]))
    assert (1, 2, 0, 1, 1, 0) in seen   # seed 0: a round without candidates between rounds with some


def test_saturation_fixture_draws_every_row_with_a_term():
    s = ref.SATURATION
    r = ref.restated("saturation", s["clusters"], s["rounds"], s["oversampling"], s["seed"], False)
    x, _, first, dup = ref.saturation_rows()
    assert r["margin_rows"] == [] and r["first"] == first
    assert r["draw_counts"] == [len(x) - 1 - len(dup)]
    assert (r["rows"][1:] == numpy.setdiff1d(numpy.arange(len(x)), [first] + dup)).all()


def test_fallback_fixture_falls_back():
    f = ref.FALLBACK
    r = ref.restated(f["fixture"], f["clusters"], f["rounds"], f["oversampling"], f["seed"])
    assert r["margin_rows"] == [] and r["fell_back"] and len(r["live_rows"]) < f["clusters"]


def _weighted_kmeanspp(x, w, k, rs, successor):
    """k-means++ over weighted rows: the first seed uniform, every other one by a draw with probability proportional
    to w * (the distance -- not squared -- to the nearest seed so far).  successor=False: the drawn row itself, the
    textbook rule.  successor=True: the row after it, as the reference's chooser and so this library's takes it
    (tests/_seed_parallel_ref.py: BLOBS)."""
    x = x.astype(numpy.float64)
    seeds = [int(rs.randint(len(x)))]
    dist = numpy.linalg.norm(x - x[seeds[0]], axis=1)
    while len(seeds) < k:
        p = w * dist
        j = int(rs.choice(len(x), p=p / p.sum()))
        seeds.append(min(j + 1, len(x) - 1) if successor else j)
        dist = numpy.minimum(dist, numpy.linalg.norm(x - x[seeds[-1]], axis=1))
    return seeds


def test_every_blob_holds_a_seed():
    b = ref.BLOBS
    r = ref.restated(b["fixture"], b["clusters"], b["rounds"], b["oversampling"], b["seed"])
    x, _ = ref.fixture(b["fixture"])
    assert (ref.blob_of(x) == numpy.arange(len(x)) // 500).all()   # 16 blobs of 500 consecutive rows
    assert r["margin_rows"] == [] and not r["fell_back"]
    cand = x[r["live_rows"]]
    assert set(ref.blob_of(cand)) == set(range(16))            # the candidates reach every blob ...
    w = r["live_counts"].astype(numpy.float64)
    for s in range(5):                                          # ... and so do the seeds drawn among them
        for successor in (False, True):
            seeds = _weighted_kmeanspp(cand, w, b["clusters"], numpy.random.RandomState(s), successor)
            assert set(ref.blob_of(cand[seeds])) == set(range(16)), (s, successor)
