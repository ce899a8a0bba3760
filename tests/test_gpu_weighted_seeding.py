"""Weighted k-means++ seeding on the device against the numpy restatement of tests/_weighted_seed_ref.py (the reference's
chooser over the terms fl(w * d); anchored on the C oracle at w = 1 by
tests/test_weighted_seed_ref_cpu.py).  tolerance = 1 stops a run at its first stop test, before any update, so the
centroids that come back ARE the seeds; every comparison is of bits.  The weights reach further than any data set's
distances do: eighty binades of them, terms thirty binades under the bulk (the outlier list, short and overflowing),
subnormal and infinite products, each through the device chooser, the host chooser, filtered and plain steps and row
shards.  Last, the k-means|| seeds -- so far compared with the public weighted call they are made by -- against the
same restatement."""
import ctypes
import os
import re
import sys
import tempfile

import numpy
import pytest

import _seed_parallel_ref as par
import _weighted_seed_ref as ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PATHS = {
    "default": {},
    "host": {"KMCUDA_AMD_KMPP_HOST": "1"},
    "filtered": {"KMCUDA_AMD_KMPP_FILTER": "2"},
    "plain": {"KMCUDA_AMD_KMPP_FILTER": "0"},
}
_SWITCHES = ("KMCUDA_AMD_KMPP_HOST", "KMCUDA_AMD_KMPP_FILTER", "KMCUDA_AMD_VIRTUAL_SHARDS")
_RUNTIME_ERROR = 4          # kmcudaRuntimeError; kmcuda_amd.api raises AssertionError("... failure (bug?)") for it
_SENTINEL = 0x5A5A5A5A


class _Stdout:
    """Captures the C library's stdout (as tests/test_gpu_kmeans.py: StdoutListener)."""

    def __enter__(self):
        sys.stdout.flush()
        self._file = tempfile.TemporaryFile()
        self._backup = os.dup(1)
        os.dup2(self._file.fileno(), 1)
        return self

    def __exit__(self, *exc):
        ctypes.CDLL(None).fflush(None)
        os.dup2(self._backup, 1)
        self._file.seek(0)
        self.text = self._file.read().decode("utf-8")
        self._file.close()
        os.close(self._backup)


def _bits(a):
    a = numpy.ascontiguousarray(a)
    return a.view(numpy.uint16 if a.dtype == numpy.float16 else numpy.uint32)


def _iterations():
    from kmcuda_amd import _lib
    it = ctypes.c_uint32(0)
    assert _lib.lib().kmamd_last_run_stats(ctypes.byref(it), None, None, None, None) == 0
    return it.value


def _set_path(monkeypatch, path, shards=None):
    for key in _SWITCHES:
        monkeypatch.delenv(key, raising=False)
    for key, val in PATHS[path].items():
        monkeypatch.setenv(key, val)
    if shards:
        monkeypatch.setenv("KMCUDA_AMD_VIRTUAL_SHARDS", str(shards))


def _seed_call(x, w, metric, seed, clusters=ref.K):
    """(seeds, host-chooser steps or None, steps or None) of one call at verbosity 2."""
    from kmcuda_amd import kmeans_cuda
    out = _Stdout()
    with out:
        cen, _ = kmeans_cuda(x, clusters, sample_weight=w, init="k-means++", tolerance=1.0, yinyang_t=0, seed=seed,
                             metric=metric, device=1, verbosity=2)
    assert _iterations() == 1
    took = re.search(r"k-means\+\+: (\d+) of (\d+) steps took the host chooser", out.text)
    return cen, (int(took.group(1)) if took else None), (int(took.group(2)) if took else None)


def _check_chooser_ran(rows, weights, path, a, b, tag, shards=1):
    """Conditions, not measurements: the device chooser decided where its window allows it (tests/
    test_weighted_seed_ref_cpu.py asserts that it does), and handed over and came back where it does not.  Shards of
    fewer than 1024 rows do not start on 256-row boundaries (row_plan) and take the host chooser by design (DESIGN.md
    6.1): every shard then weighs its slice for the host's walk."""
    print("%s: %s of %s steps took the host chooser" % (tag, a, b))
    n = len(ref.rows_fixture(rows)[0])
    if path == "host" or (shards > 1 and n // shards < 1024):
        assert a is None, "the device chooser ran"
        return
    assert a is not None, "the device chooser did not run"
    assert b == ref.K - 1
    if weights == "few-light" or (weights == "decades" and rows in ("l2-5003x32", "l2-5003x30", "fp16-5003x32",
                                                                    "wide-2000x320")):
        assert a < b, "no step was decided on the device"
    if weights in ("binades", "many-light"):
        assert a >= 1, "no step was handed over"


def _expect_seeds(rows, weights, seed=ref.SEED):
    x, metric = ref.rows_fixture(rows)
    w = ref.weights_fixture(weights, len(x))
    want = ref.restated(rows, weights, ref.K, seed)
    return x, w, metric, want


def _raw_call(x, w, metric, seed):
    """kmamd_kmeans_weighted through ctypes on sentinel-filled outputs: (rc, centroids, assignments)."""
    from kmcuda_amd import _lib
    n, d = x.shape
    cen = numpy.full((ref.K, d), 7, numpy.float32)
    asg = numpy.full(n, _SENTINEL, numpy.uint32)
    rc = _lib.lib().kmamd_kmeans_weighted(1, None, 1.0, 0.0, 1 if metric == "cos" else 0, n, d, ref.K, seed, 1, -1, 0, 0,
                                          x.ctypes.data, cen.ctypes.data, asg.ctypes.data, None, w.ctypes.data)
    return rc, cen, asg


# ----------------------------------------------------------------------------------------------------------------------
# 1. every (rows, weights) pair on the four chooser paths
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("rows,weights", ref.PAIRS, ids=["%s-%s" % p for p in ref.PAIRS])
def test_seeds_equal_the_restatement(rows, weights, path, monkeypatch):
    seed = ref.nan_walk_seeds()[0] if rows == "nan-5003x32" else ref.SEED
    x, w, metric, want = _expect_seeds(rows, weights, seed)
    assert want["failed"] is None and len(want["rows"]) == ref.K
    _set_path(monkeypatch, path)
    cen, a, b = _seed_call(x, w, metric, seed)
    _check_chooser_ran(rows, weights, path, a, b, "%s / %s / %s" % (rows, weights, path))
    assert cen.dtype == x.dtype
    diff = (_bits(cen) != _bits(x[want["rows"]])).any(axis=1)
    assert not diff.any(), "seeds %s differ from the restated rows" % numpy.nonzero(diff)[0][:8]


# ----------------------------------------------------------------------------------------------------------------------
# 2. row shards: every shard weighs its own slice
# ----------------------------------------------------------------------------------------------------------------------
_SHARD_PAIRS = [p for p in ref.PAIRS if p[0] in ("l2-5003x32", "cos-5003x32")]


@pytest.mark.parametrize("shards", [3, 8])
@pytest.mark.parametrize("rows,weights", _SHARD_PAIRS, ids=["%s-%s" % p for p in _SHARD_PAIRS])
def test_seeds_over_row_shards(rows, weights, shards, monkeypatch):
    x, w, metric, want = _expect_seeds(rows, weights)
    assert want["failed"] is None
    for path in sorted(PATHS):
        _set_path(monkeypatch, path, shards)
        cen, a, b = _seed_call(x, w, metric, ref.SEED)
        _check_chooser_ran(rows, weights, path, a, b, "%s / %s / %s / %d shards" % (rows, weights, path, shards), shards)
        diff = (_bits(cen) != _bits(x[want["rows"]])).any(axis=1)
        assert not diff.any(), "%s: seeds %s differ from the restated rows" % (path, numpy.nonzero(diff)[0][:8])


@pytest.mark.parametrize("weights", ["decades", "few-light"])
def test_seeds_over_eight_aligned_shards(weights, monkeypatch):
    """5003 rows in eight shards are 625 each: unaligned, the host chooser (above).  8209 rows give eight shards of
    at least 1024 rows on 256-row boundaries, the last one ragged: one chooser kernel over eight shards' terms and lists."""
    rows = "l2-8209x32"
    x, w, metric, want = _expect_seeds(rows, weights)
    assert want["failed"] is None
    for path in ("default", "filtered"):
        _set_path(monkeypatch, path, 8)
        cen, a, b = _seed_call(x, w, metric, ref.SEED)
        _check_chooser_ran(rows, weights, path, a, b, "%s / %s / %s / 8 shards" % (rows, weights, path), 8)
        assert a < b, "no step was decided on the device"
        diff = (_bits(cen) != _bits(x[want["rows"]])).any(axis=1)
        assert not diff.any(), "%s: seeds %s differ from the restated rows" % (path, numpy.nonzero(diff)[0][:8])


# ----------------------------------------------------------------------------------------------------------------------
# 3. a walk that leaves [1, N]: the reference's "internal bug" return, outputs untouched
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", sorted(PATHS))
def test_a_walk_out_of_range_is_a_runtime_error(path, monkeypatch):
    """The NaN fixture at a seed of srand() with a choice * N below 100: a NaN term makes choice_sum NaN, the `< 100`
    branch's loop never runs and j = 0 (kmcuda.cc:327-331).  The call returns kmcudaRuntimeError at that step and
    writes nothing."""
    from kmcuda_amd import kmeans_cuda
    seed = ref.nan_walk_seeds()[1]
    x, w, metric, want = _expect_seeds("nan-5003x32", "decades", seed)
    assert want["failed"] is not None and want["failed"][1] == 0
    _set_path(monkeypatch, path)
    rc, cen, asg = _raw_call(x, w, metric, seed)
    assert rc == _RUNTIME_ERROR
    assert (cen == 7).all() and (asg == _SENTINEL).all()
    with pytest.raises(AssertionError, match="failure"):
        kmeans_cuda(x, ref.K, sample_weight=w, init="k-means++", tolerance=1.0, yinyang_t=0, seed=seed, metric=metric,
                    device=1)


def test_infinite_terms_do_not_leave_the_range():
    """The overflow pair: fl(w * d) = +inf on five rows.  The restated walk stays in range at every step (a forward
    walk stops AT the first infinite term, a backward one where inf - inf turns NaN), so the call succeeds -- with the
    restated seeds, test_seeds_equal_the_restatement -- and the raw call fills its outputs."""
    x, w, metric, want = _expect_seeds("big-5003x32", "overflow")
    assert want["failed"] is None and want["steps"][0]["nonfinite"]
    rc, cen, asg = _raw_call(x, w, metric, ref.SEED)
    assert rc == 0
    assert numpy.array_equal(_bits(cen), _bits(x[want["rows"]])) and (asg < ref.K).all()


# ----------------------------------------------------------------------------------------------------------------------
# 4. device pointers; repeatability
# ----------------------------------------------------------------------------------------------------------------------
def test_weights_through_device_pointers():
    """Rows and weights as raw device pointers (torch tensors' storage): the host-array call's bits."""
    from kmcuda_amd import kmeans_cuda
    from kmcuda_amd.api import free_device_ptr, _DEVICE_ALLOCS
    x, w, metric, want = _expect_seeds("l2-5003x32", "binades")
    dev = torch.device("cuda", 0)
    xt, wt = torch.from_numpy(x.copy()).to(dev), torch.from_numpy(w.copy()).to(dev)
    cp, ap = kmeans_cuda((xt.data_ptr(), 0, x.shape), ref.K, sample_weight=wt.data_ptr(), init="k-means++",
                         tolerance=1.0, yinyang_t=0, seed=ref.SEED, metric=metric, device=1)
    assert _iterations() == 1
    cen = _DEVICE_ALLOCS[cp].cpu().numpy()
    free_device_ptr(cp)
    free_device_ptr(ap)
    assert numpy.array_equal(_bits(cen), _bits(x[want["rows"]]))
    assert torch.equal(wt.cpu(), torch.from_numpy(w.copy())) and torch.equal(xt.cpu(), torch.from_numpy(x.copy()))


def test_identical_calls_give_identical_seeds():
    """The pair on which every step is handed over to the host chooser and the next one enqueued behind it."""
    x, w, metric, want = _expect_seeds("cos-5003x32", "binades")
    c0, a0, _ = _seed_call(x, w, metric, ref.SEED)
    c1, a1, _ = _seed_call(x, w, metric, ref.SEED)
    assert a0 == a1 and numpy.array_equal(_bits(c0), _bits(c1))
    assert numpy.array_equal(_bits(c0), _bits(x[want["rows"]]))


# ----------------------------------------------------------------------------------------------------------------------
# 5. the k-means|| seeds against the restatement, not against the call that makes them
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["l2-5003x32", "nan-and-duplicates", "fp16-5003x32"])
def test_seed_parallel_centroids_equal_the_restatement(name):
    """kmeans_seed_parallel's K centroids are the weighted k-means++ seeds of its live candidates with weights
    (float)count.  Both halves restated on the CPU: the candidates and counts by
    tests/_seed_parallel_ref.py, the recluster by tests/_weighted_seed_ref.py over x[live rows] (half rows widen
    exactly) with the same K and seed."""
    from kmcuda_amd import kmeans_seed_parallel
    x, metric = par.fixture(name)
    cand = par.restated(name)
    assert not cand["fell_back"]
    live = x[cand["live_rows"]]
    want = ref.weighted_seeds(live, cand["live_counts"].astype(numpy.float32), par.K, par.SEED, metric)
    assert want["failed"] is None and len(want["rows"]) == par.K
    assert len(set(cand["live_counts"].tolist())) > 1            # (the weights are not constant)
    cen, info = kmeans_seed_parallel(x, par.K, rounds=par.ROUNDS, oversampling=par.ELL, metric=metric, seed=par.SEED,
                                     return_candidates=True)
    assert numpy.array_equal(info["rows"], cand["rows"]) and numpy.array_equal(info["counts"], cand["counts"])
    assert cen.dtype == x.dtype
    diff = (_bits(cen) != _bits(live[want["rows"]])).any(axis=1)
    assert not diff.any(), "seeds %s differ from the restated recluster" % numpy.nonzero(diff)[0][:8]
