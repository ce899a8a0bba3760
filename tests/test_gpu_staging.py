"""How kmeans_cuda brings its caller's buffers onto the shards: rows, sample weights and imported centroids, each as
host memory (uploaded, one slice per shard) or as a device pointer (used in place where it lies on the shard's device),
fp32 and halves, one shard and three (KMCUDA_AMD_VIRTUAL_SHARDS).

Every case is compared bit for bit with the same call made the plain way -- host numpy input, one shard.  tolerance = 1
stops the call at its first test, before any update, so that the centroids returned are the seeds: what is compared is
what the staged buffers held, read through the seeding and one assignment pass.

3000 rows in three shards are plain thirds (row_plan aligns shards to 256 rows only from 1024 rows per shard on): the
shards start at rows 0, 1000, 2000 and k-means++ takes its host chooser.  3300 rows are split at 0, 1024, 2048 with a
ragged last shard and take the device chooser over three shards.

Pinned elsewhere, through whole runs: host rows in three shards, k-means++ against one shard and the oracle
(test_gpu_kmeans.py::test_kmeanspp_over_row_shards_equals_one_shard_and_the_oracle); imported host centroids with host
weights, one and three shards (test_gpu_weighted.py::test_integer_weights_equal_copies); device rows and device
weights, fp32, one shard (test_gpu_weighted.py::test_constant_weights_through_device_pointers); device rows with
centroids imported into the caller's buffer, fp32, one shard (test_gpu_kmeans.py::
test_device_ptr_caller_outputs_and_imported_centroids); device halves with init="random", one shard
(test_gpu_fp16.py::test_fp16_import_and_device_ptrs)."""
import functools

import numpy
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_K = 12
_KW = dict(device=1, seed=3, tolerance=1.0, yinyang_t=0)
# (where the buffers lie, shards, rows); ("host", 1, n) is the plain call itself
_MODES = [("device", 1, 3000), ("device", 3, 3000), ("host", 3, 3000), ("device", 3, 3300), ("host", 3, 3300)]
_MODE_IDS = ["%s-%dshards-n%d" % m for m in _MODES]
_DTYPES = [numpy.float32, numpy.float16]
_DTYPE_IDS = ["fp32", "fp16"]


@functools.lru_cache(maxsize=None)
def _inputs(n, fp16):
    """rows (D = 20, or 32 halves), weights in [0.5, 2) and K rows to import; never written to"""
    rs = numpy.random.RandomState(1000 + n + int(fp16))
    x = rs.randn(n, 32 if fp16 else 20).astype(numpy.float16 if fp16 else numpy.float32)
    w = rs.uniform(0.5, 2.0, size=n).astype(numpy.float32)
    c = x[rs.choice(n, _K, replace=False)].copy()
    for a in (x, w, c):
        a.setflags(write=False)
    return x, w, c


def _bits(a):
    return a.view(numpy.uint16 if a.dtype == numpy.float16 else numpy.uint32)


def _call(n, fp16, init, weighted, where):
    from kmcuda_amd import kmeans_cuda
    from kmcuda_amd.api import _DEVICE_ALLOCS, free_device_ptr
    x, w, c = _inputs(n, fp16)
    if init == "import":
        init = c
    if where == "host":
        cen, asg = kmeans_cuda(x, _K, init=init, sample_weight=w if weighted else None, **_KW)
        return _bits(cen).copy(), asg.copy()
    dev = torch.device("cuda", 0)
    xt = torch.from_numpy(x.copy()).to(dev)
    wt = torch.from_numpy(w.copy()).to(dev)
    shape = (n, x.shape[1] // 2, True) if fp16 else x.shape
    cp, ap = kmeans_cuda((xt.data_ptr(), 0, shape), _K, init=init, sample_weight=wt.data_ptr() if weighted else None,
                         **_KW)
    cen = _DEVICE_ALLOCS[cp].cpu().numpy()
    asg = _DEVICE_ALLOCS[ap].cpu().numpy().view(numpy.uint32)
    free_device_ptr(cp)
    free_device_ptr(ap)
    assert cen.dtype == x.dtype
    # (used in place, unchanged)
    assert numpy.array_equal(_bits(xt.cpu().numpy()), _bits(x)) and numpy.array_equal(wt.cpu().numpy(), w)
    return _bits(cen).copy(), asg


@functools.lru_cache(maxsize=None)
def _plain_cached(n, fp16, init, weighted):
    return _call(n, fp16, init, weighted, "host")


def _plain(monkeypatch, n, fp16, init, weighted):
    """the same call with host numpy input on one shard, computed once per (rows, dtype, init, weights)"""
    monkeypatch.delenv("KMCUDA_AMD_VIRTUAL_SHARDS", raising=False)
    cen, asg = _plain_cached(n, fp16, init, weighted)
    x, _, c = _inputs(n, fp16)
    assert cen.shape == (_K, x.shape[1]) and asg.shape == (n,) and asg.max() < _K
    if init == "import":
        assert numpy.array_equal(cen, _bits(c))   # tolerance = 1: what comes back is what went in
    else:
        # ... and the seeds are rows of the input, K different ones
        rows = {r.tobytes() for r in _bits(x)}
        assert all(r.tobytes() in rows for r in cen) and len({r.tobytes() for r in cen}) == _K
    return cen, asg


def _check(monkeypatch, mode, dtype, init, weighted):
    where, shards, n = mode
    fp16 = dtype == numpy.float16
    cen0, asg0 = _plain(monkeypatch, n, fp16, init, weighted)
    if shards > 1:
        monkeypatch.setenv("KMCUDA_AMD_VIRTUAL_SHARDS", str(shards))
    cen, asg = _call(n, fp16, init, weighted, where)
    assert numpy.array_equal(cen, cen0)
    assert numpy.array_equal(asg, asg0)


@pytest.mark.parametrize("dtype", _DTYPES, ids=_DTYPE_IDS)
@pytest.mark.parametrize("mode", _MODES, ids=_MODE_IDS)
def test_rows_staged_kmeanspp(monkeypatch, mode, dtype):
    _check(monkeypatch, mode, dtype, "k-means++", False)


@pytest.mark.parametrize("dtype", _DTYPES, ids=_DTYPE_IDS)
@pytest.mark.parametrize("mode", _MODES, ids=_MODE_IDS)
def test_imported_centroids_staged(monkeypatch, mode, dtype):
    _check(monkeypatch, mode, dtype, "import", False)


@pytest.mark.parametrize("dtype", _DTYPES, ids=_DTYPE_IDS)
@pytest.mark.parametrize("mode", _MODES, ids=_MODE_IDS)
def test_weights_staged_kmeanspp(monkeypatch, mode, dtype):
    """weighted k-means++ draws from w * d: a weight that reached the wrong row moves the seeds"""
    _check(monkeypatch, mode, dtype, "k-means++", True)
    cen_w, _ = _plain(monkeypatch, mode[2], dtype == numpy.float16, "k-means++", True)
    cen_u, _ = _plain(monkeypatch, mode[2], dtype == numpy.float16, "k-means++", False)
    assert not numpy.array_equal(cen_w, cen_u)


@pytest.mark.parametrize("dtype", _DTYPES, ids=_DTYPE_IDS)
@pytest.mark.parametrize("n", [3000, 3300])
def test_random_init_copy_loop_equals_gather(monkeypatch, n, dtype):
    """init="random": three shards copy the K rows one by one from their owners, one shard gathers them in one launch"""
    _check(monkeypatch, ("host", 3, n), dtype, "random", False)
