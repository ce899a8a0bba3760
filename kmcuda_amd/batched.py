"""Batched K-means: many small independent problems in one call (C ABI: kmamd_kmeans_batched,
kmamd_kmeans_assign_batched, include/kmcuda_amd.h) -- product-quantiser codebooks, per-group or
per-head codebooks, one K-means per tenant.

    centroids, assignments, iterations = kmeans_batched(x, 256, init="random", layout="columns", problems=32)
    codes = kmeans_predict_batched(new_rows, centroids, layout="columns", dtype=numpy.uint8)

layout="problems": samples is (B, N, D), assignments (B, N).  layout="columns": samples is (N, B * D), problem b being
the column block [b * D, (b + 1) * D) of every row, read in place with no copy; assignments (N, B).  centroids are
(B, k, D) float32, iterations (B,).  L2 and float32 only; 1 <= D <= 64 and k <= max_clusters(D).  For every problem the
assignments are bit for bit what kmeans_predict gives for that problem's slice; a row whose first feature is NaN gets
k.  numpy in, numpy out (assignments / iterations uint32); torch tensors on `device` in, torch tensors out (int32).
Every argument is checked before the device is touched; what is out of range is refused, never routed elsewhere.
"""
import numpy

from . import _lib
from .api import _get_metric, _raise_for
from .knn_index import _is_torch, _ptr

_WIDTHS = (4, 8, 16, 32, 64)     # launch_dispatch.hpp: BatchedWidths
_PANEL_CELLS = 16384             # batched_job.cpp: kBatchedPanelCells
_LAYOUTS = {"problems": 0, "columns": 1}


def max_clusters(features):
    """The largest k of a problem with that many features (kmamd_batched_max_clusters); 0: no such width."""
    for dp in _WIDTHS:
        if 1 <= features <= dp:
            return _PANEL_CELLS // dp
    return 0


def _f32(x, name, rank, device):
    """(contiguous array-or-tensor, on_device) of a float32 operand of that rank."""
    if _is_torch(x):
        import torch
        if x.dtype == torch.float16:
            raise ValueError("\"%s\": float16 is not supported by the batched calls" % name)
        if x.dtype != torch.float32:
            raise TypeError("\"%s\" must be a float32 tensor" % name)
        if x.dim() != rank:
            raise ValueError("\"%s\" must be a %dD tensor" % (name, rank))
        if not x.is_cuda or x.device.index != device:
            raise ValueError("\"%s\" must be on device %d (or be a numpy array)" % (name, device))
        return x.contiguous(), True
    if isinstance(x, numpy.ndarray) and x.dtype == numpy.float16:
        raise ValueError("\"%s\": float16 is not supported by the batched calls" % name)
    if isinstance(x, numpy.ndarray) and x.dtype != numpy.float32:
        raise TypeError("\"%s\" must be a float32 numpy array" % name)
    try:
        arr = numpy.ascontiguousarray(x, dtype=numpy.float32)
    except (TypeError, ValueError):
        raise TypeError("\"%s\" must be a float32 numpy array" % name)
    if arr.ndim != rank:
        raise ValueError("\"%s\" must be a %dD numpy array" % (name, rank))
    return arr, False


def _problem_shape(samples, layout, problems, metric, sample_weight, device):
    """(samples, on_device, layout id, B, N, D) after every check that needs no centroids."""
    if _get_metric(metric) != 0:
        raise ValueError("the batched calls support the L2 metric only")
    if sample_weight is not None:
        raise ValueError("the batched calls take no sample weights")
    if layout not in _LAYOUTS:
        raise ValueError("\"layout\" must be \"problems\" or \"columns\"")
    if isinstance(device, bool) or not isinstance(device, (int, numpy.integer)) or device < 0:
        raise ValueError("\"device\" must be a device id >= 0")
    s, on_dev = _f32(samples, "samples", 3 if layout == "problems" else 2, int(device))
    if layout == "problems":
        b, n, d = (int(v) for v in s.shape)
        if problems is not None and int(problems) != b:
            raise ValueError("\"problems\" disagrees with samples.shape[0]")
    else:
        if problems is None:
            raise ValueError("layout=\"columns\" needs \"problems\" (or centroids that give it)")
        b, n = int(problems), int(s.shape[0])
        if b < 1 or int(s.shape[1]) % b:
            raise ValueError("samples.shape[1] must be a multiple of \"problems\"")
        d = int(s.shape[1]) // b
    if b < 1 or b > 65535:
        raise ValueError("the number of problems must be in [1, 65535]")
    if d < 1 or d > 64:
        raise ValueError("the number of features per problem must be in [1, 64]")
    if n > 0xFFFFFFFF:
        raise ValueError("too many samples")
    return s, on_dev, _LAYOUTS[layout], b, n, d


def _check_k(k, d):
    if isinstance(k, bool) or not isinstance(k, (int, numpy.integer)):
        raise TypeError("the number of clusters must be an integer")
    if k < 1 or k > max_clusters(d):
        raise ValueError("the number of clusters must be in [1, %d] at %d features" % (max_clusters(d), d))
    return int(k)


def _out(shape, np_dtype, on_dev, device):
    if not on_dev:
        return numpy.empty(shape, np_dtype)
    import torch
    tdt = {numpy.uint32: torch.int32, numpy.uint8: torch.uint8, numpy.float32: torch.float32}[np_dtype]
    return torch.empty(shape, dtype=tdt, device=torch.device("cuda", device))


def kmeans_batched(samples, k, *, init, max_iter=100, tolerance=0.0, seed=0, layout="problems", problems=None,
                   metric="L2", sample_weight=None, device=0, verbosity=0):
    """(centroids, assignments, iterations) of B independent K-means runs (module docstring).  init: a (B, k, D)
    array, or "random" -- k distinct rows per problem by the stateless hash draw keyed by (seed, problem, draw).
    A pass is one assignment pass and the update (fp64 sums in a fixed order, one rounding; an empty cluster keeps its
    bits); a problem stops after the pass in which at most tolerance * N rows changed, or after max_iter passes, on
    its own -- iterations[b] is the number of its passes.  layout="columns" needs `problems` unless init gives it."""
    given = not isinstance(init, str)
    if not given and init != "random":
        raise ValueError("\"init\" must be a (B, k, D) array or \"random\"")
    if given and problems is None and layout == "columns" and getattr(init, "ndim", 0) == 3:
        problems = int(init.shape[0])
    s, on_dev, layout_id, b, n, d = _problem_shape(samples, layout, problems, metric, sample_weight, device)
    k = _check_k(k, d)
    if k > n:
        raise ValueError("the number of clusters must not exceed the number of samples")
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, numpy.integer)) or not 1 <= max_iter <= 0xFFFFFFFF:
        raise ValueError("\"max_iter\" must be an integer >= 1")
    if not 0 <= tolerance <= 1:
        raise ValueError("\"tolerance\" must be in [0, 1]")
    if isinstance(seed, bool) or not isinstance(seed, (int, numpy.integer)) or not 0 <= seed <= 0xFFFFFFFF:
        raise ValueError("\"seed\" must be an integer in [0, 2^32)")
    cen = _out((b, k, d), numpy.float32, on_dev, device)
    if given:
        c0, c_dev = _f32(init, "init", 3, int(device))
        if c_dev != on_dev:
            raise TypeError("\"init\" must be of the same kind as \"samples\"")
        if tuple(c0.shape) != (b, k, d):
            raise ValueError("\"init\" must have the shape (problems, k, features) = %r" % ((b, k, d),))
        if on_dev:
            cen.copy_(c0)
        else:
            cen[...] = c0
    asg = _out((b, n) if layout_id == 0 else (n, b), numpy.uint32, on_dev, device)
    its = _out((b,), numpy.uint32, on_dev, device)
    rc = _lib.lib().kmamd_kmeans_batched(b, n, d, k, layout_id, 0, 0, 0 if given else 1, float(tolerance),
                                         int(max_iter), int(seed), int(device), int(device) if on_dev else -1,
                                         int(verbosity), _ptr(s), None, _ptr(cen), _ptr(asg), _ptr(its))
    _raise_for(rc, "kmamd_kmeans_batched")
    return cen, asg, its


def kmeans_predict_batched(samples, centroids, *, layout="problems", return_distances=False, dtype=numpy.uint32,
                           metric="L2", sample_weight=None, device=0, verbosity=0):
    """assignments [, distances] of one assignment pass of new rows against B given centroid sets, (B, k, D).
    dtype=numpy.uint8 with k <= 256 returns uint8 codes (a row without a cluster then gets the low byte of k: ask for
    uint32 where rows may hold NaN); distances are laid out as the assignments, NaN without a cluster."""
    problems = int(centroids.shape[0]) if getattr(centroids, "ndim", 0) == 3 else None
    s, on_dev, layout_id, b, n, d = _problem_shape(samples, layout, problems, metric, sample_weight, device)
    c, c_dev = _f32(centroids, "centroids", 3, int(device))
    if c_dev != on_dev:
        raise TypeError("\"centroids\" must be of the same kind as \"samples\"")
    if int(c.shape[0]) != b or int(c.shape[2]) != d:
        raise ValueError("\"centroids\" must have the shape (problems, k, features)")
    k = _check_k(int(c.shape[1]), d)
    dt = numpy.dtype(dtype)
    if dt not in (numpy.dtype(numpy.uint32), numpy.dtype(numpy.uint8)):
        raise TypeError("\"dtype\" must be numpy.uint32 or numpy.uint8")
    if dt == numpy.uint8 and k > 256:
        raise ValueError("uint8 codes need k <= 256")
    shape = (b, n) if layout_id == 0 else (n, b)
    asg = _out(shape, dt.type, on_dev, device)
    dist = _out(shape, numpy.float32, on_dev, device) if return_distances else None
    rc = _lib.lib().kmamd_kmeans_assign_batched(b, n, d, k, layout_id, 0, 0, int(device),
                                                int(device) if on_dev else -1, int(verbosity),
                                                int(dt == numpy.uint8), _ptr(s), _ptr(c), _ptr(asg),
                                                _ptr(dist) if dist is not None else None)
    _raise_for(rc, "kmamd_kmeans_assign_batched")
    return (asg, dist) if return_distances else asg
