"""New rows assigned to given centroids -- the "predict" of a trained K-means (C ABI: kmamd_kmeans_assign,
include/kmcuda_amd.h).

    centroids, _ = kmeans_cuda(train, 1024)
    assignments = kmeans_predict(rows, centroids)
    assignments, distances, (counts, distance_sums) = kmeans_predict(rows, centroids, return_distances=True,
                                                                     return_cluster_stats=True)

assignments[i] is what one kmamd_lloyd_assign pass gives row i: its nearest centroid in the reference's arithmetic,
the lowest index on a tie, never a NaN centroid -- or len(centroids), "no cluster" (what kmeans_cuda returns and
KnnIndex accepts), for a row whose first feature is NaN or whose distances are all NaN.  distances[i] is the
reference's distance of row i to that centroid (NaN without a cluster), counts[c] the number of rows of cluster c,
distance_sums[c] the float64 sum of their distances (a fixed summation order: the same bits on every call).

numpy in, numpy out (assignments / counts uint32, distances float32, distance_sums float64).  torch tensors on
`device` in, torch tensors on that device out (assignments / counts int32), with no host round trip; the call orders
with torch's work on the device (it waits for the device first and its outputs are complete when it returns).
float16 inputs select fp16x2: fp32 arithmetic on the half values, as kmeans_cuda().
"""
import os

import numpy

from . import _lib
from .api import _get_metric, _raise_for
from .knn_index import _ptr, _rows


def _check(samples, centroids, metric, device):
    metric_id = _get_metric(metric)
    if isinstance(device, bool) or not isinstance(device, (int, numpy.integer)):
        raise TypeError("\"device\" must be an integer: one device id, not kmeans_cuda's mask")
    device = int(device)
    if device < 0:
        raise ValueError("\"device\" must be a device id >= 0")
    s, fp16, n, d, on_dev = _rows(samples, "samples", device)
    c, cfp16, clusters, cd, c_dev = _rows(centroids, "centroids", device)
    if cfp16 != fp16 or c_dev != on_dev:
        raise TypeError("\"centroids\" must be of the same kind and dtype as \"samples\"")
    if cd != d:
        raise ValueError("\"centroids\" must have same number of features as \"samples\" (shape[-1])")
    if d == 0 or d > 0xFFFF:
        raise ValueError("the number of features must be in [1, 65535]")
    if clusters < 2:
        raise ValueError("\"centroids\" must have at least 2 rows")
    if clusters >= 0x7FFFFFFF or n > 0xFFFFFFFF:
        raise ValueError("too many centroids or samples")
    if fp16 and d % 2:
        raise ValueError("the number of features must be even in fp16 mode")
    return metric_id, device, s, c, fp16, n, d, clusters, on_dev


def kmeans_predict(samples, centroids, metric="L2", device=0, return_distances=False, return_cluster_stats=False,
                   verbosity=0):
    """assignments [, distances] [, (counts, distance_sums)] of the rows `samples` against `centroids` (at least 2
    rows, the kind, dtype and feature count of `samples`).  Every argument is checked before the device is touched."""
    metric_id, device, s, c, fp16, n, d, clusters, on_dev = _check(samples, centroids, metric, device)
    if on_dev:
        import torch
        dev = torch.device("cuda", device)
        asg = torch.empty((n,), dtype=torch.int32, device=dev)
        dist = torch.empty((n,), dtype=torch.float32, device=dev) if return_distances else None
        counts = torch.empty((clusters,), dtype=torch.int32, device=dev) if return_cluster_stats else None
        sums = torch.empty((clusters,), dtype=torch.float64, device=dev) if return_cluster_stats else None
    else:
        asg = numpy.empty((n,), numpy.uint32)
        dist = numpy.empty((n,), numpy.float32) if return_distances else None
        counts = numpy.empty((clusters,), numpy.uint32) if return_cluster_stats else None
        sums = numpy.empty((clusters,), numpy.float64) if return_cluster_stats else None
    rc = _lib.lib().kmamd_kmeans_assign(metric_id, n, d, clusters, device, device if on_dev else -1, int(fp16),
                                        int(verbosity), _ptr(s), _ptr(c), _ptr(asg),
                                        _ptr(dist) if dist is not None else None,
                                        _ptr(counts) if counts is not None else None,
                                        _ptr(sums) if sums is not None else None)
    _raise_for(rc, "kmamd_kmeans_assign")
    out = (asg,) + ((dist,) if return_distances else ()) + (((counts, sums),) if return_cluster_stats else ())
    return out[0] if len(out) == 1 else out


def kmeans_predict_top(samples, centroids, m, metric="L2", device=0, return_distances=True, verbosity=0):
    """(indices, distances), or indices alone, of the `m` nearest centroids of every row: (n, m) arrays, row i holding
    its qualifying centroids by (key ascending, centroid index ascending), where the key is what an assignment pass
    compares (C ABI: kmamd_kmeans_assign_top).  Column 0 is kmeans_predict's assignment.  Slots beyond
    the number of qualifying centroids -- a NaN, inf or overflowing centroid never qualifies -- and every slot of a row
    whose first feature is NaN hold len(centroids) and distance NaN.  distances are the reference's distances as
    kmeans_predict returns them (under L2 not the key: neighbouring ranks may step backwards by a last place).
    1 <= m <= min(len(centroids), 64).  Kinds and dtypes as kmeans_predict; every argument is checked before the
    device is touched."""
    metric_id, device, s, c, fp16, n, d, clusters, on_dev = _check(samples, centroids, metric, device)
    if isinstance(m, bool) or not isinstance(m, (int, numpy.integer)):
        raise TypeError("\"m\" must be an integer")
    m = int(m)
    if m < 1 or m > min(clusters, 64):
        raise ValueError("\"m\" must be in [1, min(len(centroids), 64)]")
    if fp16 and _fp16_strict():
        raise ValueError("KMCUDA_AMD_FP16_STRICT=1: the reference's half2 arithmetic has no predict form")
    if on_dev:
        import torch
        dev = torch.device("cuda", device)
        top = torch.empty((n, m), dtype=torch.int32, device=dev)
        dist = torch.empty((n, m), dtype=torch.float32, device=dev) if return_distances else None
    else:
        top = numpy.empty((n, m), numpy.uint32)
        dist = numpy.empty((n, m), numpy.float32) if return_distances else None
    rc = _lib.lib().kmamd_kmeans_assign_top(metric_id, n, d, clusters, m, device, device if on_dev else -1, int(fp16),
                                            int(verbosity), _ptr(s), _ptr(c), _ptr(top),
                                            _ptr(dist) if dist is not None else None)
    _raise_for(rc, "kmamd_kmeans_assign_top")
    return (top, dist) if return_distances else top


def _fp16_strict():
    try:
        return int(os.environ.get("KMCUDA_AMD_FP16_STRICT", "0") or 0) != 0
    except ValueError:
        return False
