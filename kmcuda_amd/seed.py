"""k-means|| seeding (Bahmani et al., "Scalable K-Means++"; C ABI: kmamd_kmeans_seed_parallel, include/kmcuda_amd.h;
DESIGN.md 6.3).

    seeds = kmeans_seed_parallel(rows, 1024)
    centroids, assignments = kmeans_cuda(rows, 1024, init=seeds)          # == kmeans_cuda(rows, 1024, init="k-means||")
    seeds, info = kmeans_seed_parallel(rows, 1024, return_candidates=True)

A handful of passes over the rows instead of k-means++'s K - 1 dependent ones: `rounds` rounds draw about
`oversampling` rows each (every row on its own, by a hash of (seed, round, row): the result does not depend on how the
rows are chunked or launched), the candidates are weighted by the rows they attract, and this library's weighted
k-means++ picks the K seeds among them.  Every seed is bit-equal to an input row.  With fewer live candidates than
clusters the seeds are plain k-means++'s (info["fell_back"]).

numpy in, numpy out; a torch tensor on `device` in, a tensor on that device out.  float16 rows select fp16x2 (fp32
arithmetic on the half values); the seeds come back in the rows' dtype.  `info` is host data either way: "rows" (the
row id of every candidate, by round, ascending within a round), "counts" (the rows each attracts; 0: a duplicate that
was dropped), "round_ends" (the number of candidates after round 0 .. rounds) and "fell_back".
"""
import ctypes
import operator

import numpy

from . import _lib
from .api import _get_metric, _raise_for, _seed_parallel_params
from .knn_index import _ptr, _rows
from .predict import _fp16_strict


def kmeans_seed_parallel(samples, clusters, rounds=5, oversampling=None, metric="L2", seed=0, device=0,
                         return_candidates=False, verbosity=0):
    """centroids, or (centroids, info).  Every argument is checked before the device is touched."""
    metric_id = _get_metric(metric)
    if isinstance(device, bool) or not isinstance(device, (int, numpy.integer)):
        raise TypeError("\"device\" must be an integer: one device id, not kmeans_cuda's mask")
    device = int(device)
    if device < 0 or device > 31:
        raise ValueError("\"device\" must be a device id in [0, 31]")
    if isinstance(clusters, (bool, float)) or not hasattr(clusters, "__index__"):
        raise TypeError("\"clusters\" must be an integer")
    clusters = operator.index(clusters)
    if isinstance(seed, (bool, float)) or not hasattr(seed, "__index__"):
        raise TypeError("\"seed\" must be an integer")
    seed = operator.index(seed) & 0xFFFFFFFF
    rounds, ell = _seed_parallel_params(rounds, oversampling)
    s, fp16, n, d, on_dev = _rows(samples, "samples", device)
    if d == 0 or d > 0xFFFF:
        raise ValueError("the number of features must be in [1, 65535]")
    if n > 0xFFFFFFFF:
        raise ValueError("too many samples")
    if clusters < 2 or clusters > n:
        raise ValueError("\"clusters\" must be in [2, len(samples)]")
    if fp16 and d % 2:
        raise ValueError("the number of features must be even in fp16 mode")
    if fp16 and _fp16_strict():
        raise ValueError("KMCUDA_AMD_FP16_STRICT=1: the reference's half2 arithmetic has no k-means|| form")
    n_rounds = rounds if rounds else 5
    if on_dev:
        import torch
        cen = torch.empty((clusters, d), dtype=s.dtype, device=torch.device("cuda", device))
    else:
        cen = numpy.empty((clusters, d), numpy.float16 if fp16 else numpy.float32)
    total = ctypes.c_uint32(0)
    fell = ctypes.c_int32(0)
    ends = numpy.zeros(n_rounds + 1, numpy.uint32)
    # the candidates: about 1 + rounds * oversampling of them (no cap).  The call is deterministic, so a list that
    # turns out too short is fetched by calling again with room for all of them.
    expect = 1.0 + n_rounds * (ell if ell else 2.0 * clusters)
    capacity = int(min(n, 2.0 * expect + 1024)) if return_candidates else 0
    while True:
        rows = numpy.zeros(capacity, numpy.uint32)
        counts = numpy.zeros(capacity, numpy.uint32)
        rc = _lib.lib().kmamd_kmeans_seed_parallel(
            metric_id, n, d, clusters, rounds, ell, seed, device, device if on_dev else -1, int(fp16), int(verbosity),
            _ptr(s), _ptr(cen), rows.ctypes.data if capacity else None, counts.ctypes.data if capacity else None,
            capacity, ctypes.cast(ctypes.byref(total), ctypes.c_void_p), ends.ctypes.data,
            ctypes.cast(ctypes.byref(fell), ctypes.c_void_p))
        _raise_for(rc, "kmamd_kmeans_seed_parallel")
        if not return_candidates or total.value <= capacity:
            break
        capacity = total.value
    if not return_candidates:
        return cen
    info = {"rows": rows[:total.value].copy(), "counts": counts[:total.value].copy(), "round_ends": ends,
            "fell_back": bool(fell.value)}
    return cen, info
