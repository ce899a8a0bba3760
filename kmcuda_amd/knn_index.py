"""k nearest neighbours of NEW rows (queries) among a clustered corpus (C ABI: kmamd_knn_index_*, include/kmcuda_amd.h).

knn_cuda() is the self-join of the corpus: every row's neighbours among the OTHER rows.  A KnnIndex prepares the
corpus once -- the same cluster-sorted copies, radii and centroid distances knn_cuda() builds -- and answers query
batches against it on the same search kernels:

    index = KnnIndex(samples, centroids, assignments, metric="L2", device=0)
    neighbors, distances = index.query(queries, k)
    index.close()

or, once, knn_query(k, samples, centroids, assignments, queries).  index.query_radius(queries, radius) /
knn_query_radius(...) answer the other question, "which rows lie within distance r", as a CSR (offsets, neighbors,
distances) -- the brute-force set, not the outcome of a visiting procedure.  A query's list is what the reference's procedure
gives for it as one more row of its cluster (its nearest centroid unless `query_assignments` says otherwise), WITHOUT
skipping anything: own cluster first, then the others in ascending id under the triangle prune.

Multi-probe (approximate) search, DESIGN.md 4.12: index.query(queries, k, nprobe=p) looks only at every query's p
nearest clusters (kmeans_predict_top's ranking, by the same kernels), index.query(queries, k, probes=P) at the clusters
the caller names (Q x p; column 0 is the query's own cluster, K is a filler).  The list is exactly what the procedure
above yields when a cluster outside the probe set is never visited: reproducible, and equal to the exact list at p = K.
return_probes appends the lists used.

Rows can be added in place, DESIGN.md 4.15: index.add(rows) (clusters by kmeans_predict on the index's centroids) or
index.add(rows, assignments) returns the id of rows[0]; the new rows take the ids n_rows, n_rows + 1, ... and the index
then answers every query exactly -- indices and distance bits -- as KnnIndex(old rows + new rows, centroids, ...) would.
index.info() is (n_rows, n_clustered, filter): filter 2 the f16 matrix-core filter, 1 the f32 one, 0 the exact search.

Rows can be removed in place, DESIGN.md 4.16: index.remove(ids) returns how many rows lost their cluster; they are never
returned again and the index then answers every query exactly -- indices and distance bits -- as KnnIndex(rows,
centroids, assignments with assignments[ids] = K) would.  Ids are stable: n_rows does not change, memory is not reclaimed
(the rows move to the no-cluster tail; no compaction, no reuse of ids), and an index that has left the f16 filter stays
where it is.  index.radii() reads the clusters' radii (a window for tests).

Filtered search, DESIGN.md 4.17: index.query(queries, k, allow=mask) answers the batch over a subset of the corpus --
mask is one flag per row id (n_rows of them, bool or uint8, on the queries' side); the lists are exactly -- indices and
distance bits -- those of KnnIndex(rows, centroids, assignments with assignments[~mask] = K), for this call only: the
index is not modified, and the next call may bring another mask.  It composes with nprobe / probes.  query_radius takes
no mask; query_radius_allow(queries, radius, mask) is the masked radius search: query_radius's result
with the denied rows struck out, bit for bit, and knn_query_radius(..., allow=mask) its one-shot form.

Capped search, DESIGN.md 4.19: index.query(queries, k, max_distance=r) returns the k nearest rows WITHIN distance r --
the same procedure reading min(kth, r) wherever it reads kth, so the cap prunes from the first candidate on instead of
being applied to a finished list.  The real entries (distance <= r, inclusive) come first, the remaining slots hold
index 0 at FLT_MAX; return_counts=True appends the number of real entries per query.  r = inf (or FLT_MAX) returns the
bits of the call without a cap.  It composes with query_assignments, nprobe / probes, allow and every return_* flag.

numpy in, numpy out (neighbors uint32, distances float32, assignments uint32).  torch tensors on the index's device
in, torch tensors on that device out (neighbors / assignments int32: 0xFFFFFFFF reads -1), with no host round trip;
the call orders with torch's work on the device (it waits for the device first and its outputs are complete when
it returns).  float16 inputs select fp16x2: fp32 arithmetic on the half values, as knn_cuda().
"""
import ctypes
import os

import numpy

from . import _lib
from ._lib import u32
from .api import _get_metric, _raise_for


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _rows(x, name, device=None):
    """(array-or-tensor, fp16, rows, features, on_device) for a 2-D float32 / float16 operand."""
    if _is_torch(x):
        import torch
        if x.dtype not in (torch.float32, torch.float16):
            raise TypeError("\"%s\" must be a 2D float32 or float16 tensor" % name)
        if x.dim() != 2:
            raise ValueError("\"%s\" must be a 2D tensor" % name)
        if not x.is_cuda:
            raise ValueError("\"%s\" must be on a GPU (or be a numpy array)" % name)
        if device is not None and x.device.index != device:
            raise ValueError("\"%s\" must be on device %d" % (name, device))
        return x.contiguous(), x.dtype == torch.float16, int(x.shape[0]), int(x.shape[1]), True
    if isinstance(x, numpy.ndarray) and x.dtype == numpy.float16:
        arr, fp16 = numpy.ascontiguousarray(x), True
    else:
        if isinstance(x, numpy.ndarray) and x.dtype != numpy.float32:
            raise TypeError("\"%s\" must be a 2D float32 or float16 numpy array" % name)
        try:
            arr = numpy.ascontiguousarray(x, dtype=numpy.float32)
        except (TypeError, ValueError):
            raise TypeError("\"%s\" must be a 2D float32 or float16 numpy array" % name)
        fp16 = False
    if arr.ndim != 2:
        raise ValueError("\"%s\" must be a 2D numpy array" % name)
    return arr, fp16, int(arr.shape[0]), int(arr.shape[1]), False


def _labels(x, n, name, clusters=None, device=None):
    """1-D cluster ids of length n (uint32 numpy / int32 tensor); with `clusters`: every id must be below it."""
    if _is_torch(x):
        import torch
        if x.dtype.is_floating_point or x.dtype == torch.bool:
            raise TypeError("\"%s\" must be a 1D integer tensor" % name)
        if x.dim() != 1:
            raise ValueError("\"%s\" must be a 1D tensor" % name)
        if x.shape[0] != n:
            raise ValueError("\"%s\" must have one entry per row (%d)" % (name, n))
        if not x.is_cuda or (device is not None and x.device.index != device):
            raise ValueError("\"%s\" must be on the index's device" % name)
        if clusters is not None and n and bool(((x < 0) | (x >= clusters)).any()):
            raise ValueError("\"%s\" must hold cluster ids in [0, %d)" % (name, clusters))
        return x.to(torch.int32).contiguous(), True
    if isinstance(x, numpy.ndarray) and x.dtype.kind not in "iu":
        raise TypeError("\"%s\" must be a 1D integer numpy array" % name)
    arr = numpy.asarray(x)
    if arr.ndim != 1:
        raise ValueError("\"%s\" must be a 1D numpy array" % name)
    if arr.shape[0] != n:
        raise ValueError("\"%s\" must have one entry per row (%d)" % (name, n))
    if clusters is not None and n and (arr.min() < 0 or arr.max() >= clusters):
        raise ValueError("\"%s\" must hold cluster ids in [0, %d)" % (name, clusters))
    return numpy.ascontiguousarray(arr, dtype=numpy.uint32), False


def _check_corpus(samples, centroids, assignments, device):
    s, fp16, n, d, on_dev = _rows(samples, "samples", device)
    c, cfp16, clusters, cd, c_dev = _rows(centroids, "centroids", device)
    if cfp16 != fp16 or c_dev != on_dev:
        raise TypeError("\"centroids\" must be of the same kind and dtype as \"samples\"")
    if cd != d:
        raise ValueError("\"centroids\" must have same number of features as \"samples\" (shape[-1])")
    if n == 0 or d == 0:
        raise ValueError("\"samples\" must not be empty")
    if clusters < 1:
        raise ValueError("\"centroids\" must not be empty")
    if fp16 and d % 2:
        raise ValueError("the number of features must be even in fp16 mode")
    if _is_torch(assignments) != on_dev:
        raise TypeError("\"assignments\" must be of the same kind as \"samples\" (numpy array or torch tensor)")
    a, _ = _labels(assignments, n, "assignments", None, device)
    return s, c, a, fp16, n, d, clusters, on_dev


def _check_k(k, n):
    if isinstance(k, bool) or not isinstance(k, (int, numpy.integer)):
        raise TypeError("\"k\" must be an integer")
    k = int(k)
    if k < 1 or k > min(n, 0xFFFF):
        raise ValueError("\"k\" must be in [1, min(number of samples, 65535)] = [1, %d]" % min(n, 0xFFFF))
    return k


def _check_queries(queries, fp16, d, clusters, query_assignments, device):
    q, qfp16, nq, qd, q_dev = _rows(queries, "queries", device)
    if qfp16 != fp16:
        raise TypeError("\"queries\" must have the dtype of \"samples\"")
    if qd != d:
        raise ValueError("\"queries\" must have same number of features as \"samples\" (shape[-1])")
    qa = None
    if query_assignments is not None:
        if _is_torch(query_assignments) != q_dev:
            raise TypeError("\"query_assignments\" must be of the same kind as \"queries\"")
        qa, _ = _labels(query_assignments, nq, "query_assignments", clusters, device)
    return q, nq, q_dev, qa


PROBE_MAX = 64   # the widest probe list (kmamd_knn_index_query_probe)


def _fp16_strict():
    try:
        return int(os.environ.get("KMCUDA_AMD_FP16_STRICT", "0") or 0) != 0
    except ValueError:
        return False


def _check_probes(nprobe, probes, nq, clusters, q_dev, query_assignments, device, fp16=False):
    """(nprobe, probes or None) of a probed query, or (None, None): the exact one."""
    if nprobe is None and probes is None:
        return None, None
    if probes is None and fp16 and _fp16_strict():
        raise ValueError("KMCUDA_AMD_FP16_STRICT=1: the reference's half2 arithmetic has no ranking of the centroids "
                         "(kmeans_predict_top refuses it too): pass \"probes\"")
    if query_assignments is not None:
        raise ValueError("\"query_assignments\" cannot be combined with \"nprobe\" / \"probes\": column 0 of the probe "
                         "list is the query's own cluster")
    if nprobe is not None:
        if isinstance(nprobe, bool) or not isinstance(nprobe, (int, numpy.integer)):
            raise TypeError("\"nprobe\" must be an integer")
        nprobe = int(nprobe)
    p = None
    if probes is not None:
        if _is_torch(probes) != q_dev:
            raise TypeError("\"probes\" must be of the same kind as \"queries\" (numpy array or torch tensor)")
        if _is_torch(probes):
            import torch
            if probes.dtype.is_floating_point or probes.dtype == torch.bool:
                raise TypeError("\"probes\" must be a 2D integer tensor")
            if probes.dim() != 2:
                raise ValueError("\"probes\" must be a 2D tensor (queries x nprobe)")
            if not probes.is_cuda or probes.device.index != device:
                raise ValueError("\"probes\" must be on the index's device")
            shape = tuple(int(v) for v in probes.shape)
            out_of_range = bool(shape[0] and shape[1] and bool(((probes < 0) | (probes > clusters)).any()))
            p = probes.to(torch.int32).contiguous()
        else:
            if not isinstance(probes, numpy.ndarray):
                probes = numpy.asarray(probes)
            if probes.dtype.kind not in "iu":
                raise TypeError("\"probes\" must be a 2D integer numpy array")
            if probes.ndim != 2:
                raise ValueError("\"probes\" must be a 2D numpy array (queries x nprobe)")
            shape = probes.shape
            out_of_range = bool(probes.size and (probes.min() < 0 or probes.max() > clusters))
            p = numpy.ascontiguousarray(probes, dtype=numpy.uint32) if not out_of_range else None
        if shape[0] != nq:
            raise ValueError("\"probes\" must have one row per query (%d)" % nq)
        if nprobe is None:
            nprobe = int(shape[1])
        elif nprobe != shape[1]:
            raise ValueError("\"nprobe\" (%d) must equal the width of \"probes\" (%d)" % (nprobe, shape[1]))
        if out_of_range:
            raise ValueError("\"probes\" must hold cluster ids in [0, %d] (%d: no cluster)" % (clusters, clusters))
    if nprobe < 1 or nprobe > min(clusters, PROBE_MAX):
        raise ValueError("\"nprobe\" must be in [1, min(number of clusters, %d)] = [1, %d]"
                         % (PROBE_MAX, min(clusters, PROBE_MAX)))
    if p is not None and nq:
        col0 = p[:, 0]
        if bool((col0 >= clusters).any()):
            raise ValueError("column 0 of \"probes\" (the query's own cluster) must be below %d" % clusters)
    return nprobe, p


def _check_allow(allow, n_rows, q_dev, device):
    """The allow-mask of a masked query as contiguous uint8 (numpy array / tensor on the index's device), or None."""
    if allow is None:
        return None
    if _is_torch(allow):
        import torch
        if not q_dev:
            raise TypeError("\"allow\" must be of the same kind as \"queries\" (numpy array or torch tensor)")
        if allow.dtype not in (torch.bool, torch.uint8):
            raise TypeError("\"allow\" must be a 1D bool or uint8 tensor")
        if allow.dim() != 1:
            raise ValueError("\"allow\" must be a 1D tensor")
        if not allow.is_cuda or allow.device.index != device:
            raise ValueError("\"allow\" must be on the index's device")
        if allow.shape[0] != n_rows:
            raise ValueError("\"allow\" must have one flag per row of the index (%d)" % n_rows)
        allow = allow.contiguous()
        return allow.view(torch.uint8) if allow.dtype == torch.bool else allow
    if not isinstance(allow, numpy.ndarray) or allow.dtype not in (numpy.bool_, numpy.uint8):
        raise TypeError("\"allow\" must be a 1D bool or uint8 numpy array")
    if q_dev:
        raise TypeError("\"allow\" must be of the same kind as \"queries\" (numpy array or torch tensor)")
    if allow.ndim != 1:
        raise ValueError("\"allow\" must be a 1D numpy array")
    if allow.shape[0] != n_rows:
        raise ValueError("\"allow\" must have one flag per row of the index (%d)" % n_rows)
    return numpy.ascontiguousarray(allow).view(numpy.uint8)


def _check_radius(radius):
    if isinstance(radius, bool) or not isinstance(radius, (int, float, numpy.integer, numpy.floating)):
        raise TypeError("\"radius\" must be a real number")
    try:
        with numpy.errstate(over="ignore"):
            r = numpy.float32(radius)
    except OverflowError:
        r = numpy.float32(numpy.inf)
    if not numpy.isfinite(r) or r < 0:
        raise ValueError("\"radius\" must be finite in float32 and >= 0")
    return float(r)


FLT_MAX = float(numpy.finfo(numpy.float32).max)


def _check_max_distance(max_distance):
    """The cap of a capped query as a Python float that is exact in float32 (inf: FLT_MAX), or None: no cap."""
    if max_distance is None:
        return None
    if hasattr(max_distance, "ndim") and not isinstance(max_distance, numpy.generic):   # a 0-d array or tensor
        if max_distance.ndim != 0:
            raise TypeError("\"max_distance\" must be a real number")
        max_distance = max_distance.item()
    if isinstance(max_distance, bool) or not isinstance(max_distance, (int, float, numpy.integer, numpy.floating)):
        raise TypeError("\"max_distance\" must be a real number")
    with numpy.errstate(over="ignore"):
        r = numpy.float32(max_distance)
    if numpy.isnan(r) or r < 0:
        raise ValueError("\"max_distance\" must not be NaN and must be >= 0")
    return min(float(r), FLT_MAX)


def _real_counts(dist, cap):
    """Per query, the entries of its list that are rows: distance <= cap (no cap: < FLT_MAX); NaN rows count 0."""
    real = dist <= cap if cap is not None else dist < FLT_MAX
    if _is_torch(dist):
        import torch
        return real.sum(dim=1, dtype=torch.int32)
    return real.sum(axis=1).astype(numpy.uint32)


def _check_radius_flags(return_distances, sort, count_only):
    if sort and not count_only and not return_distances:
        raise ValueError("\"sort\" orders by distance: it needs return_distances=True")


def _sort_slices(offsets, neighbors, distances):
    """Every query's slice reordered by (distance, row index)."""
    if _is_torch(neighbors):
        import torch
        if neighbors.numel() == 0:
            return neighbors, distances
        q = torch.repeat_interleave(torch.arange(offsets.numel() - 1, device=neighbors.device), offsets[1:] - offsets[:-1])
        order = torch.argsort(neighbors.to(torch.int64) & 0xFFFFFFFF, stable=True)
        order = order[torch.argsort(distances[order], stable=True)]
        order = order[torch.argsort(q[order], stable=True)]
        return neighbors[order], distances[order]
    q = numpy.repeat(numpy.arange(len(offsets) - 1), numpy.diff(offsets))
    order = numpy.lexsort((neighbors, distances, q))
    return neighbors[order], distances[order]


def _ptr(x):
    return ctypes.c_void_p(x.data_ptr() if _is_torch(x) else x.ctypes.data)


def _opt_ptr(x):
    return _ptr(x) if x is not None else None


class KnnIndex:
    """A corpus prepared for k-NN queries on one GPU (kmamd_knn_index_create)."""

    def __init__(self, samples, centroids, assignments, metric="L2", device=0, verbosity=0):
        metric_id = _get_metric(metric)
        s, c, a, fp16, n, d, clusters, on_dev = _check_corpus(samples, centroids, assignments, device)
        self.n_rows, self.features, self.clusters, self.fp16 = n, d, clusters, fp16
        self.metric, self.device = metric, int(device)
        self.lib = _lib.lib()
        h = ctypes.c_void_p()
        rc = self.lib.kmamd_knn_index_create(ctypes.byref(h), self.device, metric_id, int(fp16), n, d, clusters,
                                             _ptr(s), _ptr(c), _ptr(a), self.device if on_dev else -1, int(verbosity))
        _raise_for(rc, "kmamd_knn_index_create")
        self.h = h

    def query(self, queries, k, query_assignments=None, return_distances=True, return_assignments=False,
              nprobe=None, probes=None, return_probes=False, allow=None, max_distance=None, return_counts=False):
        """The k nearest corpus rows of every query row: neighbors (Q x k corpus row indices), then, as asked,
        distances (Q x k float32, the exact distances the search compared) and the queries' clusters (Q).
        nprobe / probes: the multi-probe search (module docstring) -- only the clusters of every
        query's probe list are visited; return_assignments is then column 0 of the lists and return_probes appends the
        Q x nprobe lists used (uint32 numpy / int32 tensor, K where fewer qualify).
        allow: the filtered search (module docstring) -- one flag per row of the index (n_rows; 1-D
        bool / uint8, numpy or a tensor on the index's device, as the queries are); only rows whose flag is set are
        returned, exactly as by a fresh index on which every other row has lost its cluster.  Composes with nprobe /
        probes and every return_* flag; the queries' clusters and computed probe lists do not depend on it.
        max_distance: the capped search (module docstring) -- a real number r >= 0 (inf: no cap); the
        k nearest rows within r, by the same procedure reading min(kth, r) for kth.  The real entries (distance <= r)
        come first; the slots behind them hold index 0 at FLT_MAX.  Composes with everything above.
        return_counts: appends, last, the number of real entries per query (uint32 numpy / int32 tensor) -- entries
        with distance <= r, or < FLT_MAX without a cap; 0 for a query with a NaN or inf feature."""
        if not getattr(self, "h", None):
            raise ValueError("the index is closed")
        k = _check_k(k, self.n_rows)
        cap = _check_max_distance(max_distance)
        want_distances = return_distances
        return_distances = return_distances or return_counts   # (the counts are made from the distances)
        q, nq, q_dev, qa = _check_queries(queries, self.fp16, self.features, self.clusters, query_assignments,
                                          self.device)
        nprobe, pr = _check_probes(nprobe, probes, nq, self.clusters, q_dev, query_assignments, self.device, self.fp16)
        al = _check_allow(allow, self.n_rows, q_dev, self.device)
        probed = nprobe is not None
        if return_probes and not probed:
            raise ValueError("\"return_probes\" needs \"nprobe\" or \"probes\"")
        nb = self._out((nq, k), "u", q_dev)
        dist = self._out((nq, k), "f", q_dev) if return_distances else None
        # the lists of the call: the probe lists (in: the caller's, out: those used), or the queries' clusters
        if probed:
            lists_in = pr
            lists_out = self._out((nq, nprobe), "u", q_dev) if return_assignments or return_probes else None
        else:
            lists_in = qa
            lists_out = self._out((nq,), "u", q_dev) if return_assignments else None
        if nq:
            # (the capped entry points print the KMCUDA_AMD_KNN_STATS line the uncapped query does not: never for cap=None)
            name = "kmamd_knn_index_query_probe" if probed else "kmamd_knn_index_query"
            entry = name + ("_allow" if cap is None else "_capped")
            args = [self.h, k] + ([] if cap is None else [cap]) + ([nprobe] if probed else [])
            args += [nq, _ptr(q), _opt_ptr(lists_in), _ptr(nb), _opt_ptr(dist), _opt_ptr(lists_out),
                     self.device if q_dev else -1, _opt_ptr(al)]
            _raise_for(getattr(self.lib, entry)(*args), name if cap is None else entry)
        out = (nb,) + ((dist,) if return_distances else ())
        if probed:
            if return_assignments:
                col0 = lists_out[:, 0]
                out += ((col0.contiguous() if q_dev else numpy.ascontiguousarray(col0)),)
            if return_probes:
                out += (lists_out,)
        elif return_assignments:
            out += (lists_out,)
        return self._with_counts(out[0] if len(out) == 1 else out, want_distances, return_counts, cap)

    def _out(self, shape, kind, on_dev, zeros=False):
        """An output array of a call on the side its inputs are on: a tensor on the index's device (kind "u", row ids,
        cluster ids and counts: int32; "f": float32) or a numpy array (uint32 / float32)."""
        if on_dev:
            import torch
            make = torch.zeros if zeros else torch.empty
            return make(shape, dtype=torch.int32 if kind == "u" else torch.float32,
                        device=torch.device("cuda", self.device))
        return (numpy.zeros if zeros else numpy.empty)(shape, numpy.uint32 if kind == "u" else numpy.float32)

    @staticmethod
    def _with_counts(out, want_distances, return_counts, cap):
        """`out` of a query that fetched the distances (at [1]) for the counts: the counts appended, the distances
        dropped again if the caller did not ask for them."""
        if not return_counts:
            return out
        out = out + (_real_counts(out[1], cap),)
        if not want_distances:
            out = out[:1] + out[2:]
        return out

    def query_radius(self, queries, radius, query_assignments=None, return_distances=True, sort=False,
                     count_only=False):
        """The corpus rows within `radius` of every query row: the brute-force set over the rows that
        have a cluster, by the exact distance query() returns.  count_only: counts (Q).  Else (offsets, neighbors[,
        distances]): offsets int64 of Q + 1 entries, neighbors / distances flat of length offsets[-1], query i owning
        [offsets[i]:offsets[i + 1]] in ascending (cluster id, row index) order, or by (distance, row index) with sort.
        The search runs twice, once to count and once to fill; the queries' clusters are computed once."""
        return self._query_radius(queries, radius, None, False, query_assignments, return_distances, sort, count_only)

    def query_radius_allow(self, queries, radius, allow, query_assignments=None, return_distances=True, sort=False,
                           count_only=False):
        """query_radius over the rows the mask allows: allow is one flag per row of the index (n_rows;
        1-D bool / uint8, numpy or a tensor on the index's device, as the queries are), and the result is exactly
        query_radius's -- the same return value, bit for bit -- with the denied rows struck out; equally, what a fresh
        index on which every denied row has lost its cluster returns.  The index is not modified.  The count and the
        fill each prepare the mask (two stateless calls)."""
        return self._query_radius(queries, radius, allow, True, query_assignments, return_distances, sort, count_only)

    def _query_radius(self, queries, radius, allow, masked, query_assignments, return_distances, sort, count_only):
        if not getattr(self, "h", None):
            raise ValueError("the index is closed")
        r = _check_radius(radius)
        _check_radius_flags(return_distances, sort, count_only)
        q, nq, q_dev, qa = _check_queries(queries, self.fp16, self.features, self.clusters, query_assignments,
                                          self.device)
        al = _check_allow(allow, self.n_rows, q_dev, self.device)
        if masked and al is None:
            raise TypeError("\"allow\" must be a 1D bool or uint8 numpy array or tensor")
        alp = _opt_ptr(al)
        dptr = self.device if q_dev else -1
        counts = self._out((nq,), "u", q_dev, zeros=True)
        asg = self._out((nq,), "u", q_dev) if qa is None else None
        if nq:
            rc = self.lib.kmamd_knn_index_radius_count_allow(self.h, r, nq, _ptr(q), _opt_ptr(qa), _ptr(counts),
                                                             _opt_ptr(asg), dptr, alp)
            _raise_for(rc, "kmamd_knn_index_radius_count_allow" if masked else "kmamd_knn_index_radius_count")
        if count_only:
            return counts
        if qa is None:
            qa = asg   # the fill groups the queries as the count did
        if q_dev:
            import torch
            offsets = torch.zeros((nq + 1,), dtype=torch.int64, device=counts.device)
            # (a count reads as a negative int32 from 2^31 on)
            torch.cumsum(counts.to(torch.int64) & 0xFFFFFFFF, 0, out=offsets[1:])
        else:
            offsets = numpy.zeros((nq + 1,), numpy.int64)
            numpy.cumsum(counts, out=offsets[1:])
        total = int(offsets[-1])   # (from the device: the one value that reaches the host)
        nb = self._out((total,), "u", q_dev)
        dist = self._out((total,), "f", q_dev) if return_distances else None
        if nq and total:
            rc = self.lib.kmamd_knn_index_radius_fill_allow(self.h, r, nq, _ptr(q), _ptr(qa), _ptr(offsets), _ptr(nb),
                                                            _opt_ptr(dist), dptr, alp)
            _raise_for(rc, "kmamd_knn_index_radius_fill_allow" if masked else "kmamd_knn_index_radius_fill")
        if sort:
            nb, dist = _sort_slices(offsets, nb, dist)
        return (offsets, nb, dist) if return_distances else (offsets, nb)

    def add(self, rows, assignments=None, return_assignments=False):
        """Adds `rows` (n x features, the kind and dtype rules of query()) to the index in place and returns the id of
        rows[0] -- the rows get the ids n_rows, n_rows + 1, ... -- or (that id, the rows' clusters) with
        return_assignments.  assignments: one cluster id per row (an id >= the number of clusters: the row has no
        cluster and is never returned, but takes an id); None: kmeans_predict(rows, the index's centroids).  The
        index then equals KnnIndex(old rows + rows, ...) bit for bit in every query.  Not safe against
        a concurrent call on the same index."""
        if not getattr(self, "h", None):
            raise ValueError("the index is closed")
        r, fp16, n, d, on_dev = _rows(rows, "rows", self.device)
        if fp16 != self.fp16:
            raise TypeError("\"rows\" must have the dtype of \"samples\"")
        if d != self.features:
            raise ValueError("\"rows\" must have same number of features as \"samples\" (shape[-1])")
        a = None
        if assignments is not None:
            if _is_torch(assignments) != on_dev:
                raise TypeError("\"assignments\" must be of the same kind as \"rows\" (numpy array or torch tensor)")
            a, _ = _labels(assignments, n, "assignments", None, self.device)
        elif self.fp16 and _fp16_strict():
            raise ValueError("KMCUDA_AMD_FP16_STRICT=1: the reference's half2 arithmetic has no assignment pass "
                             "(kmeans_predict refuses it too): pass \"assignments\"")
        if self.n_rows + n > 0xFFFFFFFE:
            raise ValueError("an index holds at most 0xFFFFFFFE rows")
        out = self._out((n,), "u", on_dev) if return_assignments else None
        first = u32(self.n_rows)
        rc = self.lib.kmamd_knn_index_add(self.h, n, _ptr(r), _opt_ptr(a), _opt_ptr(out), ctypes.byref(first),
                                          self.device if on_dev else -1)
        _raise_for(rc, "kmamd_knn_index_add")
        self.n_rows += n
        return (int(first.value), out) if return_assignments else int(first.value)

    def remove(self, ids):
        """Removes the rows `ids` (a 1-D integer numpy array or sequence, or an integer tensor on the index's device;
        independent of how the corpus was passed) from every later search and returns how many rows lost their cluster:
        an id without a cluster (removed before, or given as >= the number of clusters) is allowed and changes nothing, a
        repeated id counts once.  The rows keep their ids and n_rows does not change; memory is not reclaimed.  The
        index then equals KnnIndex(rows, centroids, assignments with those ids set to the number of clusters) bit for
        bit in every query.  One pass over the whole index, whatever len(ids).  Not safe against a
        concurrent call on the same index."""
        if not getattr(self, "h", None):
            raise ValueError("the index is closed")
        if _is_torch(ids):
            import torch
            if ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool:
                raise TypeError("\"ids\" must be a 1D integer tensor")
            if ids.dim() != 1:
                raise ValueError("\"ids\" must be a 1D tensor")
            if not ids.is_cuda or ids.device.index != self.device:
                raise ValueError("\"ids\" must be on the index's device (or be a numpy array)")
            n = int(ids.shape[0])
            if n and bool(((ids < 0) | (ids >= self.n_rows)).any()):
                raise ValueError("\"ids\" must hold row ids in [0, %d)" % self.n_rows)
            arr, on_dev = ids.to(torch.int32).contiguous(), True   # (an id from 2^31 on keeps its 32 bits)
        else:
            arr = ids if isinstance(ids, numpy.ndarray) else numpy.asarray(ids)
            if arr.size == 0 and not isinstance(ids, numpy.ndarray):
                arr = arr.astype(numpy.uint32)   # (an empty list has no dtype of its own)
            if arr.dtype.kind not in "iu":
                raise TypeError("\"ids\" must be a 1D integer numpy array or sequence")
            if arr.ndim != 1:
                raise ValueError("\"ids\" must be a 1D numpy array or sequence")
            n = int(arr.shape[0])
            if n and (arr.min() < 0 or arr.max() >= self.n_rows):
                raise ValueError("\"ids\" must hold row ids in [0, %d)" % self.n_rows)
            arr, on_dev = numpy.ascontiguousarray(arr, dtype=numpy.uint32), False
        lost = u32(0)
        rc = self.lib.kmamd_knn_index_remove(self.h, n, _ptr(arr) if n else None, ctypes.byref(lost),
                                             self.device if on_dev else -1)
        _raise_for(rc, "kmamd_knn_index_remove")
        return int(lost.value)

    def radii(self):
        """The clusters' radii as the searches' prune reads them: numpy float32 (clusters,), NaN for a cluster without
        rows.  A window for tests (a stale radius would only loosen the prune, never change a result)."""
        if not getattr(self, "h", None):
            raise ValueError("the index is closed")
        out = numpy.empty((self.clusters,), numpy.float32)
        rc = self.lib.kmamd_knn_index_radii(self.h, _ptr(out))
        _raise_for(rc, "kmamd_knn_index_radii")
        return out

    def radii_allow(self, allow):
        """The radii a query with the mask `allow` (a numpy mask, or a tensor on the index's device) prunes with: over
        the allowed rows, NaN for a cluster without one -- radii() of the fresh index the masked call is defined by.
        numpy float32 (clusters,).  A window for tests, as radii()."""
        if not getattr(self, "h", None):
            raise ValueError("the index is closed")
        on_dev = _is_torch(allow)
        al = _check_allow(allow, self.n_rows, on_dev, self.device)
        if al is None:
            raise TypeError("\"allow\" must be a 1D bool or uint8 numpy array or tensor")
        out = numpy.empty((self.clusters,), numpy.float32)
        rc = self.lib.kmamd_knn_index_radii_allow(self.h, _ptr(al), self.device if on_dev else -1, _ptr(out))
        _raise_for(rc, "kmamd_knn_index_radii_allow")
        return out

    def info(self):
        """(n_rows, n_clustered, filter): the rows of the index, those of them that have a cluster, and the search it
        runs -- 2: the f16 matrix-core filter, 1: the f32 one, 0: every candidate evaluated exactly."""
        if not getattr(self, "h", None):
            raise ValueError("the index is closed")
        n, nc, f = u32(0), u32(0), ctypes.c_int(0)
        rc = self.lib.kmamd_knn_index_info(self.h, ctypes.byref(n), ctypes.byref(nc), ctypes.byref(f))
        _raise_for(rc, "kmamd_knn_index_info")
        return int(n.value), int(nc.value), int(f.value)

    def close(self):
        if getattr(self, "h", None):
            self.lib.kmamd_knn_index_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def knn_query(k, samples, centroids, assignments, queries, metric="L2", device=0, query_assignments=None,
              return_distances=True, return_assignments=False, verbosity=0, nprobe=None, probes=None,
              return_probes=False, allow=None, max_distance=None, return_counts=False):
    """One-shot KnnIndex(samples, centroids, assignments, metric, device).query(queries, k, ...): every argument is
    checked before the device is touched."""
    _get_metric(metric)
    _check_max_distance(max_distance)
    _, _, _, fp16, n, d, clusters, _ = _check_corpus(samples, centroids, assignments, device)
    _check_k(k, n)
    _, nq, q_dev, _ = _check_queries(queries, fp16, d, clusters, query_assignments, device)
    np_, _ = _check_probes(nprobe, probes, nq, clusters, q_dev, query_assignments, device, fp16)
    if np_ is None and return_probes:
        raise ValueError("\"return_probes\" needs \"nprobe\" or \"probes\"")
    _check_allow(allow, n, q_dev, device)
    with KnnIndex(samples, centroids, assignments, metric=metric, device=device, verbosity=verbosity) as ix:
        return ix.query(queries, k, query_assignments=query_assignments, return_distances=return_distances,
                        return_assignments=return_assignments, nprobe=nprobe, probes=probes,
                        return_probes=return_probes, allow=allow, max_distance=max_distance,
                        return_counts=return_counts)


def knn_query_radius(radius, samples, centroids, assignments, queries, metric="L2", device=0, query_assignments=None,
                     return_distances=True, sort=False, count_only=False, verbosity=0, allow=None):
    """One-shot KnnIndex(samples, centroids, assignments, metric, device).query_radius(queries, radius, ...), or with
    allow= (one flag per sample) .query_radius_allow(queries, radius, allow, ...): every argument is checked before the
    device is touched."""
    _get_metric(metric)
    _, _, _, fp16, n, d, clusters, _ = _check_corpus(samples, centroids, assignments, device)
    _check_radius(radius)
    _check_radius_flags(return_distances, sort, count_only)
    _, _, q_dev, _ = _check_queries(queries, fp16, d, clusters, query_assignments, device)
    _check_allow(allow, n, q_dev, device)
    with KnnIndex(samples, centroids, assignments, metric=metric, device=device, verbosity=verbosity) as ix:
        if allow is not None:
            return ix.query_radius_allow(queries, radius, allow, query_assignments=query_assignments,
                                         return_distances=return_distances, sort=sort, count_only=count_only)
        return ix.query_radius(queries, radius, query_assignments=query_assignments,
                               return_distances=return_distances, sort=sort, count_only=count_only)
