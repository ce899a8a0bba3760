"""Mini-batch K-means on a model that stays on the GPU between calls (C ABI: kmamd_minibatch_*,
include/kmcuda_amd.h): update a trained model with new rows, train on a stream, or train on a corpus
that is larger than device memory.

    model = MiniBatchKMeans(seeds)                       # K x D centroids, cluster weights 0: the seeds are forgotten
    for rows in stream:
        model.partial_fit(rows)                          # one step of Sculley's update on all rows of the batch
    model.fit(corpus, steps=100, batch_size=65536)       # batches drawn from a corpus, with replacement
    centroids, weights = model.centroids, model.cluster_weights

    centroids, weights = kmeans_minibatch(corpus, 1024, batch_size=65536, steps=100)   # seeds by k-means||

One step assigns the batch as kmeans_predict does, adds up every cluster's members in fp64 in a fixed order, and moves
the centre: W' = W + sum(w), C' = (C W + sum(w x)) / W' (angular: scaled to unit length instead).  A centre without a
member in the batch stays where it is.  There is no early stop and no reassignment of starved centres.

The centroids are float32 whatever the rows are; float16 rows select fp16x2 (fp32 arithmetic on the half values).
numpy in, numpy out; a torch tensor on `device` in, tensors on that device out with no host round trip: `centroids`,
`cluster_weights` and the assignments partial_fit returns are of the kind the model's centroids were given in, and
rows of either kind are accepted by every call.
"""
import ctypes
import operator

import numpy

from . import _lib
from .api import _get_metric, _raise_for
from .knn_index import _is_torch, _ptr, _rows
from .predict import _fp16_strict


def _index(x, name, lo, hi):
    if isinstance(x, (bool, float)) or not hasattr(x, "__index__"):
        raise TypeError("\"%s\" must be an integer" % name)
    x = operator.index(x)
    if x < lo or x > hi:
        raise ValueError("\"%s\" must be in [%d, %d]" % (name, lo, hi))
    return x


def _vector(x, n, name, dtype, device, on_dev):
    """A 1-D array of n elements of `dtype`, of the kind (numpy / tensor on `device`) that on_dev says."""
    if _is_torch(x):
        import torch
        if not on_dev:
            raise TypeError("\"%s\" must be a numpy array, as the rows it goes with" % name)
        if not x.is_cuda or x.device.index != device:
            raise ValueError("\"%s\" must be on device %d" % (name, device))
        if x.dim() != 1 or x.shape[0] != n:
            raise ValueError("\"%s\" must be 1D with %d elements" % (name, n))
        want = torch.float32 if dtype == numpy.float32 else torch.float64
        if x.dtype != want:
            raise TypeError("\"%s\" must be a %s tensor" % (name, want))
        return x.contiguous()
    if on_dev:
        raise TypeError("\"%s\" must be a tensor on the device, as the rows it goes with" % name)
    if not isinstance(x, numpy.ndarray) or x.dtype != dtype:
        raise TypeError("\"%s\" must be a 1D %s numpy array" % (name, numpy.dtype(dtype).name))
    if x.ndim != 1 or x.shape[0] != n:
        raise ValueError("\"%s\" must be 1D with %d elements" % (name, n))
    return numpy.ascontiguousarray(x)


class MiniBatchKMeans:
    """The resident model: `centroids` (K x D, float32 or float16, K >= 2) and optional `cluster_weights` (K float64,
    finite and >= 0; None: zeros, so that the first batch that reaches a centre replaces it by the batch mean)."""

    def __init__(self, centroids, metric="L2", device=0, cluster_weights=None, verbosity=0):
        self.h = None
        metric_id = _get_metric(metric)
        if isinstance(device, bool) or not isinstance(device, (int, numpy.integer)):
            raise TypeError("\"device\" must be an integer: one device id, not kmeans_cuda's mask")
        device = int(device)
        if device < 0:
            raise ValueError("\"device\" must be a device id >= 0")
        c, _, clusters, d, on_dev = _rows(centroids, "centroids", device)
        if d == 0 or d > 0xFFFF:
            raise ValueError("the number of features must be in [1, 65535]")
        if clusters < 2 or clusters >= 0x7FFFFFFF:
            raise ValueError("\"centroids\" must have at least 2 rows")
        if on_dev:
            import torch
            c = c.to(torch.float32)
        else:
            c = c.astype(numpy.float32, copy=False)
        cw = None
        if cluster_weights is not None:
            cw = _vector(cluster_weights, clusters, "cluster_weights", numpy.float64, device, on_dev)
            finite = bool(((cw >= 0) & (cw < float("inf"))).all())
            if not finite:
                raise ValueError("\"cluster_weights\" must be finite and >= 0")
        self.metric, self.device, self.clusters, self.features = metric, device, clusters, d
        self._on_dev = on_dev
        self.lib = _lib.lib()
        h = ctypes.c_void_p()
        rc = self.lib.kmamd_minibatch_create(ctypes.byref(h), metric_id, d, clusters, device, device if on_dev else -1,
                                             int(verbosity), _ptr(c), _ptr(cw) if cw is not None else None)
        _raise_for(rc, "kmamd_minibatch_create")
        self.h = h

    # ---- the calls ----
    def _check_rows(self, rows, name, sample_weight):
        if not self.h:
            raise ValueError("the model is closed")
        r, fp16, n, d, on_dev = _rows(rows, name, self.device)
        if d != self.features:
            raise ValueError("\"%s\" must have the centroids' number of features (%d)" % (name, self.features))
        if fp16 and d % 2:
            raise ValueError("the number of features must be even in fp16 mode")
        if fp16 and _fp16_strict():
            raise ValueError("KMCUDA_AMD_FP16_STRICT=1: the reference's half2 arithmetic has no mini-batch form")
        w = None
        if sample_weight is not None:
            w = _vector(sample_weight, n, "sample_weight", numpy.float32, self.device, on_dev)
        return r, fp16, n, on_dev, w

    def partial_fit(self, rows, sample_weight=None, return_assignments=False):
        """One step on all of `rows` (n x D; at most kmeans_predict's chunk of rows).  sample_weight: n float32
        weights, finite and > 0, of the rows' kind -- a row of weight w counts as w copies.  Returns self, or the
        rows' assignments (uint32 numpy / int32 tensor; K: the row took no part) with return_assignments."""
        r, fp16, n, on_dev, w = self._check_rows(rows, "rows", sample_weight)
        if n > 0xFFFFFFFF:
            raise ValueError("too many rows")
        asg = None
        if return_assignments:
            if on_dev:
                import torch
                asg = torch.empty((n,), dtype=torch.int32, device=torch.device("cuda", self.device))
            else:
                asg = numpy.empty((n,), numpy.uint32)
        rc = self.lib.kmamd_minibatch_step(self.h, n, int(fp16), _ptr(r), _ptr(w) if w is not None else None,
                                           _ptr(asg) if asg is not None else None, self.device if on_dev else -1)
        if rc == 1 and w is not None:
            raise ValueError("kmamd_minibatch_step refused its arguments: \"sample_weight\" must be finite and > 0 "
                             "and a step holds at most kmeans_predict's chunk of rows")
        _raise_for(rc, "kmamd_minibatch_step")
        return asg if return_assignments else self

    def fit(self, samples, steps, batch_size, seed=0, sample_weight=None):
        """`steps` steps of `batch_size` rows each, drawn from `samples` with replacement by a stateless hash of (seed,
        the model's step counter, slot): fit(.., 10) twice is fit(.., 20).  sample_weight: one weight per corpus row,
        gathered with it.  Returns self."""
        steps = _index(steps, "steps", 0, 0xFFFFFFFF)
        batch_size = _index(batch_size, "batch_size", 1, 0xFFFFFFFF)
        if isinstance(seed, (bool, float)) or not hasattr(seed, "__index__"):
            raise TypeError("\"seed\" must be an integer")
        seed = operator.index(seed) & 0xFFFFFFFF
        s, fp16, n, on_dev, w = self._check_rows(samples, "samples", sample_weight)
        if n == 0:
            raise ValueError("\"samples\" must have at least one row")
        rc = self.lib.kmamd_minibatch_fit(self.h, n, int(fp16), _ptr(s), _ptr(w) if w is not None else None,
                                          batch_size, steps, seed, self.device if on_dev else -1)
        if rc == 1 and w is not None:
            raise ValueError("kmamd_minibatch_fit refused its arguments: \"sample_weight\" must be finite and > 0 "
                             "and a batch holds at most kmeans_predict's chunk of rows")
        _raise_for(rc, "kmamd_minibatch_fit")
        return self

    # ---- the state ----
    def _read(self, want_c, want_w):
        if not self.h:
            raise ValueError("the model is closed")
        c = w = None
        if self._on_dev:
            import torch
            dev = torch.device("cuda", self.device)
            if want_c:
                c = torch.empty((self.clusters, self.features), dtype=torch.float32, device=dev)
            if want_w:
                w = torch.empty((self.clusters,), dtype=torch.float64, device=dev)
        else:
            if want_c:
                c = numpy.empty((self.clusters, self.features), numpy.float32)
            if want_w:
                w = numpy.empty((self.clusters,), numpy.float64)
        t = ctypes.c_uint64(0)
        rc = self.lib.kmamd_minibatch_read(self.h, _ptr(c) if c is not None else None,
                                           _ptr(w) if w is not None else None, ctypes.byref(t),
                                           self.device if self._on_dev else -1)
        _raise_for(rc, "kmamd_minibatch_read")
        return c, w, int(t.value)

    @property
    def centroids(self):
        """A copy of the K x D float32 centroids."""
        return self._read(True, False)[0]

    @property
    def cluster_weights(self):
        """A copy of the K float64 cluster weights: the weight every centre has absorbed so far."""
        return self._read(False, True)[1]

    @property
    def steps_done(self):
        return self._read(False, False)[2]

    def close(self):
        if getattr(self, "h", None):
            self.lib.kmamd_minibatch_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kmeans_minibatch(samples, clusters, batch_size, steps, init="k-means||", seed=0, metric="L2", device=0,
                     sample_weight=None, verbosity=0):
    """(centroids, cluster_weights) after `steps` steps of `batch_size` rows drawn from `samples`, starting from
    `init` with cluster weights 0: "k-means||" -- kmeans_seed_parallel(samples, clusters, seed=seed) -- or an array of
    `clusters` centroids.  centroids are float32 (clusters x D), cluster_weights float64; numpy for numpy samples,
    tensors on `device` for a tensor on it.  Every argument is checked before the device is touched."""
    clusters = _index(clusters, "clusters", 2, 0x7FFFFFFE)
    steps = _index(steps, "steps", 0, 0xFFFFFFFF)
    batch_size = _index(batch_size, "batch_size", 1, 0xFFFFFFFF)
    _get_metric(metric)
    s, fp16, n, d, on_dev = _rows(samples, "samples", device if isinstance(device, int) else None)
    if n == 0:
        raise ValueError("\"samples\" must have at least one row")
    if isinstance(init, str):
        if init != "k-means||":
            raise ValueError("\"init\" must be \"k-means||\" or an array of centroids")
        from .seed import kmeans_seed_parallel
        start = kmeans_seed_parallel(s, clusters, metric=metric, seed=seed, device=device, verbosity=verbosity)
    else:
        start, _, k0, d0, c_dev = _rows(init, "init", device if isinstance(device, int) else None)
        if k0 != clusters or d0 != d:
            raise ValueError("\"init\" must hold \"clusters\" centroids with the samples' number of features")
        if c_dev != on_dev:
            raise TypeError("\"init\" must be of the same kind as \"samples\"")
    with MiniBatchKMeans(start, metric=metric, device=device, verbosity=verbosity) as model:
        model.fit(s, steps, batch_size, seed=seed, sample_weight=sample_weight)
        return model.centroids, model.cluster_weights
