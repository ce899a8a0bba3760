"""The capped search of the k-NN index (KnnIndex.query(max_distance=r)) in executable form: a plain
Python restatement of the oracle's knn_search_row (oracle/kmcuda_oracle.c) in which every read of the kth distance
reads min(kth, cap) -- the push test and the cluster test -- and nothing else changes.

It is built on what the oracle library exports only: kmo_knn_inverse, kmo_knn_radiuses, kmo_knn_cluster_distances and
kmo_distance (under kmo_set_fp16_mode(2) for the reference's half2 arithmetic).  The heap push is restated compare for
compare; `lim` is formed as two float32 subtractions.  At cap = FLT_MAX it is oracle.knn_query bit for bit
(tests/test_knn_capped_cpu.py holds it to that).

A probed list (4.12) is the list on the assignments with the rows outside the query's effective probe set set to
0xFFFFFFFF (the rule of tests/_probe_ref.py), a masked list (4.17) the list on the assignments with the denied rows set
to K.  Slow (a Python loop per candidate): keep N <= 2500 and Q <= 300."""
import ctypes

import numpy

import oracle
from _probe_ref import effective_set

NONE = 0xFFFFFFFF
FLT_MAX = float(numpy.finfo(numpy.float32).max)
_f32p = ctypes.POINTER(ctypes.c_float)
_u32p = ctypes.POINTER(ctypes.c_uint32)


def _push(k, dist, index, hd, hi):
    """push_sample (knn.cu:133-175) on the heap as two lists: distances hd, indices hi."""
    pos = 0
    while True:
        left = right = 0.0
        if 2 * pos + 1 < k:
            left = hd[2 * pos + 1]
            left_le = dist >= left
        else:
            left_le = True
        if 2 * pos + 2 < k:
            right = hd[2 * pos + 2]
            right_le = dist >= right
        else:
            right_le = True
        if left_le and right_le:
            hd[pos], hi[pos] = dist, index
            return
        if not left_le and not right_le:
            child = 2 * pos + 2 if left <= right else 2 * pos + 1
        elif left_le:
            child = 2 * pos + 2
        else:
            child = 2 * pos + 1
        hd[pos], hi[pos] = hd[child], hi[child]
        pos = child


class _Mode:
    """kmo_set_fp16_mode(2) around a half2 restatement (0 otherwise, as oracle.knn_query sets it)."""

    def __init__(self, half2):
        self.mode = 2 if half2 else 0

    def __enter__(self):
        oracle.lib().kmo_set_fp16_mode(self.mode)

    def __exit__(self, *exc):
        oracle.lib().kmo_set_fp16_mode(0)


class Corpus:
    """The corpus side of a search as knn_corpus_init makes it (CSR, radii, centroid distances), and the candidate
    distances of the queries seen so far: they depend on the pair alone, so every cap, k, probe set and mask of a
    fixture shares them (`cache`, keyed by the query's bytes)."""

    def __init__(self, x, c, a, metric="L2", half2=False, cache=None):
        if half2:
            assert x.dtype == c.dtype == numpy.float16
        self.metric = oracle._metric(metric)
        self.half2 = half2
        self.x = numpy.ascontiguousarray(x, dtype=numpy.float32)
        self.c = numpy.ascontiguousarray(c, dtype=numpy.float32)
        self.a = numpy.ascontiguousarray(a, dtype=numpy.uint32)
        self.N, self.D = self.x.shape
        self.K = self.c.shape[0]
        self.cache = {} if cache is None else cache
        L = oracle.lib()
        inv = numpy.empty(self.N, numpy.uint32)
        offsets = numpy.empty(self.K + 2, numpy.uint32)
        R = numpy.empty(self.K, numpy.float32)
        C = numpy.empty((self.K, self.K), numpy.float32)
        with _Mode(half2):
            L.kmo_knn_inverse(self.N, self.K, self.a.ctypes.data_as(_u32p), inv.ctypes.data_as(_u32p),
                              offsets.ctypes.data_as(_u32p))
            L.kmo_knn_radiuses(self.metric, self.N, self.D, self.K, self.x.ctypes.data_as(_f32p),
                               self.c.ctypes.data_as(_f32p), inv.ctypes.data_as(_u32p), offsets.ctypes.data_as(_u32p),
                               R.ctypes.data_as(_f32p))
            L.kmo_knn_cluster_distances(self.metric, self.D, self.K, self.c.ctypes.data_as(_f32p),
                                        C.ctypes.data_as(_f32p))
        self.inv, self.offsets, self.R, self.C = inv, [int(v) for v in offsets], R, C

    def with_assignments(self, a):
        """The same rows and centroids under other assignments (a probe set, a mask); shares the distance cache."""
        return Corpus(self.x.astype(numpy.float16) if self.half2 else self.x,
                      self.c.astype(numpy.float16) if self.half2 else self.c, a, self.metric, self.half2, self.cache)

    def _distances(self, q32):
        """kmo_distance of one query to every corpus row and every centroid (lists of Python floats)."""
        key = q32.tobytes()
        if key not in self.cache:
            fn = oracle.lib().kmo_distance
            qp = q32.ctypes.data_as(_f32p)
            step = self.D * 4
            with _Mode(self.half2):
                rows = [fn(self.metric, qp, ctypes.cast(self.x.ctypes.data + j * step, _f32p), self.D)
                        for j in range(self.N)]
                cen = [fn(self.metric, qp, ctypes.cast(self.c.ctypes.data + j * step, _f32p), self.D)
                       for j in range(self.K)]
            self.cache[key] = (rows, cen)
        return self.cache[key]

    def search_row(self, k, q32, mycls, cap):
        """knn_search_row with min(kth, cap) for kth: (neighbors, distances, candidates of the visited clusters)."""
        f32 = numpy.float32
        rows, cen = self._distances(q32)
        inv, offsets, K = self.inv, self.offsets, self.K
        mydist = f32(cen[mycls])
        hd, hi = [FLT_MAX] * k, [0] * k
        mndist = min(FLT_MAX, cap)
        calced = 0
        order = [mycls] + [cls for cls in range(K) if cls != mycls]
        for step, cls in enumerate(order):
            if step > 0:
                cd = self.C[cls, mycls]
                if cd != cd:
                    continue
                with numpy.errstate(all="ignore"):
                    lim = f32(f32(cd - mydist) - self.R[cls])
                if lim > mndist:
                    continue
            calced += offsets[cls + 1] - offsets[cls]
            for pos in range(offsets[cls], offsets[cls + 1]):
                other = int(inv[pos])
                dist = rows[other]
                if dist <= mndist:
                    _push(k, dist, other, hd, hi)
                    mndist = min(hd[0], cap)
        nb, dist = [0] * k, [0.0] * k
        for i in range(k - 1, -1, -1):
            nb[i], dist[i] = hi[0], hd[0]
            _push(k, -1.0, NONE, hd, hi)
        return nb, dist, calced


def _check_cap(cap):
    cap = float(numpy.float32(min(float(cap), FLT_MAX)))
    assert cap >= 0
    return cap


def capped_reference(k, corpus, q, qa=None, cap=FLT_MAX):
    """(neighbors uint32 Q x k, distances float32 Q x k, pairs in visited clusters) of the capped search of the
    queries q (float32 values; float16 under half2) on a Corpus.  qa=None: oracle.lloyd_assign, in fp32 arithmetic
    whatever the corpus's mode (4.8 point 1).  A query with a non-finite feature or a cluster id >= K: 0xFFFFFFFF /
    NaN, as oracle.knn_query."""
    cap = _check_cap(cap)
    q32 = numpy.ascontiguousarray(q, dtype=numpy.float32)
    if qa is None:
        qa, _, _ = oracle.lloyd_assign(q32, corpus.c, metric=corpus.metric)
    qa = numpy.asarray(qa).astype(numpy.int64)
    Q = len(q32)
    nb = numpy.full((Q, k), NONE, numpy.uint32)
    dist = numpy.full((Q, k), numpy.nan, numpy.float32)
    pairs = 0
    finite = numpy.isfinite(q32).all(axis=1)
    for i in range(Q):
        if not finite[i] or qa[i] >= corpus.K or qa[i] < 0:
            continue
        nb[i], dist[i], n = corpus.search_row(k, q32[i], int(qa[i]), cap)
        pairs += n
    return nb, dist, pairs


def capped_probe_reference(k, corpus, q, probes, cap=FLT_MAX):
    """capped_reference of the probed search (4.12): probes Q x p, column 0 the own cluster, K a filler.  One Corpus
    per group of queries with the same effective set."""
    probes = numpy.asarray(probes).astype(numpy.int64)
    K, Q = corpus.K, len(q)
    nb = numpy.full((Q, k), NONE, numpy.uint32)
    dist = numpy.full((Q, k), numpy.nan, numpy.float32)
    pairs = 0
    groups = {}
    for i in range(Q):
        if probes[i, 0] < K:
            groups.setdefault(effective_set(probes[i], K), []).append(i)
    for members, rows in groups.items():
        rows = numpy.asarray(rows)
        sub = corpus.with_assignments(numpy.where(numpy.isin(corpus.a, members), corpus.a, NONE).astype(numpy.uint32))
        nb[rows], dist[rows], n = capped_reference(k, sub, numpy.ascontiguousarray(q[rows]), probes[rows, 0], cap)
        pairs += n
    return nb, dist, pairs


def masked(corpus, allow):
    """The Corpus a masked search is defined by (4.17): the denied rows' assignments set to K."""
    allow = numpy.asarray(allow).astype(bool)
    return corpus.with_assignments(numpy.where(allow, corpus.a, corpus.K).astype(numpy.uint32))


def truncated(nb, dist, cap):
    """An uncapped list with every entry beyond cap replaced by the filler (index 0 at FLT_MAX); NaN rows stay."""
    cap = _check_cap(cap)
    nb, dist = nb.copy(), dist.copy()
    beyond = dist > numpy.float32(cap)
    nb[beyond] = 0
    dist[beyond] = FLT_MAX
    return nb, dist


def bits(d):
    """float32 bit patterns, every NaN mapped to one pattern."""
    d = numpy.ascontiguousarray(d, dtype=numpy.float32)
    return numpy.where(numpy.isnan(d), numpy.uint32(0x7FC00000), d.view(numpy.uint32))
