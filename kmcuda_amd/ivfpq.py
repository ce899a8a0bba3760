"""IVF-PQ: product-quantiser codes of residuals in cluster lists, probed by asymmetric distance computation (C ABI:
kmamd_ivfpq_search, kmamd_ivfpq_residuals, include/kmcuda_amd.h; the precomputed-term variant --
ivfpq_terms, ivfpq_search(terms=), IvfPqIndex(precomputed=True) -- 4.24; non-residual lists, residual=False, 4.27).

    centroids, _ = kmeans_cuda(rows, 1024)
    codebooks = ivfpq_train(rows, centroids, subspaces=32)
    index = IvfPqIndex(rows, centroids, codebooks)
    indices, distances = index.search(queries, 10, nprobe=16)

A row is stored as the uint8 codes of its residual, row minus its coarse centroid, in the list of that centroid; a query
scans the lists of the clusters it probes only.  For a query x and a probed cluster p: r = fl(x - centroids[p]),
T[m][c] = sum_j fl(fl(r_j - y_j)^2) over the m-th sub-space in ascending j (+inf for c >= ksub), a list position's
distance sum_m T[m][codes[pos][m]] in ascending m (fp32, no FMA, no root); the k first of all probed positions by
(distance, id) come back, a NaN distance behind +inf.  Slots no probed row fills hold index -1 (0xFFFFFFFF in numpy's
uint32) and distance NaN.  Limits as pq_search, 1 <= nprobe <= min(K, 64), at most 2^32 - 2 list positions; L2 and
float32 only.  numpy in, numpy out (integers uint32); torch tensors on `device` in, torch tensors out (int32); all
operands must be of the same kind.  Every argument is checked before the device is touched.

bits=4 (kmamd_ivfpq4_search): at most 16 codewords per sub-space and the codes two to a byte, (L,
ceil(M / 2)) as pq_pack4 lays them out, up to 128 sub-spaces; the definition and, for M <= 64, every output byte are
those of the same codes one to a byte.  ivfpq_train(..., ksub=16) trains for it; IvfPqIndex(..., bits=4) packs.  Not with
the precomputed-term variant.

table_dtype="float16" (kmamd_ivfpq_search_f16): every entry of a pair's table is rounded once to IEEE
binary16 and a position's distance is sum_m float(T16[m][code]) in fp32, as pq_search(table_dtype="float16"): half the
LDS per pair and per lookup, a distance of its own bits.  Byte codes and residual tables only: not with bits=4, `terms`
or precomputed=True.  search(refine=) re-ranks its shortlist exactly, which is what the option is meant for.

residual=False (kmamd_ivfpq_search_nonresidual, _f16): the lists hold the codes of the rows themselves
(FAISS's by_residual = false) and the codebooks are trained on rows.  The table is then pq_search's, T[m][c] =
sum_j fl(fl(x_j - y_j)^2) of the query's own sub-vectors, built once per query and copied by the scan blocks; the result
is pq_search's arithmetic -- with table_dtype="float16" that of pq_search(table_dtype="float16") -- over the probed
lists.  `centroids` only gives K.  Coarser codes than residuals': search(refine=) is there to buy accuracy back.  Byte
codes only: not with bits=4, `terms` or precomputed=True.

knn_rerank (kmamd_knn_rerank) re-ranks such a shortlist against the raw rows by the exact L2 distance;
IvfPqIndex(..., keep_rows=True).search(..., refine=f) does both: a shortlist of k * f, then the exact k.
"""
import numpy

from . import _lib
from .api import _get_metric, _raise_for
from .batched import _f32, _out, kmeans_batched, kmeans_predict_batched
from .knn_index import _is_torch, _labels, _ptr
from .pq import _LDS_PER_CU, _bits, _codes, _scan_lds_bytes, _table_dtype, pq_pack4, query_tile as _pq_query_tile
from .predict import kmeans_predict, kmeans_predict_top

_BLOCKS = 512                    # kernels.hpp: kIvfPqBlocks
_CHUNK_BYTES = 256 << 20         # the fp32 residuals of one row chunk while an index is built


def _residual(residual, bits=8, precomputed=False):
    """False for non-residual lists; refuses what they do not go with"""
    if not isinstance(residual, (bool, numpy.bool_)):
        raise ValueError("\"residual\" must be a bool")
    if not residual and precomputed:
        raise ValueError("the precomputed terms cheapen residual tables: residual=False goes without them")
    if not residual and bits == 4:
        raise ValueError("non-residual lists hold byte codes: residual=False goes without bits=4")
    return bool(residual)


def query_tile(subspaces, k, bits=8, table_dtype="float32", residual=True):
    """The (query, probe) pairs one scan block serves (kmamd_ivfpq_query_tile): pq.query_tile's rule with the staged
    residual sub-vectors, 256 bytes per pair, added to the block's LDS; 0: `subspaces` or `k` out of range.  bits=4
    (kmamd_ivfpq4_query_tile): pq.query_tile's 4-bit rule as it is -- that block stages where its candidates go.
    table_dtype="float16" (kmamd_ivfpq_f16_query_tile): pq.query_tile's fp16 rule as it is, for the same reason.
    residual=False: pq.query_tile's rule as it is for either table type -- that block stages nothing."""
    half = _table_dtype(table_dtype, _bits(bits))
    if not _residual(residual, bits):
        return _pq_query_tile(subspaces, k, 8, table_dtype)
    if half:
        return _pq_query_tile(subspaces, k, 8, "float16")
    if bits == 4:
        return _pq_query_tile(subspaces, k, 4)
    if not 1 <= subspaces <= 64 or not 1 <= k <= 256:
        return 0
    for budget, tiles in ((_LDS_PER_CU // 2, (16, 8, 4)), (_LDS_PER_CU, (4, 2))):
        for qt in tiles:
            if _scan_lds_bytes(subspaces, k, qt) + qt * 256 <= budget:
                return qt
    return 0


def row_split(pairs, tile, list_rows):
    """The splits every probed list is cut into when `pairs` (query, probe) pairs are launched over `list_rows` list
    positions (kmamd_ivfpq_row_split): 1 once ceil(pairs / tile) reaches 512 blocks, else ceil(512 / that), at most
    ceil(list_rows / 256); 0: an argument is 0."""
    if pairs <= 0 or tile <= 0 or list_rows <= 0:
        return 0
    tiles = -(-pairs // tile)
    return 1 if tiles >= _BLOCKS else min(-(-_BLOCKS // tiles), -(-list_rows // 256))


def _device(device):
    if isinstance(device, bool) or not isinstance(device, (int, numpy.integer)) or device < 0:
        raise ValueError("\"device\" must be a device id >= 0")
    return int(device)


def _u32(x, name, shape, device):
    """(contiguous uint32 array / int32 tensor of that shape, on_device)"""
    if _is_torch(x):
        import torch
        if x.dtype.is_floating_point or x.dtype == torch.bool:
            raise TypeError("\"%s\" must be an integer tensor" % name)
        if tuple(x.shape) != shape:
            raise ValueError("\"%s\" must have the shape %r" % (name, shape))
        if not x.is_cuda or x.device.index != device:
            raise ValueError("\"%s\" must be on device %d (or be a numpy array)" % (name, device))
        return x.to(torch.int32).contiguous(), True
    if not isinstance(x, numpy.ndarray) or x.dtype.kind not in "iu":
        raise TypeError("\"%s\" must be an integer numpy array" % name)
    if x.shape != shape:
        raise ValueError("\"%s\" must have the shape %r" % (name, shape))
    return numpy.ascontiguousarray(x, dtype=numpy.uint32), False


def _residuals(rows, centroids, assignments, on_dev, device, verbosity=0):
    """fl(rows - centroids[assignments]), NaN rows where the assignment is len(centroids)."""
    out = _out(tuple(rows.shape), numpy.float32, on_dev, device)
    rc = _lib.lib().kmamd_ivfpq_residuals(int(rows.shape[0]), int(rows.shape[1]), int(centroids.shape[0]), device,
                                          device if on_dev else -1, int(verbosity), _ptr(rows), _ptr(centroids),
                                          _ptr(assignments), _ptr(out))
    _raise_for(rc, "kmamd_ivfpq_residuals")
    return out


def _corpus(rows, centroids, assignments, device):
    """(rows, centroids, assignments, on_device) checked; assignments from kmeans_predict when not given."""
    x, on_dev = _f32(rows, "rows", 2, device)
    c, c_dev = _f32(centroids, "centroids", 2, device)
    if c_dev != on_dev:
        raise TypeError("\"centroids\" must be of the same kind as \"rows\"")
    if int(c.shape[0]) < 1 or int(c.shape[1]) != int(x.shape[1]):
        raise ValueError("\"centroids\" must be (K >= 1, %d)" % int(x.shape[1]))
    if not 1 <= int(x.shape[0]) <= 0xFFFFFFFE:
        raise ValueError("the number of rows must be in [1, 2^32 - 2]")
    if assignments is not None:
        a, a_dev = _labels(assignments, int(x.shape[0]), "assignments", device=device)
        if a_dev != on_dev:
            raise TypeError("\"assignments\" must be of the same kind as \"rows\"")
    return x, c, assignments if assignments is None else a, on_dev


def _check_books(codebooks, width, on_dev, device, bits=8):
    b, b_dev = _f32(codebooks, "codebooks", 3, device)
    if b_dev != on_dev:
        raise TypeError("\"codebooks\" must be of the same kind as the other operands")
    m, ksub, dsub = (int(v) for v in b.shape)
    max_m, max_ksub = (128, 16) if bits == 4 else (64, 256)
    if not 1 <= m <= max_m:
        raise ValueError("the number of sub-spaces must be in [1, %d]" % max_m)
    if not 1 <= dsub <= 64:
        raise ValueError("the number of features per sub-space must be in [1, 64]")
    if not 1 <= ksub <= max_ksub:
        raise ValueError("the number of codewords per sub-space must be in [1, %d]" % max_ksub)
    if m * dsub != width:
        raise ValueError("\"codebooks\" must cover the %d features: subspaces * sub_features" % width)
    return b


def ivfpq_train(rows, centroids, subspaces, ksub=256, assignments=None, *, seed=0, max_iter=25, tolerance=0.0,
                metric="L2", device=0, verbosity=0, residual=True):
    """codebooks (subspaces, ksub, D / subspaces): one kmeans_batched call (layout="columns", init="random") over the
    residuals of `rows` against `centroids` -- with residual=False over the rows themselves; rows without a cluster
    (assignment K) are left out."""
    if _get_metric(metric) != 0:
        raise ValueError("IVF-PQ supports the L2 metric only")
    residual = _residual(residual)
    device = _device(device)
    if isinstance(subspaces, bool) or not isinstance(subspaces, (int, numpy.integer)) or not 1 <= subspaces <= 64:
        raise ValueError("\"subspaces\" must be an integer in [1, 64]")
    if isinstance(ksub, bool) or not isinstance(ksub, (int, numpy.integer)) or not 1 <= ksub <= 256:
        raise ValueError("\"ksub\" must be an integer in [1, 256]")
    x, c, a, on_dev = _corpus(rows, centroids, assignments, device)
    d = int(x.shape[1])
    if d % subspaces or d // subspaces > 64:
        raise ValueError("the features must split into `subspaces` blocks of at most 64")
    if a is None:
        a = kmeans_predict(x, c, device=device, verbosity=verbosity)
    res = _residuals(x, c, a, on_dev, device, verbosity) if residual else x
    res = res[(a.long() if on_dev else a) < int(c.shape[0])]
    books, _, _ = kmeans_batched(res, int(ksub), init="random", max_iter=max_iter, tolerance=tolerance, seed=seed,
                                 layout="columns", problems=int(subspaces), device=device, verbosity=verbosity)
    return books


def ivfpq_terms(centroids, codebooks, *, metric="L2", device=0, verbosity=0):
    """terms (K, M, ksub) float32 of an index, for ivfpq_search(terms=) (kmamd_ivfpq_terms):
    terms[p][m][c] = fl(sum_j fl(y_j y_j) + 2 sum_j fl(g_j y_j)), y = codebooks[m][c], g the m-th sub-vector of
    centroids[p], both sums in ascending j.  numpy or torch like its operands."""
    if _get_metric(metric) != 0:
        raise ValueError("IVF-PQ supports the L2 metric only")
    device = _device(device)
    c, on_dev = _f32(centroids, "centroids", 2, device)
    if int(c.shape[0]) < 1:
        raise ValueError("\"centroids\" must be (K >= 1, D)")
    b = _check_books(codebooks, int(c.shape[1]), on_dev, device)
    m, ksub, dsub = (int(v) for v in b.shape)
    terms = _out((int(c.shape[0]), m, ksub), numpy.float32, on_dev, device)
    rc = _lib.lib().kmamd_ivfpq_terms(int(c.shape[0]), m * dsub, m, dsub, ksub, device, device if on_dev else -1,
                                      int(verbosity), _ptr(c), _ptr(b), _ptr(terms))
    _raise_for(rc, "kmamd_ivfpq_terms")
    return terms


def ivfpq_search(queries, centroids, codebooks, codes, ids, offsets, probes, k, *, metric="L2", device=0,
                 verbosity=0, terms=None, bits=8, table_dtype="float32", residual=True):
    """(indices, distances), each (Q, k), over a caller's own lists (module docstring): codes (L, M) uint8 in list
    order -- (L, ceil(M / 2)) packed with bits=4, which `terms` does not go with --,
    ids (L,), offsets (K + 1,), probes (Q, nprobe) -- entries >= K and repeated entries are ignored.  The
    contents of codes, ids, offsets and probes are not checked and need not be: nothing in them leads out of range.
    terms: ivfpq_terms' (K, M, ksub) float32 array of this index, of the operands' kind: the precomputed-term variant
    (kmamd_ivfpq_search_precomputed) -- T[m][c] = fl(terms[p][m][c] - 2 sum_j fl(x_j y_j)),
    d = fl(sum_j fl(fl(x_j - g_j)^2) + sum_m T[m][code]), negative or -0 as +0: the same distance in other bits.
    table_dtype="float16": the tables of halves of the module docstring (kmamd_ivfpq_search_f16); not with bits=4 or
    `terms`.
    residual=False: `codes` are those of the rows themselves and `codebooks` their quantiser (module docstring;
    kmamd_ivfpq_search_nonresidual, with table_dtype="float16" kmamd_ivfpq_search_nonresidual_f16); not with bits=4 or
    `terms`."""
    if _get_metric(metric) != 0:
        raise ValueError("IVF-PQ supports the L2 metric only")
    device = _device(device)
    if _bits(bits) == 4 and terms is not None:
        raise ValueError("the precomputed-term variant has no 4-bit codes: bits=4 goes without \"terms\"")
    half = _table_dtype(table_dtype, bits, terms is not None)
    residual = _residual(residual, bits, terms is not None)
    if isinstance(k, bool) or not isinstance(k, (int, numpy.integer)):
        raise TypeError("\"k\" must be an integer")
    q, on_dev = _f32(queries, "queries", 2, device)
    c, c_dev = _f32(centroids, "centroids", 2, device)
    if c_dev != on_dev:
        raise TypeError("\"centroids\" must be of the same kind as \"queries\"")
    nq, d = (int(v) for v in q.shape)
    clusters = int(c.shape[0])
    if clusters < 1 or int(c.shape[1]) != d:
        raise ValueError("\"centroids\" must be (K >= 1, %d)" % d)
    b = _check_books(codebooks, d, on_dev, device, bits)
    m, ksub, dsub = (int(v) for v in b.shape)
    cd, cd_dev = _codes(codes, device)
    rows = int(cd.shape[0])
    if bits == 4 and int(cd.shape[1]) != (m + 1) // 2:
        raise ValueError("\"codes\" must have one column per two sub-spaces: (L, %d)" % ((m + 1) // 2))
    if bits == 8 and int(cd.shape[1]) != m:
        raise ValueError("\"codes\" must have one column per sub-space: (L, %d)" % m)
    if not 1 <= rows <= 0xFFFFFFFE:
        raise ValueError("the number of list positions must be in [1, 2^32 - 2]")
    i, i_dev = _u32(ids, "ids", (rows,), device)
    o, o_dev = _u32(offsets, "offsets", (clusters + 1,), device)
    if getattr(probes, "ndim", 0) != 2:
        raise ValueError("\"probes\" must be a 2D array, (Q, nprobe)")
    nprobe = int(probes.shape[1])
    if not 1 <= nprobe <= min(clusters, 64):
        raise ValueError("\"nprobe\" must be in [1, min(K, 64)]")
    p, p_dev = _u32(probes, "probes", (nq, nprobe), device)
    if not on_dev == cd_dev == i_dev == o_dev == p_dev:
        raise TypeError("all operands must be of the same kind")
    if not 1 <= k <= 256:
        raise ValueError("\"k\" must be in [1, 256]")
    if nq > 0xFFFFFFFF:
        raise ValueError("too many queries")
    if terms is not None:
        a, a_dev = _f32(terms, "terms", 3, device)
        if a_dev != on_dev:
            raise TypeError("\"terms\" must be of the same kind as the other operands")
        if tuple(int(v) for v in a.shape) != (clusters, m, ksub):
            raise ValueError("\"terms\" must have the shape %r" % ((clusters, m, ksub),))
    idx = _out((nq, int(k)), numpy.uint32, on_dev, device)
    dist = _out((nq, int(k)), numpy.float32, on_dev, device)
    if nq == 0:
        return idx, dist
    head = (nq, rows, d, clusters, m, dsub, ksub, int(k), nprobe, 0, 0, device, device if on_dev else -1,
            int(verbosity), _ptr(q), _ptr(c), _ptr(b), _ptr(cd), _ptr(i), _ptr(o), _ptr(p))
    if not residual:
        name = "kmamd_ivfpq_search_nonresidual_f16" if half else "kmamd_ivfpq_search_nonresidual"
        rc = getattr(_lib.lib(), name)(*head, _ptr(idx), _ptr(dist))
    elif bits == 4:
        rc = _lib.lib().kmamd_ivfpq4_search(*head, _ptr(idx), _ptr(dist))
    elif half:
        rc = _lib.lib().kmamd_ivfpq_search_f16(*head, _ptr(idx), _ptr(dist))
    elif terms is None:
        rc = _lib.lib().kmamd_ivfpq_search(*head, _ptr(idx), _ptr(dist))
    else:
        rc = _lib.lib().kmamd_ivfpq_search_precomputed(*head, _ptr(a), _ptr(idx), _ptr(dist))
    _raise_for(rc, "kmamd_ivfpq_search")
    return idx, dist


def knn_rerank(queries, rows, candidates, k, *, metric="L2", device=0, verbosity=0):
    """(indices, distances), each (Q, k): the k nearest of every query's own candidates by the exact L2 distance
    (kmamd_knn_rerank) -- the step behind an approximate shortlist.  `candidates` is (Q, R) row ids of
    `rows` (N, D), k <= R <= 1024; entries >= N, ivfpq_search's padding among them, are ignored and an id listed twice
    appears twice.  The distances are kmeans_predict's and KnnIndex.query's bits (NaN behind +inf, -0 as +0); ties go
    to the smaller id; slots no candidate fills hold index -1 (0xFFFFFFFF in numpy's uint32) and distance NaN.
    Operand kinds as ivfpq_search.  Host operands are staged whole, `rows` included: keep them on the device."""
    if _get_metric(metric) != 0:
        raise ValueError("knn_rerank supports the L2 metric only")
    device = _device(device)
    if isinstance(k, bool) or not isinstance(k, (int, numpy.integer)):
        raise TypeError("\"k\" must be an integer")
    q, on_dev = _f32(queries, "queries", 2, device)
    x, x_dev = _f32(rows, "rows", 2, device)
    nq, d = (int(v) for v in q.shape)
    n = int(x.shape[0])
    if d < 1 or int(x.shape[1]) != d:
        raise ValueError("\"queries\" and \"rows\" must have the same number of features, at least 1")
    if not 1 <= n <= 0xFFFFFFFE:
        raise ValueError("the number of rows must be in [1, 2^32 - 2]")
    if getattr(candidates, "ndim", 0) != 2:
        raise ValueError("\"candidates\" must be a 2D array, (Q, R)")
    r = int(candidates.shape[1])
    if not 1 <= r <= 1024:
        raise ValueError("the number of candidates per query must be in [1, 1024]")
    c, c_dev = _u32(candidates, "candidates", (nq, r), device)
    if not on_dev == x_dev == c_dev:
        raise TypeError("all operands must be of the same kind")
    if not 1 <= k <= min(r, 256):
        raise ValueError("\"k\" must be in [1, min(R, 256)]")
    if nq > 0xFFFFFFFF:
        raise ValueError("too many queries")
    idx = _out((nq, int(k)), numpy.uint32, on_dev, device)
    dist = _out((nq, int(k)), numpy.float32, on_dev, device)
    if nq == 0:
        return idx, dist
    rc = _lib.lib().kmamd_knn_rerank(nq, n, d, r, int(k), 0, 0, device, device if on_dev else -1, int(verbosity),
                                     _ptr(q), _ptr(x), _ptr(c), _ptr(idx), _ptr(dist))
    _raise_for(rc, "kmamd_knn_rerank")
    return idx, dist


class IvfPqIndex:
    """`rows` encoded against `codebooks` (ivfpq_train's) and kept as cluster lists: .codes (L, M) uint8 in list order,
    .ids (L,) the row of every list position, .offsets (K + 1,), beside .centroids and .codebooks.  Lists come from a
    stable sort by assignment (a list's ids ascend); rows with assignment K are left out.  precomputed=True builds
    .terms (ivfpq_terms) once and search() runs the precomputed-term variant (ivfpq_search's `terms`).  bits=4
    (.bits): codebooks of at most 16 codewords, .codes packed two to a byte, (L, ceil(M / 2)); not with precomputed.
    table_dtype="float16" (.table_dtype): search() scans tables of halves (ivfpq_search's `table_dtype`); the index
    itself is the same; not with bits=4 or precomputed.  residual=False (.residual): .codes are those of the rows
    themselves against `codebooks` (ivfpq_train(residual=False)'s) and search() scans query-level tables
    (ivfpq_search's `residual`); not with bits=4 or precomputed."""

    def __init__(self, rows, centroids, codebooks, assignments=None, *, metric="L2", device=0, verbosity=0,
                 keep_rows=False, precomputed=False, bits=8, table_dtype="float32", residual=True):
        if _get_metric(metric) != 0:
            raise ValueError("IVF-PQ supports the L2 metric only")
        self.bits = _bits(bits)
        if self.bits == 4 and precomputed:
            raise ValueError("the precomputed-term variant has no 4-bit codes: bits=4 goes without precomputed=True")
        _table_dtype(table_dtype, self.bits, bool(precomputed))
        self.table_dtype = table_dtype
        self.residual = _residual(residual, self.bits, bool(precomputed))
        self.device, self.verbosity = _device(device), int(verbosity)
        x, c, a, on_dev = _corpus(rows, centroids, assignments, self.device)
        self.rows = x if keep_rows else None       # the checked array itself, no copy: search(refine=) reads it
        b = _check_books(codebooks, int(x.shape[1]), on_dev, self.device, self.bits)
        if a is None:
            a = kmeans_predict(x, c, device=self.device, verbosity=verbosity)
        n, clusters = int(x.shape[0]), int(c.shape[0])
        codes = _out((n, int(b.shape[0])), numpy.uint8, on_dev, self.device)
        step = max(1, _CHUNK_BYTES // (4 * int(x.shape[1])))
        for r0 in range(0, n, step):
            res = x[r0:r0 + step]
            if self.residual:
                res = _residuals(res, c, a[r0:r0 + step], on_dev, self.device, verbosity)
            codes[r0:r0 + step] = kmeans_predict_batched(res, b, layout="columns", dtype=numpy.uint8,
                                                         device=self.device, verbosity=verbosity)
        if on_dev:
            import torch
            labels = a.long() & 0xFFFFFFFF
            order = torch.sort(labels, stable=True).indices
            order = order[:int((labels < clusters).sum())]
            counts = torch.bincount(labels[order], minlength=clusters)
            offsets = torch.zeros(clusters + 1, dtype=torch.int64, device=a.device)
            offsets[1:] = torch.cumsum(counts, 0)
            self.ids, self.offsets = order.to(torch.int32), offsets.to(torch.int32)
        else:
            order = numpy.argsort(a, kind="stable")
            order = order[:int((a < clusters).sum())]
            offsets = numpy.zeros(clusters + 1, numpy.int64)
            offsets[1:] = numpy.cumsum(numpy.bincount(a[order], minlength=clusters))
            self.ids, self.offsets = order.astype(numpy.uint32), offsets.astype(numpy.uint32)
        if len(order) == 0:
            raise ValueError("no row has a cluster")
        self.centroids, self.codebooks, self.codes = c, b, codes[order]
        if self.bits == 4:     # a row at NaN has code ksub: with 16 codewords its low nibble, as a byte keeps 256's
            self.codes = pq_pack4(self.codes & 15)
        self.terms = ivfpq_terms(c, b, device=self.device, verbosity=verbosity) if precomputed else None

    def search(self, queries, k, nprobe=1, probes=None, refine=None):
        """(indices, distances) of the k nearest stored rows among the `nprobe` nearest clusters of every query
        (kmeans_predict_top's ranking), or among the clusters `probes` (Q, nprobe) lists.
        refine: an integer factor >= 1 with k * refine <= 256, on an index built with keep_rows=True: the search runs
        at k * refine and knn_rerank picks the k nearest of that shortlist against the kept rows.  The distances are
        then exact L2 distances (kmeans_predict's bits), not ADC sums of squares."""
        if refine is not None:
            if isinstance(refine, bool) or not isinstance(refine, (int, numpy.integer)) or refine < 1:
                raise ValueError("\"refine\" must be an integer >= 1")
            if not isinstance(k, (int, numpy.integer)) or isinstance(k, bool) or not 1 <= k * refine <= 256:
                raise ValueError("\"k\" must be an integer >= 1 with k * refine <= 256")
            if getattr(self, "rows", None) is None:
                raise ValueError("\"refine\" needs an index built with keep_rows=True")
            shortlist, _ = self.search(queries, int(k * refine), nprobe, probes)
            return knn_rerank(queries, self.rows, shortlist, int(k), device=self.device, verbosity=self.verbosity)
        if probes is None:
            q, _ = _f32(queries, "queries", 2, self.device)
            clusters = int(self.centroids.shape[0])
            if isinstance(nprobe, bool) or not isinstance(nprobe, (int, numpy.integer)):
                raise TypeError("\"nprobe\" must be an integer")
            if not 1 <= nprobe <= min(clusters, 64):
                raise ValueError("\"nprobe\" must be in [1, min(K, 64)]")
            if not isinstance(k, (int, numpy.integer)) or isinstance(k, bool) or not 1 <= k <= 256:
                raise ValueError("\"k\" must be an integer in [1, 256]")
            if int(q.shape[0]) == 0:
                probes = _out((0, int(nprobe)), numpy.uint32, _is_torch(q), self.device)
            else:
                probes = kmeans_predict_top(q, self.centroids, int(nprobe), device=self.device,
                                            return_distances=False, verbosity=self.verbosity)
        return ivfpq_search(queries, self.centroids, self.codebooks, self.codes, self.ids, self.offsets, probes, k,
                            device=self.device, verbosity=self.verbosity, terms=getattr(self, "terms", None),
                            bits=getattr(self, "bits", 8), table_dtype=getattr(self, "table_dtype", "float32"),
                            residual=getattr(self, "residual", True))
