"""Top-k search over product-quantiser codes by asymmetric distance computation (C ABI: kmamd_pq_search,
include/kmcuda_amd.h) -- the search the codes of the batched calls are made for.

    codebooks, _, _ = kmeans_batched(x, 256, init="random", layout="columns", problems=M)
    codes = kmeans_predict_batched(x, codebooks, layout="columns", dtype=numpy.uint8)
    indices, distances = pq_search(queries, codebooks, codes, 10)

queries is (Q, M * dsub) float32, codebooks (M, ksub, dsub) float32, codes (N, M) uint8.  For every query a table of
its squared sub-space distances to every codeword, T[m][c] = sum_j fl(fl(x_j - y_j)^2) in ascending j, +inf for
c >= ksub; a row's distance is sum_m T[m][codes[i][m]] in ascending m (fp32, no FMA, no root); the k first rows by
(distance, row index) come back, bit for bit numpy.argsort(d, kind="stable")[:k] of that arithmetic, a NaN distance
behind +inf.  1 <= M <= 64, 1 <= dsub <= 64, 1 <= ksub <= 256, 1 <= N < 2^32, 1 <= k <= min(N, 256); L2 and float32
only.  numpy in, numpy out (indices uint32); torch tensors on `device` in, torch tensors out (indices int32); the three
operands must be of the same kind.  Every argument is checked before the device is touched; what is out of range is
refused, never routed elsewhere.

bits=4 (kmamd_pq4_search): codes of at most 16 codewords per sub-space, two to a byte -- codes is
(N, ceil(M / 2)) uint8, pq_pack4's output: sub-space 2j in bits 0..3 of byte j, sub-space 2j + 1 in bits 4..7, the last
high nibble ignored when M is odd, a nibble >= ksub at +inf.  1 <= M <= 128, 1 <= ksub <= 16, the definition unchanged:
for M <= 64 the result is, byte for byte, that of the same codes one to a byte.

table_dtype="float16" (kmamd_pq_search_f16): every table entry is rounded once to IEEE binary16 (to
nearest even, subnormals kept, beyond 65504 +inf) and a row's distance is sum_m float(T16[m][code]) in fp32 --
T.astype(numpy.float16).astype(numpy.float32) and the same ascending sum.  Half the LDS per query and per lookup; a
slightly different distance with its own bits.  Byte codes only: not with bits=4.
"""
import numpy

from . import _lib
from .api import _get_metric, _raise_for
from .batched import _f32, _out
from .knn_index import _is_torch, _ptr

_LDS_PER_CU = 160 << 10          # pq_scan.hip: kPqLdsPerCu


def _candidate_cap(k):
    cap = 64
    while cap < 2 * k:
        cap <<= 1
    return cap


def _scan_lds_bytes(m, k, qt, entries=256, entry_bytes=4):
    return qt * (m * entries * entry_bytes + _candidate_cap(k) * 8 + 16) + 16


def _bits(bits):
    if isinstance(bits, bool) or bits not in (4, 8):
        raise ValueError("\"bits\" must be 8 or 4")
    return int(bits)


def _table_dtype(table_dtype, bits=8, precomputed=False):
    """True for "float16"; refuses what fp16 tables do not go with"""
    if not isinstance(table_dtype, str) or table_dtype not in ("float32", "float16"):
        raise ValueError("\"table_dtype\" must be \"float32\" or \"float16\"")
    if table_dtype == "float16" and bits == 4:
        raise ValueError("fp16 tables serve the byte codes: table_dtype=\"float16\" goes without bits=4")
    if table_dtype == "float16" and precomputed:
        raise ValueError("the precomputed-term variant has fp32 tables: table_dtype=\"float16\" goes without it")
    return table_dtype == "float16"


def query_tile(subspaces, k, bits=8, table_dtype="float32"):
    """The queries one scan block serves (kmamd_pq_query_tile): their tables share the block's LDS.  16, 8 or 4 where
    two blocks fit a CU's LDS, else 4 or 2 with one; 0: `subspaces` or `k` out of range.  bits=4
    (kmamd_pq4_query_tile, also the pair tile of the 4-bit IVF scan): tables of 16 entries, up to 128 sub-spaces, and
    always two blocks.  table_dtype="float16" (kmamd_pq_f16_query_tile, also the pair tile of that IVF scan): entries
    of two bytes, 16, 8 or 4 with two blocks, else 4 with one."""
    half = _table_dtype(table_dtype, _bits(bits))
    if bits == 4:
        if not 1 <= subspaces <= 128 or not 1 <= k <= 256:
            return 0
        return next(qt for qt in (16, 8, 4) if _scan_lds_bytes(subspaces, k, qt, 16) <= _LDS_PER_CU // 2)
    if not 1 <= subspaces <= 64 or not 1 <= k <= 256:
        return 0
    if half:
        return next((qt for qt in (16, 8, 4) if _scan_lds_bytes(subspaces, k, qt, 256, 2) <= _LDS_PER_CU // 2), 4)
    for qt in (16, 8, 4):
        if _scan_lds_bytes(subspaces, k, qt) <= _LDS_PER_CU // 2:
            return qt
    for qt in (4, 2):
        if _scan_lds_bytes(subspaces, k, qt) <= _LDS_PER_CU:
            return qt
    return 0


def _codes(x, device):
    """(contiguous (N, M) uint8 array-or-tensor, on_device)"""
    if _is_torch(x):
        import torch
        if x.dtype != torch.uint8:
            raise TypeError("\"codes\" must be a uint8 tensor")
        if x.dim() != 2:
            raise ValueError("\"codes\" must be a 2D tensor")
        if not x.is_cuda or x.device.index != device:
            raise ValueError("\"codes\" must be on device %d (or be a numpy array)" % device)
        return x.contiguous(), True
    if not isinstance(x, numpy.ndarray) or x.dtype != numpy.uint8:
        raise TypeError("\"codes\" must be a uint8 numpy array")
    if x.ndim != 2:
        raise ValueError("\"codes\" must be a 2D numpy array")
    return numpy.ascontiguousarray(x), False


def pq_pack4(codes):
    """(N, M) uint8 codes, every one at most 15, packed two to a byte for bits=4: (N, ceil(M / 2)) uint8, column 2j in
    bits 0..3 of byte j and column 2j + 1 in bits 4..7 (0 behind an odd M).  numpy in, numpy out; torch in, torch out."""
    torch_in = _is_torch(codes)
    if torch_in:
        import torch
        if codes.dtype != torch.uint8:
            raise TypeError("\"codes\" must be a uint8 tensor")
    elif not isinstance(codes, numpy.ndarray) or codes.dtype != numpy.uint8:
        raise TypeError("\"codes\" must be a uint8 numpy array")
    if codes.ndim != 2:
        raise ValueError("\"codes\" must be 2D, (N, M)")
    if codes.shape[0] and codes.shape[1] and int(codes.max()) > 15:
        raise ValueError("a 4-bit code is at most 15")
    n, m = (int(v) for v in codes.shape)
    out = codes.new_zeros((n, (m + 1) // 2)) if torch_in else numpy.zeros((n, (m + 1) // 2), numpy.uint8)
    out[:, :m // 2] = codes[:, 1::2] << 4
    out |= codes[:, 0::2]
    return out


def pq_search(queries, codebooks, codes, k, *, metric="L2", device=0, verbosity=0, bits=8, table_dtype="float32"):
    """(indices, distances), each (Q, k): the k rows of `codes` nearest to every query by ADC (module docstring)."""
    bits = _bits(bits)
    half = _table_dtype(table_dtype, bits)
    max_m, max_ksub = (128, 16) if bits == 4 else (64, 256)
    if _get_metric(metric) != 0:
        raise ValueError("pq_search supports the L2 metric only")
    if isinstance(device, bool) or not isinstance(device, (int, numpy.integer)) or device < 0:
        raise ValueError("\"device\" must be a device id >= 0")
    if isinstance(k, bool) or not isinstance(k, (int, numpy.integer)):
        raise TypeError("\"k\" must be an integer")
    q, q_dev = _f32(queries, "queries", 2, int(device))
    b, b_dev = _f32(codebooks, "codebooks", 3, int(device))
    c, c_dev = _codes(codes, int(device))
    if not q_dev == b_dev == c_dev:
        raise TypeError("\"queries\", \"codebooks\" and \"codes\" must be of the same kind")
    m, ksub, dsub = (int(v) for v in b.shape)
    n = int(c.shape[0])
    if not 1 <= m <= max_m:
        raise ValueError("the number of sub-spaces must be in [1, %d]" % max_m)
    if not 1 <= dsub <= 64:
        raise ValueError("the number of features per sub-space must be in [1, 64]")
    if not 1 <= ksub <= max_ksub:
        raise ValueError("the number of codewords per sub-space must be in [1, %d]" % max_ksub)
    if bits == 4 and int(c.shape[1]) != (m + 1) // 2:
        raise ValueError("\"codes\" must have one column per two sub-spaces: (N, %d)" % ((m + 1) // 2))
    if bits == 8 and int(c.shape[1]) != m:
        raise ValueError("\"codes\" must have one column per sub-space: (N, %d)" % m)
    if int(q.shape[1]) != m * dsub:
        raise ValueError("\"queries\" must have %d columns" % (m * dsub))
    if not 1 <= n <= 0xFFFFFFFF:
        raise ValueError("the number of code rows must be in [1, 2^32)")
    if not 1 <= k <= min(n, 256):
        raise ValueError("\"k\" must be in [1, min(N, 256)]")
    nq = int(q.shape[0])
    if nq > 0xFFFFFFFF:
        raise ValueError("too many queries")
    idx = _out((nq, int(k)), numpy.uint32, q_dev, device)
    dist = _out((nq, int(k)), numpy.float32, q_dev, device)
    if nq == 0:
        return idx, dist
    name = "kmamd_pq4_search" if bits == 4 else "kmamd_pq_search_f16" if half else "kmamd_pq_search"
    rc = getattr(_lib.lib(), name)(nq, n, m * dsub, m, dsub, ksub, int(k), 0, 0, int(device),
                                   int(device) if q_dev else -1, int(verbosity), _ptr(q), _ptr(b), _ptr(c),
                                   _ptr(idx), _ptr(dist))
    _raise_for(rc, name)
    return idx, dist
