"""kmeans_predict_top on rows wider than 256 features: the streamed score kernel (assign_top_wide.hip)
in front of the shared select stage, bit for bit against the CPU oracle as tests/test_gpu_predict_top.py defines it.

The kernel's edges: 128-row blocks, 128-centroid panels of 32-centroid tiles, 32-feature chunks, 16-byte row loads where
D % 4 == 0 and the row pointer allows them.  NaN rows, non-finite centroids, ties and the clamp at D = 320 are
test_gpu_predict_top.py's test_edges / test_sweep_over_features / test_column_0_is_kmeans_predict.
"""
import numpy
import pytest

from test_gpu_predict_top import _check, _data, _dev, _ms, _same, _stats, _top

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


# the contenders of these inputs by the kernel's own bound in fp64: 4112 of 65 536 pairs at (64, 320), 4183 of 307 200
# at (300, 1000), at most 6 per row: the cap total // 2 is a condition, not a measurement
@pytest.mark.parametrize("k,d", [(64, 320), (300, 1000)])
def test_the_filter_filters_wide_rows(k, d, monkeypatch):
    rs = numpy.random.RandomState(5)
    n, m = 1024, 4
    c = (10.0 * rs.randn(k, d)).astype(numpy.float32)
    x = (c[rs.randint(0, k, n)] + 0.5 * rs.randn(n, d)).astype(numpy.float32)
    default = _top(x, c, m, "L2")
    exact, total = _stats()
    print("filtered: %d exact keys of %d pairs (%.4f)" % (exact, total, exact / total))
    assert total == n * k
    assert n * m <= exact <= total // 2
    monkeypatch.setenv("KMCUDA_AMD_ASSIGN_TOP", "exact")
    assert _same(_top(x, c, m, "L2"), default)
    exact, total = _stats()
    assert exact == total == n * k


# D: 257 one feature into a padded chunk and rows that are not 16-byte aligned (fp32 only: the interface refuses an odd
# feature count in fp16 mode), 288 whole chunks, 1000 16-byte rows short of a chunk, 1536 beyond every other filter;
# (N, K): one row; one under a 128-row block with a partial 32-centroid tile; one over a block with a second, partial
# panel; several blocks and panels, the last panel of two tiles
_SHAPES = [(d, 129, 130) for d in (257, 288, 1536)]
_SHAPES += [(1000, n, k) for n, k in ((1, 2), (127, 33), (129, 130), (300, 300))]
_CASES = [s + (t,) for s in _SHAPES for t in (numpy.float32, numpy.float16) if not (s[0] % 2 and t is numpy.float16)]


@pytest.mark.parametrize("metric", ["L2", "angular"])
@pytest.mark.parametrize("d,n,k,dtype", _CASES, ids=lambda v: v.__name__ if isinstance(v, type) else str(v))
def test_shapes(d, n, k, dtype, metric):
    x, c = _data(n, d, k, metric, dtype)
    name = numpy.dtype(dtype).name
    for m in _ms(k):
        _check(_top(x, c, m, metric), x, c, m, metric, ("wide", d, n, k, metric, name), "%dx%d K=%d" % (n, d, k))


def test_several_score_matrices(monkeypatch):
    x, c = _data(1000, 320, 16, "L2")
    whole = _check(_top(x, c, 5, "L2"), x, c, 5, "L2", what="1000x320 K=16")
    monkeypatch.setenv("KMCUDA_AMD_ASSIGN_TOP_ROWS", "300")   # 384-row score matrices: three, the last short
    assert _same(_top(x, c, 5, "L2"), whole)


def test_misaligned_device_view():
    x, c = _data(130, 257, 16, "L2")
    xs = torch.from_numpy(x).to(_dev())[1:]
    assert xs.data_ptr() % 16 != 0 and xs.is_contiguous()
    idx, dist = _top(xs, torch.from_numpy(c).to(_dev()), 3, "L2")
    _check((idx.cpu().numpy().view(numpy.uint32), dist.cpu().numpy()), x[1:], c, 3, "L2", what="x[1:] D=257")


def test_probed_query_on_a_wide_index(monkeypatch):
    from _probe_ref import check_probe
    from test_gpu_knn_probe import corpus, fresh
    x, c, a = corpus(1200, 320, 12, 77)
    check_probe(10, x, c, a, fresh(c, 90, 78), nprobe=3, expect="f16", monkeypatch=monkeypatch)
