"""The capped search of the k-NN index on the GPU (KnnIndex.query(max_distance=r)) against its
definition in executable form, tests/_capped_ref.py: every search kernel in its query, probe and mask form, the caps
where a list changes (0, percentiles of the k-th distances, a value equal to a returned distance, above every distance,
FLT_MAX and inf), k around the heap sizes and up to the corpus, the host path's chunking and fallbacks, a live index,
and the counters that show the cap reaching the cluster prune.

One helper checks every case.  L2 and the half2 arithmetic: indices and distance bit patterns equal the restatement's,
NaN rows and FLT_MAX fillers included.  Angular: the allowance of tests/_angular.py and nothing wider, every returned
distance within 2 float32 ulp of oracle.distance, at a cap no oracle distance lies within 4 ulp of (asserted), so that
an acos last-place difference cannot move a row across it.  return_counts equals the entries <= r of the restatement's
list.  `expect` names the search that must have run, read from what verbosity 1 prints."""
import re

import numpy
import pytest

import oracle
from _angular import assert_knn_only_acos_matters
from _capped_ref import (FLT_MAX, NONE, Corpus, bits, capped_probe_reference, capped_reference, masked)
from test_gpu_kmeans import StdoutListener
from test_gpu_knn_edges import blobs, unit_corpus
from test_gpu_knn_query_edges import EXACT, INDEX_HALF_RANGE, QUERY_HALF_RANGE, batch, half_case
from test_knn_capped_cpu import prune_fixture

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PATHS = {"f16": {}, "f32": {"KMCUDA_AMD_FILTER": "f32"}, "exact": {"KMCUDA_AMD_KNN_EXACT": 1}}
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def fixture(d, n=1500, nq=120, metric="L2"):
    """(x, c, a, q, Corpus, uncapped lists at k = 10) of a blob corpus (unit rows for the angular metric), built once per
    module; the Corpus keeps every candidate distance it has computed."""
    def make():
        if metric == "L2":
            x, c, a = blobs(n, d, 24, 1.0, seed=100 + d, spread=0.05)
            q = batch(x, c, 0.05, seed=d, fresh=nq)
        else:
            x = unit_corpus(n, d, seed=d)
            c = x[numpy.random.RandomState(d).choice(n, 24, replace=False)].copy()
            a, _, _ = oracle.lloyd_assign(x, c, metric=oracle.COS)
            q = batch(x, c, 0.3, seed=d, fresh=nq, unit=True)
        corpus = Corpus(x, c, a, metric)
        return x, c, a, q, corpus, capped_reference(10, corpus, q)[:2]
    return cached(("fixture", d, n, nq, metric), make)


def caps_of(dist, k=None):
    """The caps of a case from its uncapped lists: 0, the 5th / 25th / 50th / 75th percentile of the k-th distances, a
    value equal to one returned distance, above every distance, FLT_MAX and inf."""
    real = dist[~numpy.isnan(dist).any(axis=1)]
    kth = real[:, -1 if k is None else k - 1]
    kth = kth[kth < FLT_MAX]
    caps = [0.0] + [float(numpy.float32(numpy.percentile(kth, p))) for p in (5, 25, 50, 75)]
    caps.append(float(real[len(real) // 2, real.shape[1] // 2]))
    caps.append(float(numpy.float32(real[real < FLT_MAX].max() * 1.5)))
    return caps + [FLT_MAX, float("inf")]


def angular_cap(corpus, q, dist):
    """The float32 midpoint of the widest gap between consecutive pooled oracle distances of the uncapped lists in
    their 30th-70th percentile band; no oracle distance of any (query, row) pair lies within 4 ulp of it."""
    pool = numpy.unique(dist[numpy.isfinite(dist) & (dist < FLT_MAX)])
    band = pool[int(0.3 * len(pool)):int(0.7 * len(pool))]
    i = int(numpy.argmax(numpy.diff(band)))
    cap = numpy.float32((numpy.float64(band[i]) + numpy.float64(band[i + 1])) / 2)
    every = numpy.array([corpus._distances(row)[0] for row in numpy.ascontiguousarray(q, dtype=numpy.float32)
                         if numpy.isfinite(row).all()], numpy.float32)
    assert (numpy.abs(every - cap) > 4 * numpy.spacing(cap)).all()
    return float(cap)


def to_numpy(res):
    res = res if isinstance(res, tuple) else (res,)
    return tuple(r.cpu().numpy().view(numpy.uint32) if r.dtype == torch.int32 else r.cpu().numpy() for r in res)


class Index:
    """A KnnIndex built with verbosity 1 under the environment of a case, and everything it prints."""

    def __init__(self, x, c, a, metric="L2", env=None, monkeypatch=None, device=False):
        from kmcuda_amd import KnnIndex
        for key, v in (env or {}).items():
            monkeypatch.setenv(key, str(v))
        self.device = device
        self.out = StdoutListener()
        with self.out:
            if device:
                dev = torch.device("cuda", 0)
                a = torch.from_numpy(numpy.ascontiguousarray(a, dtype=numpy.uint32).view(numpy.int32)).to(dev)
                x, c = torch.from_numpy(x).to(dev), torch.from_numpy(c).to(dev)
            self.ix = KnnIndex(x, c, a, metric=metric, verbosity=1)
        self.text = self.out.text

    def query(self, q, k, **kw):
        out = StdoutListener()
        with out:
            if self.device:
                dev = torch.device("cuda", 0)
                for name in ("query_assignments", "probes", "allow"):
                    if kw.get(name) is not None:
                        v = numpy.ascontiguousarray(kw[name])
                        v = v.view(numpy.int32) if v.dtype == numpy.uint32 else v
                        kw[name] = torch.from_numpy(v).to(dev)
                res = to_numpy(self.ix.query(torch.from_numpy(q).to(dev), k, **kw))
                res = res if len(res) > 1 else res[0]
            else:
                res = self.ix.query(q, k, **kw)
        self.text += out.text
        self.last = out.text
        return res

    def close(self):
        self.ix.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def check_expect(text, expect):
    assert expect in ("f16", "f32", "exact", "index_half_range", "query_half_range")
    assert (EXACT in text) == (expect == "exact"), text
    assert (INDEX_HALF_RANGE in text) == (expect == "index_half_range"), text
    assert (QUERY_HALF_RANGE in text) == (expect == "query_half_range"), text


def check_capped(index, corpus, q, k, cap, qa=None, nprobe=None, probes=None, allow=None, what=""):
    """index.query(q, k, max_distance=cap, ...) == the restatement on `corpus` (the index's rows, centroids and
    assignments; the mask and the probe lists the index says it used are applied here).  Returns (neighbors, distances,
    counts, pairs in visited clusters by the restatement)."""
    probed = nprobe is not None or probes is not None
    kw = dict(max_distance=cap, return_counts=True, allow=allow)
    if probed:
        nb, dist, used, counts = index.query(q, k, nprobe=nprobe, probes=probes, return_probes=True, **kw)
        if probes is not None:
            assert (used == numpy.asarray(probes).astype(numpy.uint32)).all(), what
    else:
        nb, dist, got_qa, counts = index.query(q, k, query_assignments=qa, return_assignments=True, **kw)
    what = "%s D=%d k=%d cap=%r %s" % (what, corpus.D, k, cap, "probed" if probed else "")
    ref_corpus = corpus if allow is None else masked(corpus, allow)
    q32 = numpy.ascontiguousarray(q, dtype=numpy.float32)
    if probed:
        ref_nb, ref_dist, pairs = capped_probe_reference(k, ref_corpus, q, used, cap)
    else:
        if qa is None and corpus.metric == oracle.L2:   # 4.8 point 1: the clusters the index computed are the oracle's
            finite = numpy.isfinite(q32).all(axis=1)
            assert (got_qa[finite] == oracle.lloyd_assign(q32, corpus.c)[0][finite]).all(), what
        ref_nb, ref_dist, pairs = capped_reference(k, ref_corpus, q, got_qa, cap)
    if corpus.metric == oracle.L2:
        bad = numpy.nonzero((nb != ref_nb).any(axis=1))[0]
        assert bad.size == 0, "%s: %d lists differ from the restatement, first %d: %s vs %s" % (
            what, bad.size, bad[0], nb[bad[0]], ref_nb[bad[0]])
        bad = numpy.nonzero((bits(dist) != bits(ref_dist)).any(axis=1))[0]
        assert bad.size == 0, "%s: %d distance rows differ from the restatement, first %d: %s vs %s" % (
            what, bad.size, bad[0], dist[bad[0]], ref_dist[bad[0]])
    else:
        has = ~numpy.isnan(ref_dist).all(axis=1)
        assert (nb[~has] == NONE).all() and numpy.isnan(dist[~has]).all(), what
        filler = ref_dist == FLT_MAX
        assert (filler == (dist == FLT_MAX)).all() and (nb[filler] == 0).all(), what
        assert (numpy.isnan(dist) == numpy.isnan(ref_dist)).all(), what
        # (the fillers are equal: the allowance is for the real entries -- index 0 of a filler is a row like any other)
        allowed = assert_knn_only_acos_matters(corpus.x, nb[has], ref_nb[has], what, queries=q32[has])
        print("angular allowance: %d of %d rows (%s)" % (allowed, len(q), what))
        for i, j in zip(*numpy.nonzero(~filler & ~numpy.isnan(ref_dist))):
            want = numpy.float32(oracle.distance(q32[i], corpus.x[nb[i, j]], metric=oracle.COS))
            assert abs(dist[i, j] - want) <= 2 * numpy.spacing(max(dist[i, j], want)), (what, i, j, dist[i, j], want)
    c32 = numpy.float32(min(cap, FLT_MAX))
    assert counts.dtype == numpy.uint32 and (counts == (ref_dist <= c32).sum(axis=1)).all(), what
    real = dist <= c32
    assert (real[:, :-1] >= real[:, 1:]).all() and (nb[~real & ~numpy.isnan(dist)] == 0).all(), what   # real entries first
    return nb, dist, counts, pairs


def same(got, want, what=""):
    assert (got[0] == want[0]).all() and (bits(got[1]) == bits(want[1])).all(), what


# ---- paths x caps, and the identity at FLT_MAX / inf ------------------------------------------------------------------
@pytest.mark.parametrize("d,path", [(16, "f16"), (256, "f16"), (512, "f16"), (16, "f32"), (256, "f32"), (16, "exact"),
                                    (1100, "exact_wide")])
def test_paths_and_caps(d, path, monkeypatch):
    x, c, a, q, corpus, ref = fixture(d, n=1500 if d <= 256 else 1200)
    with Index(x, c, a, env=PATHS.get(path, {}), monkeypatch=monkeypatch) as ix:
        plain = ix.query(q, 10)
        same(plain, ref, path)
        cut = []
        for cap in caps_of(ref[1]):
            nb, dist, counts, _ = check_capped(ix, corpus, q, 10, cap, what=path)
            cut.append(int(counts.sum()))
            if cap >= FLT_MAX:
                same((nb, dist), plain, (path, cap))
        check_expect(ix.text, "exact" if path == "exact_wide" else path)
    assert 0 < cut[0] < cut[1] < cut[2] < cut[3] < cut[4] < cut[6] == cut[7] == cut[8] == ref[1].size


@pytest.mark.parametrize("d,path", [(16, "f16"), (256, "f16"), (768, "f16"), (16, "f32"), (16, "exact")])
def test_angular(d, path, monkeypatch):
    x, c, a, q, corpus, ref = fixture(d, n=1200, nq=80, metric="angular")
    cap = angular_cap(corpus, q, ref[1])
    with Index(x, c, a, metric="angular", env=PATHS[path], monkeypatch=monkeypatch) as ix:
        _, _, counts, _ = check_capped(ix, corpus, q, 10, cap, what=path)
        assert 0 < counts.sum() < ref[1].size
        check_capped(ix, corpus, q, 10, FLT_MAX, what=path)
        check_expect(ix.text, path)


# ---- k ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["f16", "exact"])
def test_k(path, monkeypatch):
    x, c, a, q, corpus, ref = fixture(16)
    median = float(numpy.median(ref[1][:, 9]))
    with Index(x, c, a, env=PATHS[path], monkeypatch=monkeypatch) as ix:
        for k in (1, 2, 65, 200):
            for cap in (median, float(numpy.median(ref[1][:, 0]))):
                nb, dist, counts, _ = check_capped(ix, corpus, q, k, cap, what=path)
            assert (counts < k).any() and counts.any()
            # return_distances=False, with and without the counts
            only = ix.query(q, k, max_distance=cap, return_distances=False)
            assert isinstance(only, numpy.ndarray) and (only == nb).all()
            two = ix.query(q, k, max_distance=cap, return_distances=False, return_counts=True)
            assert len(two) == 2 and (two[0] == nb).all() and (two[1] == counts).all()
        # k = n_clustered under a cap: a filler tail behind the rows within it
        few = numpy.ascontiguousarray(q[:24])
        nb, dist, counts, _ = check_capped(ix, corpus, few, len(x), median, what=path)
        assert 0 < counts.max() < len(x) and (dist[:, -1] == FLT_MAX).all()
        # no cap: the counts are the entries below FLT_MAX
        plain = ix.query(few, 5, return_counts=True)
        assert len(plain) == 3 and (plain[2] == 5).all()


# ---- probed -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["f16", "exact"])
def test_probed(path, monkeypatch):
    x, c, a, q, corpus, ref = fixture(16)
    K = len(c)
    caps = [float(numpy.percentile(ref[1][:, 9], p)) for p in (25, 75)] + [FLT_MAX]
    rs = numpy.random.RandomState(3)
    own = oracle.lloyd_assign(q, c)[0]
    given = numpy.concatenate([own[:, None], rs.randint(0, K + 1, (len(q), 4))], axis=1).astype(numpy.uint32)
    with Index(x, c, a, env=PATHS[path], monkeypatch=monkeypatch) as ix:
        for cap in caps:
            for p in (1, 3):
                check_capped(ix, corpus, q, 10, cap, nprobe=p, what=path)
            check_capped(ix, corpus, q, 10, cap, probes=given, what=path)
            nb, dist, _, _ = check_capped(ix, corpus, q, 10, cap, nprobe=K, what=path)
            used = ix.query(q, 10, nprobe=K, return_probes=True, max_distance=cap)[2]
            exact = check_capped(ix, corpus, q, 10, cap, qa=numpy.ascontiguousarray(used[:, 0]), what=path)
            same((nb, dist), exact, (path, cap))
        same(ix.query(q, 10, nprobe=3, max_distance=float("inf")), ix.query(q, 10, nprobe=3), path)
        check_expect(ix.text, path)


# ---- masked -----------------------------------------------------------------------------------------------------------
def masks(a, K):
    rs = numpy.random.RandomState(9)
    half = rs.rand(len(a)) < 0.5
    emptied = ~numpy.isin(a, [1, 5, 6, 17])
    return {"half": half, "emptied clusters": emptied & (rs.rand(len(a)) < 0.8), "none": numpy.zeros(len(a), bool)}


@pytest.mark.parametrize("path", ["f16", "exact"])
@pytest.mark.parametrize("name", ["half", "emptied clusters", "none"])
def test_masked(name, path, monkeypatch):
    x, c, a, q, corpus, ref = fixture(16)
    mask = masks(a, len(c))[name]
    cap = float(numpy.percentile(ref[1][:, 9], 60))
    with Index(x, c, a, env=PATHS[path], monkeypatch=monkeypatch) as ix:
        for r in (cap, FLT_MAX):
            nb, dist, counts, _ = check_capped(ix, corpus, q, 10, r, allow=mask, what=(path, name))
            check_capped(ix, corpus, q, 10, r, allow=mask, nprobe=3, what=(path, name))
            if name == "none":
                # (at r = FLT_MAX a filler's distance is <= r: the count's rule, `distance <= r`, takes it for an entry)
                assert (nb == 0).all() and (dist == FLT_MAX).all() and (counts == (0 if r < FLT_MAX else 10)).all()
            else:
                assert mask[nb[dist <= numpy.float32(r)]].all() and counts.any()
        same(ix.query(q, 10, allow=mask, max_distance=float("inf")), ix.query(q, 10, allow=mask), (path, name))
        check_expect(ix.text, path)


# ---- fp16x2 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("strict", [False, True])
def test_fp16x2(d, strict, monkeypatch):
    x, c, a = half_case(d, "L2")
    q = batch(x, c, 0.15, seed=92, fresh=100)
    qa = oracle.lloyd_assign(q.astype(numpy.float32), c.astype(numpy.float32))[0]
    corpus = cached(("half corpus", d, strict), lambda: Corpus(x, c, a, half2=True) if strict else
                    Corpus(x.astype(numpy.float32), c.astype(numpy.float32), a))
    ref = capped_reference(10, corpus, q, qa)
    env = {"KMCUDA_AMD_FP16_STRICT": 1} if strict else {}
    with Index(x, c, a, env=env, monkeypatch=monkeypatch) as ix:
        plain = ix.query(q, 10, query_assignments=qa)
        same(plain, ref, (d, strict))
        for cap in (0.0, float(numpy.percentile(ref[1][:, 9], 30)), float(ref[1][7, 4]), float("inf")):
            got = check_capped(ix, corpus, q, 10, cap, qa=qa, what=("half", strict))
            if cap >= FLT_MAX:
                same(got, plain, (d, strict))
        check_expect(ix.text, "exact" if strict else "f16")
    if strict:
        assert (bits(ref[1]) != bits(oracle.knn_query(10, x, c, a, q, query_assignments=qa)[1])).any()


# ---- edges of the host path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["f16", "f32", "exact"])
def test_chunks_and_a_chunk_of_nan_queries(path, monkeypatch):
    x, c, a, _, corpus, ref = fixture(16)
    q = batch(x, c, 0.05, seed=5, fresh=200)
    assert len(q) == 250
    q[64:128, 7] = numpy.nan
    cap = float(numpy.percentile(ref[1][:, 9], 40))
    with Index(x, c, a, env=PATHS[path], monkeypatch=monkeypatch) as ix:
        whole = check_capped(ix, corpus, q, 10, cap, what=path)
        monkeypatch.setenv("KMCUDA_AMD_KNN_QUERY_CHUNK", "64")
        chunked = check_capped(ix, corpus, q, 10, cap, what=path)
        if path != "f32":   # (there is no f32-filtered probe search: it would print the exact search's line)
            probed = check_capped(ix, corpus, q, 10, cap, nprobe=2, what=path)
            assert (probed[2][64:128] == 0).all()
        check_expect(ix.text, path)
    same(whole, chunked, path)
    assert (whole[2] == chunked[2]).all() and (whole[2][64:128] == 0).all()
    assert (whole[0][64:128] == NONE).all() and numpy.isnan(whole[1][64:128]).all()


@pytest.mark.parametrize("d", [64, 512])
def test_beyond_the_half_range(d, monkeypatch):
    """A corpus beyond the half range (the index leaves the f16 filter), and one chunk of a batch that leaves it."""
    n = 1500 if d == 64 else 1200
    x, c, a = cached(("2e5", d), lambda: blobs(n, d, 24, 2e5, seed=d + 137, spread=0.05))
    q = batch(x, c, 0.05 * 2e5, seed=d, fresh=100)
    corpus = cached(("2e5 corpus", d), lambda: Corpus(x, c, a))
    ref = capped_reference(10, corpus, q)
    with Index(x, c, a, monkeypatch=monkeypatch) as ix:
        for cap in (float(numpy.percentile(ref[1][:, 9], 40)), FLT_MAX):
            check_capped(ix, corpus, q, 10, cap, what="2e5")
        check_expect(ix.text, "index_half_range")
    x, c, a, q, corpus, ref = fixture(d, n=1500 if d <= 256 else 1200)
    q = q.copy()
    q[100, 5] = 1e6
    monkeypatch.setenv("KMCUDA_AMD_KNN_QUERY_CHUNK", "64")
    with Index(x, c, a, monkeypatch=monkeypatch) as ix:
        check_capped(ix, corpus, q, 10, float(numpy.percentile(ref[1][:, 9], 40)), what="chunk")
        assert ix.text.count(QUERY_HALF_RANGE) == 1


@pytest.mark.parametrize("path", ["f16", "exact"])
def test_device_tensors(path, monkeypatch):
    x, c, a, q, corpus, ref = fixture(16)
    cap = float(numpy.percentile(ref[1][:, 9], 40))
    mask = masks(a, len(c))["half"]
    with Index(x, c, a, env=PATHS[path], monkeypatch=monkeypatch, device=True) as ix:
        check_capped(ix, corpus, q, 10, cap, what="device")
        check_capped(ix, corpus, q, 10, cap, nprobe=3, what="device")
        check_capped(ix, corpus, q, 10, cap, allow=mask.view(numpy.uint8), what="device")
        dev = torch.device("cuda", 0)
        res = ix.ix.query(torch.from_numpy(q).to(dev), 10, max_distance=cap, return_counts=True)
        assert all(r.is_cuda for r in res) and res[2].dtype == torch.int32 and res[2].shape == (len(q),)
        check_expect(ix.text, path)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("path", ["f16", "exact"])
def test_mask_probes_and_cap_in_one_chunk_loop(path, device, monkeypatch):
    """allow, nprobe and max_distance together over four chunks (the last one partial): the restatement's lists, and
    bit for bit those of the same call in one chunk."""
    x, c, a, _, corpus, ref = fixture(16)
    q = batch(x, c, 0.05, seed=5, fresh=200)
    assert len(q) == 250
    mask = masks(a, len(c))["half"].view(numpy.uint8)
    cap = float(numpy.percentile(ref[1][:, 9], 60))
    with Index(x, c, a, env=PATHS[path], monkeypatch=monkeypatch, device=device) as ix:
        whole = check_capped(ix, corpus, q, 10, cap, allow=mask, nprobe=3, what=(path, device, "whole"))
        monkeypatch.setenv("KMCUDA_AMD_KNN_QUERY_CHUNK", "64")
        chunked = check_capped(ix, corpus, q, 10, cap, allow=mask, nprobe=3, what=(path, device, "chunked"))
        check_expect(ix.text, path)
    same(whole, chunked, (path, device))
    assert (whole[2] == chunked[2]).all() and 0 < whole[2].sum() < whole[0].size


@pytest.mark.parametrize("tight", [0, 1])
@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_query_order_and_centroid_bounds(order, tight, monkeypatch):
    x, c, a, q, corpus, ref = fixture(16)
    env = {"KMCUDA_AMD_KNN_ORDER": order, "KMCUDA_AMD_KNN_TIGHT": tight}
    with Index(x, c, a, env=env, monkeypatch=monkeypatch) as ix:
        for cap in (float(numpy.percentile(ref[1][:, 9], 40)), FLT_MAX):
            check_capped(ix, corpus, q, 10, cap, what=env)
        check_expect(ix.text, "f16")


@pytest.mark.parametrize("path", ["f16", "f32", "exact"])
def test_wrong_but_legal_query_assignments(path, monkeypatch):
    """Tie-free queries: any cluster id gives the list of the computed clusters (the prune is rigorous under the cap)."""
    x, c, a, q, corpus, ref = fixture(16)
    free = numpy.array([len(set(corpus._distances(row)[0])) == corpus.N for row in q])
    q = numpy.ascontiguousarray(q[free])
    assert len(q) >= 100
    cap = float(numpy.percentile(ref[1][:, 9], 40))
    rs = numpy.random.RandomState(11)
    with Index(x, c, a, env=PATHS[path], monkeypatch=monkeypatch) as ix:
        base = check_capped(ix, corpus, q, 10, cap, what=path)
        for qa in (rs.randint(0, len(c), len(q)), numpy.zeros(len(q)), numpy.full(len(q), len(c) - 1)):
            got = check_capped(ix, corpus, q, 10, cap, qa=qa.astype(numpy.uint32), what=path)
            same(got, base, path)


# ---- a live index -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["f16", "exact"])
def test_after_add_and_remove(path, monkeypatch):
    x, c, a, q, corpus, ref = fixture(16)
    cap = float(numpy.percentile(ref[1][:, 9], 40))
    rs = numpy.random.RandomState(13)
    gone = rs.choice(len(x), 300, replace=False)
    a2 = a.copy()
    a2[gone] = len(c)
    with Index(x[:1000], c, a[:1000], env=PATHS[path], monkeypatch=monkeypatch) as ix:
        ix.ix.add(x[1000:], a[1000:])
        added = check_capped(ix, corpus, q, 10, cap, what="added")
        assert ix.ix.remove(gone) == 300
        removed = check_capped(ix, corpus.with_assignments(a2), q, 10, cap, what="removed")
    with Index(x, c, a, env=PATHS[path], monkeypatch=monkeypatch) as fresh:
        same(added, fresh.query(q, 10, max_distance=cap), path)
    with Index(x, c, a2, env=PATHS[path], monkeypatch=monkeypatch) as fresh:
        same(removed, fresh.query(q, 10, max_distance=cap), path)
        same(removed, fresh.query(q, 10, max_distance=cap, nprobe=len(c)), path)


# ---- the cap reaches the prune ----------------------------------------------------------------------------------------
def visited_pairs(text):
    found = re.findall(r"k-NN index capped query: (\d+) pairs in visited clusters", text)
    assert len(found) == 1, text
    return int(found[0])


@pytest.mark.parametrize("path", ["exact", "f16"])
def test_the_cap_reaches_the_prune(path, monkeypatch):
    """A cap applied to a finished list would visit what the uncapped search visits."""
    x, c, a, q, cap = prune_fixture()
    corpus = cached("prune corpus", lambda: Corpus(x, c, a))
    monkeypatch.setenv("KMCUDA_AMD_KNN_STATS", "1")
    with Index(x, c, a, env=PATHS[path], monkeypatch=monkeypatch) as ix:
        _, _, _, want = check_capped(ix, corpus, q, 10, cap, what=path)
        capped = visited_pairs(ix.last)
        _, _, _, want_all = check_capped(ix, corpus, q, 10, FLT_MAX, what=path)
        uncapped = visited_pairs(ix.last)
        ix.query(q, 10)
        assert "capped query" not in ix.last   # the line is the capped call's alone
        check_expect(ix.text, path)
    print("pairs in visited clusters (%s): %d capped (restatement %d), %d at FLT_MAX (restatement %d)" % (
        path, capped, want, uncapped, want_all))
    assert want < want_all
    if path == "exact":
        assert capped == want and uncapped == want_all
    else:
        assert capped <= want and uncapped <= want_all
    assert capped < uncapped
