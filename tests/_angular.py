"""What may differ between the device and the oracle under the angular metric, and what may not.

`acosf` is libm in the oracle, ocml on the GPU and CUDA's in the reference (parity-unpinned), so a row whose
two nearest centroids are within a last place of each other in the oracle's OWN arithmetic may land on either.  Anything
else is a defect -- in particular a row whose candidates both sit at distance 0: the clamp `p >= 1 ? 0 : acos(p)`
(metric_abstraction.h:171-177) involves no acos, the lowest index wins (tests/test_gpu_angular_clamp.py)."""
import numpy

import oracle


def assert_only_acos_matters(x, c, got, ref, what="", max_fraction=2e-3):
    """got / ref: assignments of the rows x against the centroids c (device / oracle).  Returns the number of rows that
    differ -- every one of them an acos last-place matter, never a clamp tie, and no more than max_fraction of the rows."""
    got, ref = numpy.asarray(got), numpy.asarray(ref)
    bad = numpy.nonzero(got != ref)[0]
    assert bad.size <= max_fraction * len(ref), "%s: %d of %d rows differ" % (what, bad.size, len(ref))
    k = c.shape[0]
    for i in bad:
        assert got[i] < k and ref[i] < k, (what, int(i), int(got[i]), int(ref[i]))
        dg = oracle.distance(x[i], c[got[i]], metric=oracle.COS)
        dr = oracle.distance(x[i], c[ref[i]], metric=oracle.COS)
        assert not (dg == 0.0 and dr == 0.0), "%s: row %d: a tie at the clamp went to %d, not %d" % (what, i, got[i], ref[i])
        assert abs(dg - dr) <= 2 * numpy.spacing(numpy.float32(max(dg, dr))), \
            "%s: row %d: distances %r (device's %d) and %r (oracle's %d) are not a last-place matter" % (
                what, i, dg, got[i], dr, ref[i])
    return int(bad.size)


def assert_knn_only_acos_matters(x, got, ref, what="", queries=None):
    """got / ref: k-NN lists of the rows x (device / oracle); with `queries`, the lists of those rows among the rows x
    (row i of got / ref belongs to queries[i]).  An entry may differ only where the two lists' oracle
    distances, each list in sorted order, agree within 2 float32 ulp at that slot.  Every other entry is equal.  (Unlike
    an assignment, a tie at the clamp's 0 is no exception here: which clusters a query visits depends on the acos of the
    centroid distances and radii, and a candidate at the heap's top distance is pushed when visited.)  Returns the
    number of rows that differ."""
    x = numpy.asarray(x, dtype=numpy.float32)
    q = x if queries is None else numpy.asarray(queries, dtype=numpy.float32)
    got, ref = numpy.asarray(got), numpy.asarray(ref)
    rows = numpy.nonzero((got != ref).any(axis=1))[0]
    for i in rows:
        assert (got[i] < len(x)).all() and (ref[i] < len(x)).all(), (what, int(i), got[i], ref[i])
        dg = numpy.sort([oracle.distance(q[i], x[j], metric=oracle.COS) for j in got[i]]).astype(numpy.float32)
        dr = numpy.sort([oracle.distance(q[i], x[j], metric=oracle.COS) for j in ref[i]]).astype(numpy.float32)
        for s in numpy.nonzero(got[i] != ref[i])[0]:
            assert abs(dg[s] - dr[s]) <= 2 * numpy.spacing(max(dg[s], dr[s])), \
                "%s: row %d slot %d: distances %r / %r are not a last-place matter" % (what, i, s, dg, dr)
    return int(rows.size)
