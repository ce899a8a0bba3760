"""One engine moving BETWEEN the kinds of Lloyd pass (kmcuda_amd/csrc/engine.cpp: Engine::lloyd_assign and the stage
functions it calls): a plain pass without a row cache, the pass that builds the cache, the steady state behind a plain
update and behind the update fused with the next preparation, passes that carry bounds (whole, counted, listed), an exact
pass, the f32 filter, the cache dropped and built again.  Every kind must leave or void the state the next one reads --
carry_valid_, prepared_for_, row_cache_valid_, mu_frozen_, the statistics' double buffer, the list counters -- and the other
test files check the kinds one at a time.

Bar, after EVERY pass.  L2: assignments, previous assignments and the reassignment count bit for bit against the oracle's
kmeans_assign_lloyd replayed from the pass's input state.  Angular: bit for bit against a twin loop of plain filtered
passes from the same seeds (ocml's and libm's acosf differ in the last place, so the oracle is no bit-exact reference
there; test_gpu_carry.py has the tolerance form).

Rows: blobs in three latent dimensions, embedded in D features.  Blobs, so that carried passes spare rows; overlapping
in few dimensions, so that a run over 2900 rows keeps moving for the ~20 passes of the sequence (chosen with the oracle's
kmeans(): every case moves >= 5 rows per iteration for >= 26 iterations) -- a run that stopped would compare passes that
do nothing.  The shapes are the smallest with several 128- and 256-row blocks, a ragged last block and a ragged last
centroid tile."""
import numpy
import pytest

import oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NO_LIST = 0xFFFFFFFF

# name: (N, D, K, seed of the rows, expected filter_kind())
SHAPES = {
    "a": (2900, 24, 33, 4, (1, 32)),     # narrow rows
    "b": (2900, 100, 33, 4, (1, 128)),   # D % 4 != 0: no settle kernel, the pair kernel + the exact kernel on the side stream
    "c": (2900, 256, 40, 4, (1, 256)),   # the widest register-resident width
    "d": (1500, 320, 33, 6, (2, 320)),   # the streamed filter
}


def _rows(n, d, k, seed, metric, half):
    rs = numpy.random.RandomState(seed)
    q, blobs = 3, max(8, k // 2)
    centres = rs.rand(blobs, q) * 5.0
    z = centres[rs.randint(0, blobs, n)] + rs.randn(n, q)
    x = (z @ rs.randn(q, d) + 0.05 * rs.randn(n, d)).astype(numpy.float32)
    if metric == "cos":
        x = (x / numpy.linalg.norm(x, axis=1, keepdims=True)).astype(numpy.float32)
    if half:
        x = x.astype(numpy.float16).astype(numpy.float32)
    init = x[numpy.random.RandomState(5).choice(n, k, replace=False)].copy()
    return x, init


class _Drive:
    """The loop under test (row cache off at first) and, for the angular metric, its twin of plain filtered passes."""

    def __init__(self, shape, metric, half):
        from kmcuda_amd.distributed import HipBackend, ShardedLloyd
        n, d, k, seed, self.kind = SHAPES[shape]
        self.n, self.metric = n, metric
        self.x, init = _rows(n, d, k, seed, metric, half)
        dev = torch.device("cuda", 0)
        xs = torch.from_numpy(self.x).to(dev)
        self.loops = []
        for twin in ([False] if metric == "L2" else [False, True]):
            h = xs.to(torch.float16) if half else None
            loop = ShardedLloyd(HipBackend(xs, k, metric, device_index=0, half_rows=h, row_cache=twin), n)
            loop.set_centroids(torch.from_numpy(init).to(dev))
            self.loops.append(loop)
        self.loop = self.loops[0]
        self.engine = self.loop.b.engine
        self.passes, self.fused_last = 0, False
        assert self.engine.filter_kind() == self.kind

    def step(self, what, fused=False, exact=False):
        """One iteration: the pass (exact: the exact kernels alone), the update (fused: the device-side stop rule, and
        on fp32 L2 rows the next pass's preparation in the same launch).  Then the bar."""
        b = self.loop.b
        cen_in = b.centroids.cpu().numpy().copy()
        asg_in = b.assignments.cpu().numpy().view(numpy.uint32).copy()
        if exact:
            b.assign = lambda: self.engine.lloyd_assign(b.samples, b.centroids, b.assignments, b.assignments_prev, exact=True)
        try:
            for loop in self.loops:
                if fused:
                    if not self.fused_last:   # (the plain update leaves its pass's count in the counter; the fused one clears it)
                        loop.b.reset_changed()
                    loop.step(tolerance=0.0)
                else:
                    loop.drain()   # (the report of an earlier fused iteration, while its slot is still its own)
                    loop.step()
        finally:
            if exact:
                del b.assign
        for loop in self.loops:
            loop.b.synchronize()
        self.fused_last = fused
        self.passes += 1
        where = "pass %d (%s)" % (self.passes, what)
        a = b.assignments.cpu().numpy().view(numpy.uint32)
        p = b.assignments_prev.cpu().numpy().view(numpy.uint32)
        changed = int((a != p).sum())
        if self.metric == "L2":
            ref, ref_prev, ref_changed = oracle.lloyd_assign(self.x, cen_in, assignments=asg_in)
            print("%s: %d rows moved (oracle: %d), %d assignments differ" % (where, changed, ref_changed, int((a != ref).sum())))
            assert (a == ref).all(), "%s: %d assignments differ from the oracle's" % (where, int((a != ref).sum()))
            assert (p == ref_prev).all(), "%s: previous assignments differ from the oracle's" % where
            assert changed == ref_changed and self.loop.changed_last() == ref_changed, (where, changed, ref_changed)
        else:
            t = self.loops[1].b
            ta = t.assignments.cpu().numpy().view(numpy.uint32)
            print("%s: %d rows moved, %d assignments differ from the twin's" % (where, changed, int((a != ta).sum())))
            assert (a == ta).all(), "%s: %d assignments differ from the plain loop's" % (where, int((a != ta).sum()))
            assert (p == t.assignments_prev.cpu().numpy().view(numpy.uint32)).all(), where
            assert self.loop.changed_last() == self.loops[1].changed_last() == changed, where
            assert torch.equal(b.centroids.view(torch.int32), t.centroids.view(torch.int32)), where
        assert changed > 0, "%s: the run has stopped moving -- the passes behind it would test nothing" % where
        assert self.engine.filter_kind() == self.kind, where

    def steps_1_to_7(self):
        e = self.engine
        self.step("1: plain, no row cache")
        e.set_row_cache(True)
        self.step("2: builds the row cache")
        self.step("3: steady, behind a plain update")
        self.step("4: steady, its update fused", fused=True)
        self.step("4: steady, behind the fused update", fused=True)
        assert e.carry_stats() == (0, NO_LIST)
        e.set_carry(True)
        self.step("5: whole pass, leaves bounds", fused=True)
        assert e.carry_stats() == (0, NO_LIST)     # (bounds none had moved: no list to count, nothing spared)
        self.step("6: whole pass, bounds moved, list counted", fused=True)
        # The spared-rows statistic is written by LISTED passes alone (lloyd_coarse.hpp / lloyd_wide.hip: N - list -
        # pairs, when the pass takes its rows from the list), so what step 6 shows is its count; the statistic itself is
        # asserted behind the first listed pass, the earliest point at which it can be anything but 0.
        spared, last = e.carry_stats()
        assert last <= self.n, (spared, last)
        self.step("7: listed pass")
        spared, last = e.carry_stats()
        assert spared > 0 and last < self.n, (spared, last)
        return spared

    def steps_8_to_11(self, spared, streamed):
        e = self.engine
        self.step("7: listed pass, prepared inside the pass")
        self.step("8: exact", exact=True)
        self.step("9: whole pass again (the exact pass voided the bounds)")
        assert e.carry_stats()[1] == NO_LIST
        self.step("9: counted", fused=True)
        self.step("9: listed", fused=True)
        again = e.carry_stats()[0]
        assert again > spared, (spared, again)
        if not streamed:   # (the streamed filter has one arithmetic: the switch does not reach it)
            e.set_filter("f32")
            self.step("10: the f32 filter")
            e.set_filter("f16")
        self.step("10: carried again")
        self.step("10: carried again")
        before = e.carry_stats()[0]
        e.set_row_cache(False)
        self.step("11: plain, the row cache dropped")
        assert e.carry_stats()[0] == before     # (no steady state, no bounds)
        e.set_row_cache(True)
        self.step("11: builds the row cache again")
        self.step("11: steady: whole pass, leaves bounds")
        assert e.carry_stats()[1] == NO_LIST


@pytest.mark.parametrize("case", [("a", "L2", False), ("a", "L2", True), ("a", "cos", False), ("b", "L2", False),
                                  ("c", "L2", False), ("d", "L2", False)],
                         ids=lambda c: "%s-%s-%s" % (c[0], c[1], "fp16x2" if c[2] else "fp32"))
def test_one_engine_through_every_kind_of_pass(case, monkeypatch):
    shape, metric, half = case
    # (read when the bounds are first allocated, step 5: every pass with a counted list is then a LISTED one, whatever
    #  the list's length -- the default policy's choice between the two is tests/test_boundary_cpu.py's)
    monkeypatch.setenv("KMCUDA_AMD_CARRY_MAX", "1.0")
    drive = _Drive(shape, metric, half)
    spared = drive.steps_1_to_7()
    drive.steps_8_to_11(spared, streamed=drive.kind[0] == 2)


@pytest.mark.parametrize("switch", [("KMCUDA_AMD_SETTLE", "0"), ("KMCUDA_AMD_DUO", "0"), ("KMCUDA_AMD_DUO", "2")],
                         ids=lambda s: "%s=%s" % (s[0][len("KMCUDA_AMD_"):], s[1]))
def test_steps_1_to_7_under_the_engine_s_switches(switch, monkeypatch):
    """SETTLE=0: the pair kernel + the exact kernel on the side stream instead of the one-launch settle kernel.  DUO=0: no
    duo list, stage 2 sweeps for every listed row.  DUO=2 (what conftest.py sets for the whole suite, stated here so that
    the case does not depend on it; an engine left to itself uses the list only where it pays, never at this size): the
    duo kernel on the side stream beside stage 2 in every two-stage pass."""
    monkeypatch.setenv(*switch)   # (Engine::init reads them)
    monkeypatch.setenv("KMCUDA_AMD_CARRY_MAX", "1.0")
    drive = _Drive("a", "L2", False)
    duo = []
    step = drive.step

    def step_and_count(*args, **kw):
        step(*args, **kw)
        duo.append(drive.engine.duo_rows())

    drive.step = step_and_count
    drive.steps_1_to_7()
    print("duo rows per pass:", duo)
    if switch == ("KMCUDA_AMD_DUO", "0"):
        assert duo == [0] * len(duo), duo
    if switch == ("KMCUDA_AMD_DUO", "2"):
        assert sum(duo) > 0, duo
