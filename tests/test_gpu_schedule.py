"""The schedule of kmeans_cuda() (kmcuda_amd/csrc/kmcuda_api.cpp: Job::run; DESIGN.md 4.4, "The schedule, row by row"):
one call per row of that table, and per call the phase lines a caller sees at verbosity=1 -- as literal text in literal
order, with the iteration lines between them counted -- and the results the documents promise to be the same run.

Rows: blobs in three latent dimensions embedded in 24 features (tests/test_gpu_assign_paths.py: such rows keep moving
where plain blobs stop within 5-15 iterations), 3000 x 24 fp32, K = 40, yinyang_t = 0.1 (G = 4), init="random",
seed 3, tolerance 0.005 (15 rows).  Chosen with the oracle's kmeans(): its plain Lloyd run takes 25 iterations,

    3000 411 233 | 155 132 118 106 108 105 86 78 79 56 42 34 29 33 25 22 17 21 22 21 19 11

-- 3 down to the hand-over point (233 <= 11 % of 3000 = 330 < 411; 233 > 15, so the run goes on) and 22 after it.  The
other thresholds the rows need lie as far from a count: tolerance 0.08 (240 rows) stops the run AT the hand-over test,
tolerance 0.12 (360 rows) is "too high" and stops at iteration 3 as well, KMCUDA_AMD_YY_SWITCH=0.05 (150 rows) is
first met by iteration 5 (132; iteration 4 has 155), and the reference's bounds take over behind iteration 7: the host
learns iteration 5's count with iteration 6 enqueued, update and all (Job::lloyd speculates), so iteration 7 is the
first whose update it can hold back -- three iterations behind the "carrying" line, then the bounds' refresh.

What is exact and what is not: a run under KMCUDA_AMD_EXACT_UPDATE=1 is the oracle's arithmetic, so its counts are the
ones above.  The default update sums in another order: its counts are its own, asserted equal between
the rows that are the same run and at least the four iterations behind the hand-over point that the shape was chosen
for.  Rows whose arithmetic differs from the default run's (the reference's bounds, three shards, the weighted update)
are held to what tests/test_gpu_yinyang.py holds them to: the same iteration lines up to the hand-over point and a
final inertia within 1e-3 of the default run's (test_schedules_agree_on_a_row_cached_shape).  Every row of the table
is reached at this shape."""
import os

import numpy
import pytest

import oracle
from test_gpu_kmeans import StdoutListener

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, D, K, SEED, TOLERANCE = 3000, 24, 40, 3, 0.005
BEFORE, AFTER = 3, 22   # the oracle's iterations down to the hand-over point and after it (the module docstring)

RUN = "running Lloyd until reassignments drop below 330"
GOES_ON = "Lloyd goes on"
GOES_ON_CARRYING = "Lloyd goes on, carrying per-sample distance bounds from pass to pass"
CARRYING = "carrying per-sample distance bounds from pass to pass"
REFRESH = "refreshing Yinyang bounds..."
TOO_FEW = "too few clusters for this yinyang_t => Lloyd"
TOO_HIGH = "tolerance is too high (>= 0.11) => Lloyd"
PHASE_LINES = (RUN, GOES_ON, GOES_ON_CARRYING, CARRYING, REFRESH, TOO_FEW, TOO_HIGH)

GROUPS = "<the group clustering's own lines>"   # (numbered from 1 again: the reference prints them too, kmeans.cu:1062-1100)
MANY = "<iterations: at least 4>"
SOME = "<iterations: at least 1>"
SWITCHES = ("KMCUDA_AMD_CARRY", "KMCUDA_AMD_YY", "KMCUDA_AMD_YY_SWITCH", "KMCUDA_AMD_EXACT_UPDATE", "KMCUDA_AMD_SPECULATE",
            "KMCUDA_AMD_VIRTUAL_SHARDS", "KMCUDA_AMD_FP16_STRICT", "KMCUDA_AMD_TIMING")

# row of the table -> (environment, arguments that differ, the lines of verbosity=1)
DEFAULT_LINES = [RUN, BEFORE, GROUPS, GOES_ON, 1, CARRYING, MANY]
ROWS = {
    "too-few-clusters": ({}, dict(yinyang_t=0), [TOO_FEW, MANY]),
    "tolerance-too-high": ({}, dict(tolerance=0.12), [TOO_HIGH, BEFORE]),
    "stops-at-the-hand-over": ({}, dict(tolerance=0.08), [RUN, BEFORE]),
    "default": ({}, {}, DEFAULT_LINES),
    "default-silent": ({}, dict(verbosity=0), []),
    "carry-0": ({"KMCUDA_AMD_CARRY": "0"}, {}, [RUN, BEFORE, GROUPS, GOES_ON, MANY]),
    "carry-1": ({"KMCUDA_AMD_CARRY": "1"}, {}, [RUN, BEFORE, GROUPS, GOES_ON_CARRYING, MANY]),
    "yy-reference": ({"KMCUDA_AMD_YY": "reference"}, {}, [RUN, BEFORE, GROUPS, REFRESH, MANY]),
    "yy-switch-0.05": ({"KMCUDA_AMD_YY_SWITCH": "0.05"}, {}, [RUN, BEFORE, GROUPS, GOES_ON, 1, CARRYING, 3, REFRESH, SOME]),
    "exact-update": ({"KMCUDA_AMD_EXACT_UPDATE": "1"}, {}, [RUN, BEFORE, GROUPS, REFRESH, MANY]),
    "exact-update-yy-carry": ({"KMCUDA_AMD_EXACT_UPDATE": "1", "KMCUDA_AMD_YY": "carry"}, {},
                              [RUN, BEFORE, GROUPS, GOES_ON, 1, CARRYING, AFTER - 1]),
    "speculate-0": ({"KMCUDA_AMD_SPECULATE": "0"}, {}, DEFAULT_LINES),
    "virtual-shards-3": ({"KMCUDA_AMD_VIRTUAL_SHARDS": "3"}, {}, DEFAULT_LINES),
    "weights-of-1": ({}, dict(sample_weight=numpy.ones(N, numpy.float32)), DEFAULT_LINES),
}


def _rows():
    rs = numpy.random.RandomState(1)
    q, blobs = 3, max(8, K // 2)
    centres = rs.rand(blobs, q) * 5.0
    z = centres[rs.randint(0, blobs, N)] + rs.randn(N, q)
    return (z @ rs.randn(q, D) + 0.05 * rs.randn(N, D)).astype(numpy.float32)


class Run:
    """One call: what it printed, parsed, and what it returned."""

    def __init__(self, text, centroids, assignments):
        self.text, self.centroids, self.assignments = text, centroids, assignments
        self.tokens, self.main, self.group_lines = [], [], []
        in_groups = False
        for line in text.splitlines():
            if line in PHASE_LINES:
                self.tokens.append(line)
                in_groups = False
            elif line.startswith("iteration "):
                number = int(line.split()[1].rstrip(":"))
                if not in_groups and number == 1 and self.main:
                    in_groups = True
                    self.tokens.append(GROUPS)
                if in_groups:
                    self.group_lines.append(line)
                    continue
                self.main.append(line)
                if self.tokens and isinstance(self.tokens[-1], int):
                    self.tokens[-1] += 1
                else:
                    self.tokens.append(1)
        numbers = [int(line.split()[1].rstrip(":")) for line in self.main]
        assert numbers == list(range(1, len(numbers) + 1)), text   # the call's own lines count 1, 2, 3, ...

    def counts(self):
        return [int(line.split()[2]) for line in self.main]


@pytest.fixture(scope="module")
def runs():
    """Every row's call, made once; the oracle's plain Lloyd run beside them."""
    from kmcuda_amd import kmeans_cuda
    x = _rows()
    saved = {name: os.environ.pop(name, None) for name in SWITCHES}
    out = {}
    try:
        for row, (env, args, _) in ROWS.items():
            os.environ.update(env)
            try:
                kw = dict(init="random", seed=SEED, tolerance=TOLERANCE, yinyang_t=0.1, device=1, verbosity=1)
                kw.update(args)
                listener = StdoutListener()
                with listener:
                    centroids, assignments = kmeans_cuda(x, K, **kw)
            finally:
                for name in env:
                    del os.environ[name]
            out[row] = Run(listener.text, centroids, assignments)
            print("%s: %s" % (row, out[row].tokens))
    finally:
        for name, value in saved.items():
            if value is not None:
                os.environ[name] = value
    ocen, oasg, olog = oracle.kmeans(x, K, init="random", seed=SEED, tolerance=TOLERANCE, yinyang_t=0)
    olog = [int(v) for v in olog]
    # the shape is what the module docstring says it is
    assert len(olog) == BEFORE + AFTER and olog[BEFORE - 1] <= 0.11 * N < olog[BEFORE - 2] and olog[BEFORE - 1] > TOLERANCE * N
    assert olog[BEFORE - 1] <= 0.08 * N and olog[BEFORE - 1] <= 0.12 * N < olog[BEFORE - 2]
    assert olog[3] > 0.05 * N >= olog[4]
    out["oracle"] = (ocen, oasg, olog)
    out["rows"] = x
    return out


def _same_outputs(a, b):
    return (a.assignments == b.assignments).all() and (a.centroids.view(numpy.uint32) == b.centroids.view(numpy.uint32)).all()


@pytest.mark.parametrize("row", list(ROWS))
def test_phase_lines(runs, row):
    """The lines of the table's row: literal text, literal order, the iteration lines between them counted."""
    got, want = runs[row].tokens, ROWS[row][2]
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        if w == MANY:
            assert isinstance(g, int) and g >= 4, (got, want)
        elif w == SOME:
            assert isinstance(g, int) and g >= 1, (got, want)
        else:
            assert g == w and type(g) is type(w), (got, want)
    if row == "default-silent":
        assert runs[row].text == ""
    if row == "too-few-clusters":   # (plain Lloyd all the way takes as many passes as the default schedule's)
        assert len(runs[row].main) == len(runs["default"].main)


@pytest.mark.parametrize("row", ["default-silent", "carry-0", "carry-1", "speculate-0"])
def test_rows_that_are_the_default_run(runs, row):
    """Carried passes against plain ones, the device's stop rule against the host's, a silent call (which replays the
    group clustering's draws) against a verbose one (which clusters): the same run, bit for bit."""
    base = runs["default"]
    assert _same_outputs(runs[row], base)
    if row != "default-silent":
        assert runs[row].main == base.main
        assert runs[row].group_lines == base.group_lines and base.group_lines


def test_default_schedule_under_the_exact_update_is_the_oracle_s_lloyd(runs):
    """KMCUDA_AMD_EXACT_UPDATE=1 with KMCUDA_AMD_YY=carry is the reference's kmeans_cuda_lloyd bit
    for bit -- counts, assignments, centroids."""
    ocen, oasg, olog = runs["oracle"]
    got = runs["exact-update-yy-carry"]
    assert got.counts() == olog
    assert (got.assignments == oasg).all()
    assert (got.centroids.view(numpy.uint32) == ocen.view(numpy.uint32)).all()
    assert runs["exact-update"].counts()[:BEFORE] == olog[:BEFORE]


@pytest.mark.parametrize("row", ["yy-reference", "yy-switch-0.05", "virtual-shards-3", "weights-of-1", "exact-update"])
def test_rows_of_another_arithmetic(runs, row):
    """The reference's bounds decide by another arithmetic than a Lloyd pass, three shards sum the update in another
    order than one, the weighted update multiplies by 1.0 on another path: the same lines up to the hand-over point
    (the strict update: the oracle's, above), then a run of its own that ends as good."""
    x, base, got = runs["rows"], runs["default"], runs[row]
    if row != "exact-update":
        assert got.main[:BEFORE] == base.main[:BEFORE]

    def inertia(r):
        return float(((x - r.centroids[r.assignments]) ** 2).sum())
    assert abs(inertia(got) / inertia(base) - 1) < 1e-3, (inertia(got), inertia(base))
