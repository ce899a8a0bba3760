"""The numpy restatement of weighted k-means++ seeding (tests/_weighted_seed_ref.py) against the C oracle where the two
must agree -- constant power-of-two weights scale every term, sum and threshold exactly, so the restated rows are the
oracle's unweighted seeds bit for bit -- and the conditions the GPU tests' fixtures have to meet, asserted on the
restatement's per-step records so that no GPU case passes vacuously.  No GPU."""
import collections

import numpy
import pytest

import oracle
import _weighted_seed_ref as ref


def _oracle_seeds(rows, seed):
    x, metric = ref.rows_fixture(rows)
    return oracle.init_centroids(x, ref.K, "kmeans++", seed, oracle.COS if metric == "cos" else oracle.L2)


@pytest.mark.parametrize("rows", ref.ROWS)
def test_constant_weights_give_the_oracle_s_seeds(rows):
    """w = 1, 2^-3 and 2^5 on every row fixture, seeds 3 and 11 and one whose first choice * N is below 100.  Where
    the walk leaves [1, N] (the NaN fixture: a NaN term makes every comparison fail) the oracle returns its error at
    the same step."""
    x, _ = ref.rows_fixture(rows)
    x32 = numpy.asarray(x, numpy.float32)
    small = ref.small_choice_seed(rows)
    for seed in (3, 11, small):
        try:
            want = _oracle_seeds(rows, seed)
        except ValueError:
            want = None
        for weights in ("ones", "pow2:-3", "pow2:5"):
            got = ref.restated(rows, weights, ref.K, seed)
            if seed == small:
                assert got["steps"][0]["branch"] == "small"
            if want is None:
                assert got["failed"] is not None, (seed, weights)
                continue
            assert got["failed"] is None, (seed, weights, got["failed"])
            assert numpy.array_equal(x32[got["rows"]].view(numpy.uint32), want.view(numpy.uint32)), (seed, weights)


def test_the_nan_fixture_has_a_seed_of_each_kind():
    """One srand() seed with which the NaN fixture's walk stays in range and one with which it returns j = 0; the
    oracle agrees on both."""
    good, bad = ref.nan_walk_seeds()
    x, _ = ref.rows_fixture("nan-5003x32")
    got = ref.restated("nan-5003x32", "decades", ref.K, good)
    assert got["failed"] is None and len(got["rows"]) == ref.K
    assert all(s["nonfinite"] for s in got["steps"])
    got = ref.restated("nan-5003x32", "decades", ref.K, bad)
    assert got["failed"] is not None and got["failed"][1] == 0
    _oracle_seeds("nan-5003x32", good)
    with pytest.raises(ValueError):
        _oracle_seeds("nan-5003x32", bad)


def _steps(rows, weights):
    got = ref.restated(rows, weights)
    return got, got["steps"]


@pytest.mark.parametrize("rows", ["l2-5003x32", "cos-5003x32"])
def test_binades_never_fit_the_exact_window(rows):
    got, steps = _steps(rows, "binades")
    assert len(steps) == ref.K - 1
    assert all(ref.outside_window(s, got["log2n"]) for s in steps)


@pytest.mark.parametrize("rows", ["l2-5003x32", "l2-5003x30", "fp16-5003x32", "wide-2000x320", "l2-8209x32"])
def test_decades_on_l2_rows_fit_the_window_with_nothing_listed(rows):
    """What lets the GPU test ask for steps decided on the device."""
    got, steps = _steps(rows, "decades")
    assert all(not ref.outside_window(s, got["log2n"]) and s["under_cut"] == 0 and not s["nonfinite"] for s in steps)


@pytest.mark.parametrize("rows", ["l2-5003x32", "cos-5003x32", "l2-8209x32"])
def test_few_light_lists_a_few(rows):
    got, steps = _steps(rows, "few-light")
    listed = [s["under_cut"] for s in steps]
    print(listed)
    assert sum(1 <= c <= ref.LIST_CAP for c in listed) * 2 >= len(steps)
    assert max(listed) <= ref.LIST_CAP


def test_many_light_overflows_the_list():
    _, steps = _steps("l2-5003x32", "many-light")
    assert any(s["under_cut"] > ref.LIST_CAP for s in steps)


def test_underflow_has_subnormal_and_zero_terms():
    _, steps = _steps("l2-5003x32", "underflow")
    assert all(s["subnormal"] > 0 and s["zero"] > 0 for s in steps)
    assert steps[0]["subnormal"] >= 2000


def test_overflow_has_infinite_terms():
    """From the first step on, for most of the steps: a step whose walk runs forward into an infinite term seeds that
    row, whose term is 0 from then on, so the last steps may be finite again -- the return from them is run too."""
    got, steps = _steps("big-5003x32", "overflow")
    flags = [s["nonfinite"] for s in steps]
    print(flags)
    assert flags[0] and sum(flags) * 2 > len(flags)
    assert flags == sorted(flags, reverse=True)   # (once the infinite terms are used up they do not come back)


@pytest.mark.parametrize("rows,weights", [p for p in ref.PAIRS if p[0] != "nan-5003x32"])
def test_the_weights_change_the_seeds(rows, weights):
    """Every non-constant family draws other rows than the unweighted chooser on the same rows and stream.  (The NaN
    fixture is left out: with a NaN term the walk ends at row choice * N whatever the terms are.)"""
    assert weights in ref.NON_CONSTANT
    a, b = ref.restated(rows, weights), ref.restated(rows, "ones")
    assert a["rows"][0] == b["rows"][0]
    assert not numpy.array_equal(a["rows"], b["rows"])


def test_every_branch_of_the_walk_is_taken():
    taken = collections.Counter()
    for rows, weights in ref.PAIRS:
        taken.update(s["branch"] for s in ref.restated(rows, weights)["steps"])
    for rows in ref.ROWS:
        taken.update(s["branch"] for s in ref.restated(rows, "ones", ref.K, ref.small_choice_seed(rows))["steps"])
    print(dict(taken))
    assert taken["small"] > 0 and taken["forward"] > 0 and taken["backward"] > 0


def test_no_pair_fails_at_the_default_seed_but_the_walk_can():
    """The pairs' restated seeds are complete at the default seed (the GPU tests then compare K rows)."""
    for rows, weights in ref.PAIRS:
        if rows == "nan-5003x32":
            continue
        got = ref.restated(rows, weights)
        assert got["failed"] is None and len(got["rows"]) == ref.K, (rows, weights)
