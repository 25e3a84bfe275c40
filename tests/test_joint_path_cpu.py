"""What the joint path checks without a device: the symbols, JointSearch replayed on synthetic step
functions errors(penalty), the argument checks of the Python layer (which come before any device
work), and the yardstick of tests/joint_path_ref.py against a case worked by hand."""
import ctypes
import math

import numpy as np
import pandas as pd
import pytest

from joint_path_ref import NO_PEAKS, PEAK_END, PEAK_START, PEAKS, joint_label_errors_ref

WIDTH, ROUNDS, TOL = 8, 20, 0.05
GAINS = (1e-3, 1e6)          # the scale of the synthetic models: the gains at penalty 0
EMPTY = 3e6                  # from here on the synthetic model has no peak
# A bracketing search knows a run of few errors only once one of its penalties is evaluated, and
# round 2 is the only round that looks everywhere: a minimum on [A, B) is found iff a penalty of
# round 2's ladder lies in it (always when B / A exceeds the ladder's ratio, 10^(9/7) here).
LADDER = [math.exp(math.log(GAINS[0]) + (math.log(GAINS[1]) - math.log(GAINS[0])) * k / (WIDTH - 1.0))
          for k in range(WIDTH)]


@pytest.fixture(scope="module")
def psd():
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd
    return peaksegdisk_amd


def test_symbols_and_exports(psd):
    from peaksegdisk_amd import _native as native
    for name in ("peakseg_hip_joint_path_max_penalties", "peakseg_hip_problem_set_pack_joint_path",
                 "peakseg_hip_problem_set_packed_joint_path_download", "peakseg_hip_joint_path_last_ms",
                 "peakseg_hip_problem_set_pack_joint_label_errors",
                 "peakseg_hip_problem_set_packed_joint_label_errors_download",
                 "peakseg_hip_joint_label_errors_last_ms"):
        assert hasattr(native.lib, name) and name in native.EXPORTED_SYMBOLS
    assert native.lib.peakseg_hip_joint_path_max_penalties() >= 16
    for name in ("joint_target_interval_dense", "joint_target_interval_reads",
                 "learn_joint_penalty_dense", "learn_joint_penalty_reads", "JointSearch",
                 "JointTargetInterval", "joint_target_interval"):
        assert name in psd.__all__ and hasattr(psd, name)
    assert hasattr(psd.ProblemSet, "joint_path") and hasattr(psd.ProblemSet, "joint_label_errors")
    # nothing to report and nothing to refuse without a set
    assert native.lib.peakseg_hip_problem_set_pack_joint_path(*[None] * 2, 0, None, 0, *[None] * 4, 0,
                                                              *[None] * 13) == -1
    assert native.lib.peakseg_hip_problem_set_pack_joint_label_errors(*[None] * 5, 0, *[None] * 5) == -1
    assert native.lib.peakseg_hip_problem_set_packed_joint_path_download(*[None] * 12) == -1
    assert native.lib.peakseg_hip_problem_set_packed_joint_label_errors_download(*[None] * 6) == -1
    ms = ctypes.c_float(-1.0)
    assert native.lib.peakseg_hip_joint_path_last_ms(ctypes.byref(ms)) == 0 and ms.value >= 0.0
    assert native.lib.peakseg_hip_joint_label_errors_last_ms(ctypes.byref(ms)) == 0 and ms.value >= 0.0


# ---- JointSearch on synthetic step functions ---------------------------------------------------

def replay(psd, errors, gains=GAINS, empty=EMPTY, width=WIDTH, tol=TOL, max_rounds=ROUNDS):
    """the search on errors(penalty) -> (result, the penalties asked round by round); peaks(penalty)
    is 1 below `empty` and 0 from there on"""
    search = psd.JointSearch(tol)
    asked = []
    for _ in range(max_rounds):
        penalties = search.next_penalties(width)
        if not penalties:
            break
        assert len(penalties) <= width
        asked.append(penalties)
        for penalty in penalties:
            peaks = 0 if gains is None or penalty >= empty else 1
            search.add(penalty, peaks, 3 * peaks, errors(penalty), 0, errors(penalty))
        if len(asked) == 1:
            assert penalties == [0.0]
            search.scale(*(gains if gains is not None else (None, None)))
    else:
        assert not search.next_penalties(width), "the search did not end within max_rounds"
    flat = [p for r in asked for p in r]
    assert len(set(flat)) == len(flat), "a penalty was asked for twice"
    result = search.result()
    assert result.rounds == len(asked) <= max_rounds
    assert list(result.models.columns) == ["penalty", "peaks", "samples_up", "errors", "fp", "fn", "round"]
    assert sorted(result.models["penalty"]) == sorted(flat)
    worse = result.models[result.models["errors"] > result.min_errors]["penalty"].to_numpy()
    logs = np.log(np.maximum(worse, 1e-300))
    assert not ((logs >= result.min_log_lambda) & (logs <= result.max_log_lambda) & (worse > 0)).any()
    return result, asked


def step(a, b, inside=0, outside=2):
    return lambda x: inside if a <= x < b else outside


def within(log_end, value, tol=TOL):
    return abs(log_end - math.log(value)) <= math.log(1.0 + tol) + 1e-12


@pytest.mark.parametrize("a, b", [(1e-3, 2e-2), (2e-3, 9e5), (0.5, 40.0), (7.0, 7.5), (3e4, 1e5),
                                  (1.234e2, 1.5e2), (2e3, 9.9e5), (1.1e-3, 0.9)])
def test_search_finite_interval(psd, a, b):
    """a minimum on a finite [A, B) that round 2 sees, wide or narrow: both ends are found within a
    factor 1 + tol, closed, and .penalty is exp of the midpoint"""
    assert any(a <= x < b for x in LADDER)
    result, _ = replay(psd, step(a, b))
    assert result.min_errors == 0 and result.lower_closed and result.upper_closed
    assert within(result.min_log_lambda, a) and within(result.max_log_lambda, b)
    assert math.log(a) <= result.min_log_lambda <= result.max_log_lambda < math.log(b)
    assert result.penalty == pytest.approx(math.exp(0.5 * (result.min_log_lambda + result.max_log_lambda)))


def test_search_bounds_hold_everywhere(psd):
    """for A, B anywhere in [1e-3, 1e6] the search ends within 20 rounds of at most 8 penalties
    (replay asserts both), and where round 2 sees [A, B) both ends are within a factor 1 + tol"""
    rng = np.random.default_rng(11)
    most = seen = 0
    for _ in range(200):
        a, b = np.sort(np.exp(rng.uniform(math.log(1e-3), math.log(1e6), 2)))
        result, asked = replay(psd, step(a, b))
        most = max(most, len(asked))
        if any(a <= x < b for x in LADDER):
            seen += 1
            assert within(result.min_log_lambda, a) and within(result.max_log_lambda, b), (a, b)
        else:                                     # every evaluated penalty has 2 errors
            assert result.min_errors == 2 and result.penalty == 0.0
    assert most <= ROUNDS and seen >= 100


def test_search_minimum_reaching_zero(psd):
    """errors are fewest from penalty 0 up to B: the lower end is -inf, .penalty = exp(max - 1)"""
    result, _ = replay(psd, lambda x: 1 if x < 55.0 else 4)
    assert result.min_errors == 1 and result.min_log_lambda == -math.inf
    assert result.lower_closed and result.upper_closed and within(result.max_log_lambda, 55.0)
    assert result.penalty == pytest.approx(math.exp(result.max_log_lambda - 1.0))


def test_search_minimum_reaching_the_empty_model(psd):
    """errors are fewest from A on, the empty model included: the upper end is +inf, .penalty =
    exp(min + 1)"""
    result, _ = replay(psd, lambda x: 5 if x < 321.0 else 2)
    assert result.min_errors == 2 and result.max_log_lambda == math.inf
    assert result.lower_closed and result.upper_closed and within(result.min_log_lambda, 321.0)
    assert result.penalty == pytest.approx(math.exp(result.min_log_lambda + 1.0))
    assert (result.models["peaks"] == 0).any()


def test_search_two_runs_of_equal_errors(psd):
    """two runs of the fewest errors: the one wider in log(penalty); of two equally wide ones the
    one of the larger penalties"""
    errors = lambda x: 0 if 1.0 <= x < 4.0 or 100.0 <= x < 3200.0 else 3     # noqa: E731
    result, _ = replay(psd, errors)
    assert within(result.min_log_lambda, 100.0) and within(result.max_log_lambda, 3200.0)
    search = psd.JointSearch(TOL)
    search.next_penalties(WIDTH)
    search.add(0.0, 1, 1, 3, 0, 3)
    search.scale(1.0, 100.0)
    search.asked |= {1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0}
    search.round = 2
    for penalty, e in ((1.0, 0), (2.0, 0), (4.0, 3), (8.0, 0), (16.0, 0), (32.0, 3), (64.0, 3)):
        search.add(penalty, 1, 1, e, 0, e)
    best, first, last = search.chosen()[:3]
    assert (best, first, last) == (0, 4, 5)                        # [8, 16], not [1, 2]


def test_search_run_splits(psd):
    """a function that is not monotone: after the doubling round, round 4 places 1.22, 1.48, 1.81 and 2.20 in the lower
    flank (1, 2.68) of round 2's run; 1.48 has the fewest errors again but 1.81 has more, so the
    run splits there, and the result is the wider part with its own lower end found"""
    def errors(x):
        if 1.7 <= x < 2.0:
            return 7                                           # a spike
        return 1 if 1.4 <= x < 900.0 else 5
    result, asked = replay(psd, errors, gains=(1.0, 1e3), empty=3e3)
    assert [round(x, 2) for x in asked[3][:4]] == [1.22, 1.48, 1.81, 2.2]
    lo, hi = math.exp(result.min_log_lambda), math.exp(result.max_log_lambda)
    assert result.min_errors == 1 and 2.0 <= lo < hi < 900.0
    assert within(result.min_log_lambda, 2.0) and within(result.max_log_lambda, 900.0)
    models = result.models
    inside = models[(models["penalty"] >= lo) & (models["penalty"] <= hi)]
    assert (inside["errors"] == 1).all() and (models["errors"] == 7).any()
    left = models[(models["penalty"] >= 1.4) & (models["penalty"] < 1.7)]
    assert len(left) and (left["errors"] == 1).all()           # the other part of the split run


def test_search_without_labels_and_without_peaks(psd):
    """no labels at all: every model has 0 errors, both ends are infinite and .penalty is 0.0; a
    model without any gain at penalty 0 ends the search after round 1"""
    result, asked = replay(psd, lambda x: 0)
    assert (result.min_log_lambda, result.max_log_lambda) == (-math.inf, math.inf)
    assert result.penalty == 0.0 and result.lower_closed and result.upper_closed
    assert (result.models["peaks"] == 0).any()                 # it went up to an empty model
    result, asked = replay(psd, lambda x: 2, gains=None)
    assert asked == [[0.0]] and result.penalty == 0.0 and result.min_errors == 2


def test_search_small_widths_and_misuse(psd):
    for width in (1, 3, 5):                                    # (their round 2 sees [0.5, 40))
        result, asked = replay(psd, step(0.5, 40.0), width=width, max_rounds=200)
        assert within(result.min_log_lambda, 0.5) and within(result.max_log_lambda, 40.0)
        assert all(len(r) <= width for r in asked)
    search = psd.JointSearch()
    assert search.next_penalties(8) == [0.0]
    with pytest.raises(ValueError, match="not asked for"):
        search.add(1.0, 1, 1, 0, 0, 0)
    with pytest.raises(ValueError, match="were not added"):
        search.next_penalties(8)
    search.add(0.0, 1, 1, 0, 0, 0)
    with pytest.raises(ValueError, match="scale"):
        search.next_penalties(8)
    with pytest.raises(ValueError, match="smallest"):
        search.scale(2.0, 1.0)
    with pytest.raises(ValueError, match="tol"):
        psd.JointSearch(0.0)


# ---- the Python layer and the yardstick ----------------------------------------------------------

def test_entries_check_their_arguments_first(psd):
    v = [np.ones(50, np.int32)] * 2
    good = (np.array([1], np.int32), np.array([9], np.int32), ["peaks"])
    with pytest.raises(ValueError, match="one entry per sample"):
        psd.learn_joint_penalty_dense(v, [good], penalties=1.0)
    with pytest.raises(ValueError, match="not one of"):
        psd.learn_joint_penalty_dense(v, [good, (good[0], good[1], ["peak"])], penalties=1.0)
    with pytest.raises(ValueError, match="tol"):
        psd.learn_joint_penalty_dense(v, [good, None], penalties=1.0, tol=0.0)
    with pytest.raises(ValueError, match="max_rounds"):
        psd.joint_target_interval_dense(v, [good, None], penalties=1.0, max_rounds=1)
    with pytest.raises(ValueError, match="a list of vectors"):
        psd.joint_target_interval_dense(v[0], [good], penalties=1.0)
    with pytest.raises(ValueError, match="a list of samples"):
        psd.learn_joint_penalty_reads([np.ones(3, np.int32)], [good], penalties=1.0)
    with pytest.raises(ValueError):                             # exactly one source of penalties
        psd.learn_joint_penalty_dense(v, [good, None])


def test_yardstick_by_hand():
    """two members, two windows; member 1 is up at the first peak only"""
    joint = pd.DataFrame({"peakStart": np.array([10, 30, -1], np.int32),
                          "peakEnd": np.array([20, 40, -1], np.int32)})
    model = [{"members": np.array([0, 2]), "joint": joint,
              "up": np.array([[1, 1], [1, 0], [0, 0]], np.int32)}]
    labels = [(np.array([5, 5, 20, 10, 15], np.int32), np.array([45, 10, 30, 11, 40], np.int32),
               np.array([PEAKS, NO_PEAKS, NO_PEAKS, PEAK_START, PEAK_END], np.int32)),
              (np.array([0], np.int32), np.array([100], np.int32), np.array([PEAKS], np.int32)),
              (np.array([5, 25, 5], np.int32), np.array([45, 45, 45], np.int32),
               np.array([PEAK_START, PEAKS, NO_PEAKS], np.int32))]
    model_totals, problem_totals, rows = joint_label_errors_ref([model], labels)
    assert rows[0][0][0].tolist() == [2, 0, 0, 1, 2]           # counts of member 0's labels
    assert rows[0][0][1].tolist() == [0, 0, 0, 0, 1] and not rows[0][0][2].any()
    assert rows[0][1][0].tolist() == [0] and rows[0][1][2].tolist() == [1]    # in no group
    assert rows[0][2][0].tolist() == [1, 0, 1] and rows[0][2][1].tolist() == [0, 0, 1]
    assert rows[0][2][2].tolist() == [0, 1, 0]
    assert problem_totals[0].tolist() == [[1, 1, 0, 4, 3], [1, 0, 1, 0, 1], [2, 1, 1, 2, 2]]
    assert model_totals[0].tolist() == [4, 2, 2, 6, 6]
