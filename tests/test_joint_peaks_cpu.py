"""Joint peaks without a device: the Python layer's argument checks (they come before any call of
the library), the yardstick tests/joint_ref.py by hand on three tiny cases whose answers are worked
out in the comments, and its margin assertion firing where two candidates tie."""
import math

import numpy as np
import pytest

import joint_ref
from joint_ref import MarginError, clip_window, cluster_window, joint_peaks_ref


class _Refuses:
    """stands where the library is: any call of it fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the arguments were checked" % name)


def bare_set(n_problems, n_contigs):
    from peaksegdisk_amd.grid import ProblemSet
    pset = ProblemSet.__new__(ProblemSet)
    pset._lib = _Refuses()
    pset._h = None
    pset.device = 0
    pset.problems = [(c % n_contigs, 1.0) for c in range(n_problems)]
    pset._n_contigs = lambda: n_contigs
    return pset


def test_python_layer_checks_its_arguments_first():
    import __graft_entry__ as entry
    entry.build_hip()  # the package refuses to import without its HIP library
    pset = bare_set(3, 3)
    good = (np.array([5], np.int32), np.array([9], np.int32))
    with pytest.raises(ValueError, match="one group per problem"):
        pset.joint_peaks([0, 0], windows=[good])
    with pytest.raises(ValueError, match="integers"):
        pset.joint_peaks([0, 0.5, 0], windows=[good])
    with pytest.raises(ValueError, match="one entry of windows per group"):
        pset.joint_peaks([0, 1, 1], windows=[good])
    with pytest.raises(ValueError, match="not \\(start, end\\)"):
        pset.joint_peaks([0, 0, 0], windows=[(good[0],)])
    with pytest.raises(ValueError, match="1 window starts and 2 ends"):
        pset.joint_peaks([0, 0, 0], windows=[(good[0], np.array([9, 12], np.int32))])
    with pytest.raises(ValueError, match="window end has dtype int64"):
        pset.joint_peaks([0, 0, 0], windows=[(good[0], np.array([9], np.int64))])
    with pytest.raises(ValueError, match="window start is a list"):
        pset.joint_peaks([0, 0, 0], windows=[([5], good[1])])
    with pytest.raises(ValueError, match="one value per contig"):
        pset.joint_peaks([0, 0, 0], windows=[good], first_chromStart=[0, 0])


def test_api_checks_its_arguments_first():
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd as psd
    vectors = [np.full(10, 2, np.int32)] * 2
    for bad in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="joint_penalty"):
            psd.joint_peaks_dense(vectors, penalties=1.0, joint_penalty=bad)
    with pytest.raises(ValueError, match="a list of vectors"):
        psd.joint_peaks_dense(vectors[0], penalties=1.0)
    with pytest.raises(ValueError, match="one per sample"):
        psd.joint_peaks_dense(vectors, penalties=1.0, groups=[0])
    with pytest.raises(ValueError, match="a list of samples"):
        psd.joint_peaks_reads([np.zeros(3, np.int32)], penalties=1.0)
    assert {"joint_peaks_dense", "joint_peaks_reads", "JointPeaks"} <= set(psd.__all__)


def test_yardstick_one_candidate():
    # [1, 9, 1] on the window [0, 3): W = 3, b = 1, the one candidate is (1, 2).
    # S = 1, 9, 1 and L = 1, 1, 1: 9 * 1 > 1 * 1 on both sides, feasible.
    # gain = 1 log 1 + 9 log 9 + 1 log 1 - 11 log(11 / 3) = 9 log 9 - 11 log(11 / 3) = 5.4829...
    ref = joint_peaks_ref([np.array([1, 9, 1])], [0], (0, 3), 0.0)
    want = 9 * math.log(9) - 11 * math.log(11 / 3)
    assert (ref["peakStart"], ref["peakEnd"], ref["levels"], ref["samples_up"]) == (1, 2, 1, 1)
    assert abs(float(ref["objective"]) - want) < 1e-12 and abs(float(ref["gain"][0]) - want) < 1e-12
    assert ref["sum"].tolist() == [9] and ref["bases"].tolist() == [1] and ref["up"].tolist() == [1]
    assert ref["trace"][0]["runner_up"] == -np.inf and 0 < ref["E"] < 1e-12
    # at a penalty above the gain no member is up: no joint peak, and everything is 0
    ref = joint_peaks_ref([np.array([1, 9, 1])], [0], (0, 3), 6.0)
    assert (ref["peakStart"], ref["peakEnd"], ref["levels"], ref["samples_up"]) == (-1, -1, 0, 0)
    assert ref["objective"] == 0 and not ref["gain"].any() and not ref["sum"].any()


def test_yardstick_two_members_one_infeasible():
    # window [10, 14) of two members that begin at 10: A = [0, 6, 6, 0], B = [5, 1, 1, 5].
    # Candidates (s, e): (11, 12), (11, 13), (12, 13).  B dips where A peaks: at (11, 13) B has
    # S2 L1 = 2 * 1 against S1 L2 = 5 * 2: infeasible, and so it is at the other two.  For A:
    #   (11, 13): S = 0, 12, 0, L = 1, 2, 1: gain = 12 log 6 - 12 log 3 = 12 log 2 = 8.3177...
    #   (11, 12): S = 0, 6, 6, L = 1, 1, 2: 6 * 2 > 6 * 1 feasible: 6 log 6 + 6 log 3 - 12 log 3
    #             = 6 log 2 = 4.1588...; (12, 13) is its mirror image, the same gain.
    # The best is (11, 13); the runner-up's G is 6 log 2.
    A, B = np.array([0, 6, 6, 0]), np.array([5, 1, 1, 5])
    ref = joint_peaks_ref([A, B], [10, 10], (10, 14), 0.0)
    assert (ref["peakStart"], ref["peakEnd"], ref["samples_up"]) == (11, 13, 1)
    assert abs(float(ref["objective"]) - 12 * math.log(2)) < 1e-12
    assert abs(float(ref["trace"][0]["runner_up"]) - 6 * math.log(2)) < 1e-12
    assert ref["up"].tolist() == [1, 0] and ref["gain"][1] == 0 and ref["sum"].tolist() == [12, 2]
    assert ref["bases"].tolist() == [2, 2]
    # the penalty is paid per member that is up: G = 12 log 2 - 3
    ref = joint_peaks_ref([A, B], [10, 10], (10, 14), 3.0)
    assert abs(float(ref["objective"]) - (12 * math.log(2) - 3)) < 1e-12 and ref["samples_up"] == 1


def test_yardstick_two_levels_and_clipping():
    # One member of 70 bases that begins at 100: 1 everywhere, 9 on [130, 150).  The window as given,
    # [90, 300), is clipped to the extent [100, 170): W = 70, b = 2 (35 bins), two levels.  130 and
    # 150 are on level 0's boundaries (100 + 2 i), so level 0 finds (130, 150) and level 1 (b = 1,
    # candidates 126 .. 134 x 146 .. 154) keeps it.  S = 30, 180, 20 and L = 30, 20, 20:
    # gain = 30 log 1 + 180 log 9 + 20 log 1 - 230 log(230 / 70).
    v = np.ones(70, np.int64)
    v[30:50] = 9
    ref = joint_peaks_ref([v], [100], (90, 300), 0.0)
    assert (ref["windowStart"], ref["windowEnd"]) == (100, 170)
    assert [(lv["b"], lv["s"], lv["e"]) for lv in ref["trace"]] == [(2, 130, 150), (1, 130, 150)]
    want = 180 * math.log(9) - 230 * math.log(230 / 70)
    assert ref["levels"] == 2 and abs(float(ref["objective"]) - want) < 1e-10
    assert ref["sum"].tolist() == [180] and ref["bases"].tolist() == [20]
    # the helpers: a window wholly outside the extent, no members, and a cluster's window
    assert clip_window([100], [70], (0, 50)) == (100, 100) and clip_window([], [], (0, 50)) == (0, 0)
    assert clip_window([100, 120], [70, 30], (90, 300)) == (120, 150)
    assert cluster_window(130, 150) == (110, 170)
    assert joint_peaks_ref([v], [100], (0, 50), 0.0)["peakStart"] == -1
    assert joint_peaks_ref([], [], (0, 50), 0.0)["levels"] == 0


def test_margin_assertion_fires_on_a_flat_objective():
    # two equal bumps, mirror images of each other: (1, 2) and (4, 5) have the same G to the last
    # bit, the objective is flat between them, and a rounding could decide: not a usable scenario
    with pytest.raises(MarginError, match="runner-up"):
        joint_peaks_ref([np.array([0, 9, 0, 0, 9, 0])], [0], (0, 6), 0.0)
    # ... unless the margins are not asked for (the host path of tools/joint_timing.py)
    ref = joint_peaks_ref([np.array([0, 9, 0, 0, 9, 0])], [0], (0, 6), 0.0, real=np.float64,
                          check_margin=False)
    assert (ref["peakStart"], ref["peakEnd"]) == (1, 2)              # the smallest s among equals
    # a member whose gain sits on the penalty: `up` could go either way
    gain = float(joint_peaks_ref([np.array([1, 9, 1])], [0], (0, 3), 0.0)["gain"][0])
    with pytest.raises(MarginError):
        joint_peaks_ref([np.array([1, 9, 1]), np.array([1, 9, 1])], [0, 0], (0, 3), gain)
    # a constant member is infeasible everywhere by the exact integer test: robustly no joint peak
    ref = joint_peaks_ref([np.full(40, 7)], [0], (0, 40), 0.0)
    assert ref["peakStart"] == -1 and ref["trace"][0]["G"] == 0
    assert joint_ref.BINS == 64
