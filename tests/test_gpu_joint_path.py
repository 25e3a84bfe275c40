"""ProblemSet.joint_path (joint peaks at many penalties in one call), ProblemSet.joint_label_errors
(the label errors of every such model) and learn_joint_penalty_dense.

The scenario functions are shared with the emulator rehearsal (tests/test_joint_path_emu.py).
Yardsticks: every penalty's model must equal ProblemSet.joint_peaks at that penalty bit for bit
(same_bits of tests/test_gpu_joint_peaks.py; that entry is pinned by tests/joint_ref.py, which the
first scenarios also check directly per penalty, its margins asserted on the CPU first); the label
errors must equal tests/joint_path_ref.py, integers compared for equality.  Every call is made
twice: the second gives the same bits.  In every path scenario a window without a peak at a penalty
has none at every larger penalty of the call."""
import ctypes
import os

import numpy as np
import pytest

from joint_path_ref import NO_PEAKS, PEAK_END, PEAK_START, PEAKS, joint_label_errors_ref
from test_gpu_dense import as_cuda, as_numpy
from test_gpu_joint_peaks import (FRAME, bumps, check_group, member_vector, same_bits,
                                  wrap_windows)

GPU = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def psd():
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd
    from peaksegdisk_amd import _native
    assert _native.lib.peakseg_hip_device_count() >= 1, "no HIP device: GPU tests need an MI355X"
    return peaksegdisk_amd


def _lib():
    from peaksegdisk_amd import _native
    return _native.lib


def check_monotone(penalties, models):
    """once a window has no peak at a penalty, it has none at every larger penalty of the call"""
    order = np.argsort(penalties, kind="stable")
    for g in range(len(models[0])):
        gone = np.zeros(len(models[0][g]["joint"]), bool)
        for p in order:
            has = models[p][g]["joint"]["peakStart"].to_numpy() >= 0
            assert not (gone & has).any(), (g, penalties[p])
            gone |= ~has


def path_and_loop(pset, groups, penalties, windows, firsts, wrap):
    """joint_path twice (the same bits), joint_peaks at every penalty (the same bits as the path's
    model), the timer, monotonicity -> the path's models"""
    given = (lambda: None) if windows is None else (lambda: wrap_windows(windows, wrap))
    models = pset.joint_path(groups, penalties, windows=given(), first_chromStart=firsts)
    again = pset.joint_path(groups, penalties, windows=given(), first_chromStart=firsts)
    ms = ctypes.c_float(-1.0)
    assert _lib().peakseg_hip_joint_path_last_ms(ctypes.byref(ms)) == 0 and ms.value >= 0.0
    assert len(models) == len(penalties)
    for p, penalty in enumerate(penalties):
        same_bits(models[p], again[p])
        single = pset.joint_peaks(groups, penalty=penalty, windows=given(), first_chromStart=firsts)
        assert len(single) == len(models[p])
        same_bits(models[p], single)
        for a, b in zip(models[p], single):
            assert a["members"].tolist() == b["members"].tolist()
            assert list(a["joint"].columns) == FRAME
    check_monotone(penalties, models)
    return models


def run_path(psd, wrap, vectors, firsts, groups, windows, penalties, what="", ref=True):
    """a set of one problem per vector (never solved), path_and_loop on it and, with ref, every
    penalty's groups against joint_ref.joint_peaks_ref (which asserts its margins first)"""
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors],
                                     [(c, INF) for c in range(len(vectors))])
    try:
        models = path_and_loop(pset, groups, penalties, windows, firsts, wrap)
    finally:
        pset.close()
    if ref:
        for g in range(len(windows)):     # (a group at all its penalties: the yardstick keeps what
            members = [q for q in range(len(groups)) if groups[q] == g]    # they have in common)
            for p, penalty in enumerate(penalties):
                check_group(models[p][g], [vectors[q] for q in members], [firsts[q] for q in members],
                            windows[g], penalty, "%s penalty %g group %d" % (what, penalty, g))
    return models


def moving_peak():
    """four members of 400 bases, base 2: member 0 a bump [64, 96) of height 9, members 1-3 bumps
    [256, 288) of heights 5, 6, 7"""
    return [bumps(400, 0, [(64, 96, 9)])] + [bumps(400, 0, [(256, 288, h)]) for h in (5, 6, 7)]


MOVING_PENALTIES = [46.0, 0.0, 1e4, 150.0, 1.5, INF, 60.0, 100.0, 170.0, 46.0]
MOVING_PEAKS = {0.0: (256, 288, 3), 1.5: (256, 288, 3), 46.0: (64, 96, 1), 60.0: (64, 96, 1),
                100.0: (64, 96, 1), 150.0: (64, 96, 1), 170.0: (64, 96, 1), 1e4: (-1, -1, 0),
                INF: (-1, -1, 0)}


# ---- the path scenarios ------------------------------------------------------------------------

def scenario_moving_peak(psd, wrap):
    """the peak moves with the penalty: siblings on different level-0 choices, siblings that idle
    while others refine; the penalties unsorted, one of them twice, 0 and +Inf among them"""
    models = run_path(psd, wrap, moving_peak(), [0] * 4, [0] * 4, [[(0, 400)]], MOVING_PENALTIES,
                      "moving peak")
    for penalty, model in zip(MOVING_PENALTIES, models):
        row = model[0]["joint"].iloc[0]
        assert (row["peakStart"], row["peakEnd"], row["samples_up"]) == MOVING_PEAKS[penalty], penalty
    assert models[0][0]["up"][0].tolist() == [1, 0, 0, 0] and models[1][0]["up"][0].tolist() == [0, 1, 1, 1]
    assert models[0][0]["joint"]["levels"].tolist() == [4] and models[5][0]["joint"]["levels"].tolist() == [0]


def scenario_n_penalties(psd, wrap):
    """1, 2 and the maximum number of penalties; the maximum + 1, 0, and a negative or NaN penalty
    at a non-zero index are refused with status 22 and the index in the text"""
    most = _lib().peakseg_hip_joint_path_max_penalties()
    assert most >= 16
    vectors, windows = moving_peak(), [[(0, 400)]]
    ladder = [0.0, 1.5] + [40.0 + 10.0 * k for k in range(most - 4)] + [1e4, INF]
    assert len(ladder) == most
    for penalties in ([60.0], [1.5, 100.0], ladder):
        run_path(psd, wrap, vectors, [0] * 4, [0] * 4, windows, penalties, "n_penalties")
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors], [(c, INF) for c in range(4)])
    try:
        for penalties, text in (([1.0] * (most + 1), "%d penalties" % (most + 1)), ([], "0 penalties"),
                                ([0.0, 1.0, -2.0], "penalty 2"), ([0.0, float("nan")], "penalty 1")):
            with pytest.raises(RuntimeError, match=text) as ei:
                pset.joint_path([0] * 4, penalties, windows=wrap_windows(windows, wrap))
            assert ei.value.status == 22
            assert _lib().peakseg_hip_problem_set_packed_joint_path_download(
                pset._h, *[None] * 11) == -1
        # what pack_joint_peaks refuses is refused in the same way
        with pytest.raises(RuntimeError, match="group 0: window 1") as ei:
            pset.joint_path([0] * 4, [1.0], windows=wrap_windows([[(0, 400), (9, 9)]], wrap))
        assert ei.value.status == 22
        with pytest.raises(RuntimeError) as ei:                       # no windows: needs a solve
            pset.joint_path([0] * 4, [1.0])
        assert ei.value.status == 13
        with pytest.raises(ValueError, match="one group per problem"):
            pset.joint_path([0], [1.0], windows=[None])
        models = pset.joint_path([0] * 4, [60.0], windows=wrap_windows(windows, wrap))
        assert models[0][0]["joint"]["peakStart"].tolist() == [64]     # the set still answers
    finally:
        pset.close()
    # tables that do not fit: the same set and call again, allowed 8 bytes less than everything it
    # held after its tables were there: status 14, said before anything is allocated
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors], [(c, INF) for c in range(4)])
    try:
        pset.joint_path([0] * 4, [60.0], windows=wrap_windows(windows, wrap))
        room = pset.hbm_bytes
    finally:
        pset.close()
    os.environ["PEAKSEG_HIP_MAX_BYTES"] = str(room - 8)
    try:
        capped = psd.ProblemSet.from_dense([wrap(v) for v in vectors], [(c, INF) for c in range(4)])
    finally:
        del os.environ["PEAKSEG_HIP_MAX_BYTES"]
    try:
        before = capped.hbm_bytes
        with pytest.raises(RuntimeError, match="do not fit") as ei:
            capped.joint_path([0] * 4, [60.0], windows=wrap_windows(windows, wrap))
        assert ei.value.status == 14 and capped.hbm_bytes == before
    finally:
        capped.close()


def member_groups(kinds_of_groups):
    """a group per entry (size, {member: kind}): member_vector(k, kind), "peak" where none is
    given -> (vectors, groups); the contigs start at 1000"""
    vectors, groups = [], []
    for g, (size, kinds) in enumerate(kinds_of_groups):
        for k in range(size):
            vectors.append(member_vector(k, kinds.get(k, "peak")))
            groups.append(g)
    return vectors, groups


MEMBER_SIZES = [1, 64, 65, 130]


def members_set():
    """the 260 problems of scenario_members: in the group of 65 an all-zero member, an infeasible
    one and a weak one"""
    return member_groups([(size, {3: "zero", 40: "dip", 64: "weak"} if size == 65 else {})
                          for size in MEMBER_SIZES])


def scenario_members(psd, wrap):
    """groups of 1, 64, 65 and 130 members with three penalties each: the accumulators of several
    penalties across the boundaries of the slabs of 64 members (and of the smaller slabs of the
    later levels); in the group of 65 an all-zero member, an infeasible one and a weak one"""
    sizes = MEMBER_SIZES
    vectors, groups = members_set()
    firsts = [1000] * len(vectors)
    windows = [[(1020, 1180)]] * len(sizes)
    models = run_path(psd, wrap, vectors, firsts, groups, windows, [25.0, 1e9, 0.0], "members")
    for g, size in enumerate(sizes):
        row = models[0][g]["joint"].iloc[0]
        assert (row["peakStart"], row["peakEnd"], row["levels"]) == (1070, 1110, 3), g
        assert row["samples_up"] == (size - 3 if size == 65 else size)
        assert models[1][g]["joint"]["peakStart"].tolist() == [-1]
        assert models[2][g]["joint"]["samples_up"].tolist() == [size - 2 if size == 65 else size]
    assert models[0][2]["up"][0, [3, 40, 64]].tolist() == [0, 0, 0]
    assert models[2][2]["up"][0, [3, 40, 64]].tolist() == [0, 0, 1]


def scenario_widths(psd, wrap):
    """W = 2, 3, 64, 65 and 129 in one call with four penalties: windows finish at different
    levels; and a window of 2^15 + 1 bases, eleven levels, its peak on odd coordinates"""
    spans = [(150, 170, 50), (300, 301, 90), (420, 470, 60)]
    vectors = [bumps(600, 0, spans), bumps(600, 0, [(a, b, h - 9) for a, b, h in spans], base=3)]
    vectors += [bumps(33000, 0, [(10001, 20003, 40 + 5 * k)], base=3 + k) for k in range(2)]
    windows = [[(140, 142), (299, 302), (128, 192), (128, 193), (400, 529)], [(100, 100 + 2 ** 15 + 1)]]
    penalties = [30.0, 0.0, 1e9, 5.0]
    models = run_path(psd, wrap, vectors, [0] * 4, [0, 0, 1, 1], windows, penalties, "widths")
    for p in (0, 1, 3):
        assert models[p][0]["joint"]["levels"].tolist() == [0, 1, 1, 2, 3]
        assert models[p][0]["joint"]["peakStart"].tolist() == [-1, 300, 150, 150, 420]
        assert models[p][1]["joint"]["levels"].tolist() == [11]
        row = models[p][1]["joint"].iloc[0]
        assert (row["peakStart"], row["peakEnd"]) == (10001, 20003)
    assert models[2][1]["joint"]["levels"].tolist() == [0]


def scenario_groups(psd, wrap):
    """several groups, one without members, one without windows, a problem in no group, members
    with different first_chromStart, windows clipped to the members' common extent"""
    spans = [(1150, 1200, 50), (1530, 1570, 70), (1593, 1596, 90)]
    vectors = [bumps(600, 1000, spans), bumps(700, 1100, spans, base=3),
               bumps(400, 0, [(150, 170, 30)]),
               bumps(400, 0, [(150, 170, 50)], base=3), bumps(400, 0, [(150, 170, 44)], base=4)]
    firsts = [1000, 1100, 0, 0, 0]
    groups = [0, 0, -1, 3, 3]
    windows = [[(900, 1300), (1500, 2000), (100, 200), (1590, 1700), (1598, 2000)],
               [(100, 228)], [], [(120, 200), (140, 180)]]
    models = run_path(psd, wrap, vectors, firsts, groups, windows, [0.0, 40.0, 1e9], "groups")
    for model in models[:2]:
        frame = model[0]["joint"]
        assert frame["windowStart"].tolist() == [1100, 1500, 1100, 1590, 1598]
        assert frame["windowEnd"].tolist() == [1300, 1600, 1100, 1600, 1600]
        assert frame["peakStart"].tolist() == [1150, 1530, -1, 1593, -1]
        assert model[1]["joint"]["peakStart"].tolist() == [-1] and model[1]["gain"].shape == (1, 0)
        assert len(model[2]["joint"]) == 0 and model[2]["gain"].shape == (0, 0)
        assert model[3]["joint"]["peakStart"].tolist() == [150, 150]
        assert model[3]["members"].tolist() == [3, 4]
    pset = psd.ProblemSet.from_dense([wrap(vectors[0])], [(0, 1.0)])
    try:
        assert pset.joint_path([-1], [0.0, 1.0], windows=[]) == [[], []]
    finally:
        pset.close()


def scenario_solved(psd, wrap):
    """windows=None on the solved set of the cluster tests: the clusters' windows at three
    penalties, each equal to joint_peaks (which tests/test_gpu_joint_peaks.py pins there)"""
    from test_gpu_peak_clusters import GROUPS, PROBLEMS, SAMPLES, steps
    firsts = [s[0] for s in SAMPLES]
    vectors = [steps(length, first, spans) for first, length, spans in SAMPLES]
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors], PROBLEMS)
    try:
        pset.solve()
        models = path_and_loop(pset, GROUPS, [5.0, 0.0, 1e9], None, firsts, wrap)
    finally:
        pset.close()
    assert any((entry["joint"]["peakStart"] >= 0).any() for entry in models[0])
    assert not any((entry["joint"]["peakStart"] >= 0).any() for entry in models[2])


def download_path(pset, n_pen, windows, entries):
    dtypes = (np.int32,) * 4 + (np.float64, np.int32, np.int32, np.float64, np.int32, np.int64, np.int32)
    cols = [np.zeros(n_pen * n, dt) for n, dt in zip((windows,) * 7 + (entries,) * 4, dtypes)]
    assert _lib().peakseg_hip_problem_set_packed_joint_path_download(
        pset._h, *[a.ctypes.data for a in cols]) == 0
    return [a.tobytes() for a in cols]


def download_peaks(pset, windows, entries):
    dtypes = (np.int32,) * 4 + (np.float64, np.int32, np.int32, np.float64, np.int32, np.int64, np.int32)
    cols = [np.zeros(n, dt) for n, dt in zip((windows,) * 7 + (entries,) * 4, dtypes)]
    assert _lib().peakseg_hip_problem_set_packed_joint_peaks_download(
        pset._h, *[a.ctypes.data for a in cols]) == 0
    return [a.tobytes() for a in cols]


def scenario_independence(psd, wrap):
    """the two calls keep their own buffers: what joint_path packed is still there, bit for bit,
    after a joint_peaks of other windows and another penalty, and the other way round"""
    vectors = moving_peak()
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors], [(c, INF) for c in range(4)])
    try:
        one = wrap_windows([[(0, 400)]], wrap)
        other = wrap_windows([[(200, 400), (0, 128), (40, 300)]], wrap)
        pset.joint_path([0] * 4, [0.0, 60.0, 1e4], windows=one)
        packed = download_path(pset, 3, 1, 4)
        single = pset.joint_peaks([0] * 4, penalty=1.5, windows=other)
        assert download_path(pset, 3, 1, 4) == packed
        kept = download_peaks(pset, 3, 12)
        pset.joint_path([0] * 4, [100.0, 0.0], windows=one)
        assert download_peaks(pset, 3, 12) == kept
        same_bits(single, pset.joint_peaks([0] * 4, penalty=1.5, windows=other))
        assert np.frombuffer(packed[2], np.int32).tolist() == [256, 64, -1]
    finally:
        pset.close()


SLAB = 64                                             # members of a level-0 slab, of any instance
LATER_SLAB = {1: 64, 2: 64, 4: 57, 8: 28, 16: 14}     # members of a later level's slab, by instance
# 16 penalties, every prefix of which is a call: some members do not reach 25, no window has a
# peak at 1e9 (it idles between penalties that refine), 0, and values every strong member exceeds
LADDER = [25.0, 1e9, 0.0] + [30.0 + 7.0 * k for k in range(13)]


def instance_of(n_pen):
    """the accumulators the kernels are compiled for: the next power of two"""
    width = 1
    while width < n_pen:
        width *= 2
    return width


def widths_case(n_pen):
    """the groups of scenario_penalty_widths_past_slabs for a call of n_pen penalties ->
    [(size, {member: kind})]"""
    later = LATER_SLAB[instance_of(n_pen)]
    # on a later level's slab line, one past it (the zero member the last of the first slab, the
    # weak one the first of the second), and one past level 0's (for 1 and 2 penalties the same)
    cases = [(later, {}), (later + 1, {1: "dip", later - 1: "zero", later: "weak"})]
    if later + 1 != SLAB + 1:
        cases.append((SLAB + 1, {3: "dip", SLAB - 1: "zero", SLAB: "weak"}))
    if n_pen in (8, 16):
        cases.append((2 * SLAB + 1, {SLAB - 1: "zero", SLAB: "dip", 2 * SLAB: "weak"}))
    return cases


def scenario_penalty_widths_past_slabs(psd, wrap):
    """every instance of search0_kernel and refine_kernel (1, 2, 4, 8 and 16 accumulators), once
    with as many penalties as accumulators and once with padded ones, on groups on and one past
    the slab line of the later levels (64, 64, 57, 28 and 14 members), one past level 0's (65: the
    carry in HBM) and, for 8 and 16 penalties, of three level-0 slabs (129); two windows per group
    (W = 160 and 120: three levels and two), so the carry of a window is not the group's"""
    windows = [(1020, 1180), (1030, 1150)]
    seen = set()
    for n_pen in (1, 2, 3, 4, 5, 8, 9, 16):
        width, cases = instance_of(n_pen), widths_case(n_pen)
        later = LATER_SLAB[width]
        sizes = [size for size, _ in cases]
        assert width >= n_pen > width // 2 and later in sizes and later + 1 in sizes
        assert SLAB + 1 in sizes and all(size > 2 * SLAB for size in sizes[3:])
        if n_pen in (8, 16):
            assert -(-sizes[3] // SLAB) == 3 and -(-sizes[3] // later) == {8: 5, 16: 10}[n_pen]
        seen.add((width, n_pen == width))
        penalties = LADDER[:n_pen]
        vectors, groups = member_groups(cases)
        models = run_path(psd, wrap, vectors, [1000] * len(vectors), groups,
                          [windows] * len(cases), penalties, "%d penalties" % n_pen)
        for penalty, model in zip(penalties, models):
            for (size, kinds), entry in zip(cases, model):
                frame = entry["joint"]
                if penalty == 1e9:
                    assert frame["peakStart"].tolist() == [-1, -1] and not entry["up"].any()
                    assert frame["levels"].tolist() == [0, 0]
                    continue
                assert frame["peakStart"].tolist() == [1070, 1070], (n_pen, penalty, size)
                assert frame["peakEnd"].tolist() == [1110, 1110] and frame["levels"].tolist() == [3, 2]
                want = np.ones(size, np.int32)
                for k, kind in kinds.items():
                    want[k] = kind == "weak" and penalty == 0.0
                assert entry["up"].tolist() == [want.tolist()] * 2, (n_pen, penalty, size)
    assert seen == {(w, full) for w in LATER_SLAB for full in (True, False)} - {(1, False), (2, False)}


MANY_STRONG = {0: 9, 35: 10, 69: 11}                  # member: the height of its bump [64, 96)
MANY_PENALTIES = [100.0, 0.0, 1e4, 150.0, 1.5, INF, 60.0, 200.0, 46.0, 80.0, 20.0, 120.0, 240.0,
                  175.0, 300.0, 110.0]


def scenario_moving_peak_many_members(psd, wrap):
    """the moving peak in a group of 70 members at 16 penalties: three strong members with a bump
    [64, 96), one of them in the second level-0 slab, and 67 weak ones with a bump [256, 288).  The
    small penalties end on the weak members' peak, those that no weak member reaches on the strong
    ones', the largest on none: the rows of the penalties differ within every slab, at level 0
    through the carry and at the later levels (five slabs of 14 members)"""
    size = 70
    vectors = [bumps(400, 0, [(64, 96, MANY_STRONG[k])]) if k in MANY_STRONG else
               bumps(400, 0, [(256, 288, 5 + k % 3)]) for k in range(size)]
    assert size > SLAB and max(MANY_STRONG) >= SLAB > min(MANY_STRONG)
    assert len(MANY_PENALTIES) == 16 == _lib().peakseg_hip_joint_path_max_penalties()
    assert -(-size // LATER_SLAB[16]) == 5
    models = run_path(psd, wrap, vectors, [0] * size, [0] * size, [[(0, 400)]], MANY_PENALTIES,
                      "moving peak, many members")
    ends = {}
    for penalty, model in zip(MANY_PENALTIES, models):
        row = model[0]["joint"].iloc[0]
        ends[penalty] = (int(row["peakStart"]), int(row["peakEnd"]), int(row["samples_up"]))
    assert len({e[:2] for e in ends.values() if e[0] >= 0}) >= 2      # two penalties, two peaks
    assert any(e[0] < 0 for e in ends.values())                        # and one without
    weak = size - len(MANY_STRONG)
    assert ends[0.0] == ends[1.5] == ends[20.0] == (256, 288, weak)
    assert ends[60.0][:2] == ends[80.0][:2] == (256, 288) and weak > ends[60.0][2] > ends[80.0][2] > 0
    assert ends[100.0] == ends[110.0] == ends[150.0] == ends[175.0] == (64, 96, 3)
    assert ends[200.0] == (64, 96, 2) and ends[240.0] == (64, 96, 1)
    assert ends[300.0] == ends[1e4] == ends[INF] == (-1, -1, 0)
    up = models[MANY_PENALTIES.index(200.0)][0]["up"][0]
    assert np.flatnonzero(up).tolist() == [35, 69]


def scenario_many_windows(psd, wrap):
    """the 300 windows in two groups of tests/test_gpu_joint_peaks.py at 3 penalties: setup_kernel
    has a thread per (penalty, window), 900 rows in four workgroups, the groups' boundary inside a
    workgroup of every penalty; then 16 penalties on the first 20 windows, 320 rows"""
    from test_gpu_joint_peaks import many_windows_case
    vectors, firsts, groups, windows, peaks = many_windows_case()
    threads, n = 256, len(windows[0]) + len(windows[1])
    penalties = [20.0, 1e9, 0.0]
    assert n == 300 and len(penalties) * n > 3 * threads
    for p in range(len(penalties)):       # the first row of the second group is no workgroup's first
        assert (p * n + len(windows[0])) % threads != 0
    models = run_path(psd, wrap, vectors, firsts, groups, windows, penalties, "many windows")
    for p in (0, 2):
        found = [(int(a), int(b)) for entry in models[p]
                 for a, b in zip(entry["joint"]["peakStart"], entry["joint"]["peakEnd"])]
        assert found == peaks
    assert not any((entry["joint"]["peakStart"] >= 0).any() for entry in models[1])
    every = windows[0] + windows[1]
    few = [every[:13], every[13:20]]
    assert threads < len(LADDER) * 20 < 2 * threads
    models = run_path(psd, wrap, vectors, firsts, groups, few, LADDER, "many windows, 16 penalties")
    for penalty, model in zip(LADDER, models):
        found = [(int(a), int(b)) for entry in model
                 for a, b in zip(entry["joint"]["peakStart"], entry["joint"]["peakEnd"])]
        assert found == (peaks[:20] if penalty < 1e9 else [(-1, -1)] * 20), penalty


# ---- the label-error scenarios -----------------------------------------------------------------

def label_entry(rows):
    """[(start, end, code)] -> what joint_label_errors takes; [] -> None"""
    if not rows:
        return None
    return tuple(np.array([r[j] for r in rows], np.int32) for j in range(3))


def check_labels(pset, models, labels, wrap):
    """joint_label_errors twice (the same bits) against the yardstick -> (model, problem, rows)"""
    given = [None if e is None else tuple(wrap(a) for a in e) for e in labels]
    got = pset.joint_label_errors(given)
    again = pset.joint_label_errors(given)
    ms = ctypes.c_float(-1.0)
    assert _lib().peakseg_hip_joint_label_errors_last_ms(ctypes.byref(ms)) == 0 and ms.value >= 0.0
    want = joint_label_errors_ref(models, labels)
    for result in (got, again):
        assert result[0].dtype == np.int64 and result[1].dtype == np.int32
        assert np.array_equal(result[0], want[0]), (result[0], want[0])
        assert np.array_equal(result[1], want[1])
        for p in range(len(models)):
            for q in range(len(labels)):
                for a, b in zip(result[2][p][q], want[2][p][q]):
                    assert a.dtype == np.int32 and np.array_equal(a, b), (p, q, a, b)
    return got


def scenario_label_relations(psd, wrap):
    """every annotation at counts 0, 1 and 2; the boundaries of the three relations; two windows
    whose peaks coincide; a problem in no group; a problem without labels; labels far outside every
    window"""
    spans = [(150, 170, 50), (420, 470, 60)]
    vectors = [bumps(600, 0, spans), bumps(600, 0, [(a, b, h - 9) for a, b, h in spans], base=3),
               bumps(600, 0, spans, base=4), bumps(600, 0, spans, base=5)]
    groups = [0, 0, -1, 1]
    windows = [[(100, 229), (380, 600)], [(100, 229), (120, 200)]]
    every = [(region + (a,)) for a in range(4) for region in ((200, 300), (140, 200), (100, 500))]
    edges = [(100, 150, NO_PEAKS), (170, 200, PEAKS), (150, 160, PEAK_START), (160, 170, PEAK_END),
             (151, 200, PEAK_START), (100, 169, PEAK_END), (149, 151, NO_PEAKS), (169, 171, PEAKS)]
    far = [(2000000000, 2000000100, a) for a in range(4)] + [(-2000000000, -5, PEAKS)]
    labels = [label_entry(every + edges), None, label_entry(every), label_entry(
        [(140, 160, PEAK_START), (160, 180, PEAK_END), (100, 200, NO_PEAKS), (100, 200, PEAKS)] + far)]
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors], [(c, INF) for c in range(4)])
    try:
        models = pset.joint_path(groups, [0.0, 1e9], windows=wrap_windows(windows, wrap))
        model, problem, rows = check_labels(pset, models, labels, wrap)
    finally:
        pset.close()
    assert models[0][0]["joint"]["peakStart"].tolist() == [150, 420]
    assert models[0][1]["joint"]["peakStart"].tolist() == [150, 150]
    count, fp, fn = rows[0][0]
    assert count[:12].tolist() == [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2]
    assert fp[:12].tolist() == [0, 1, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0]
    assert fn[:12].tolist() == [0, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0]
    assert count[12:].tolist() == [0, 0, 1, 1, 0, 0, 1, 1]
    assert not rows[0][2][0].any() and rows[0][2][2].tolist() == [0, 0, 0] + [1] * 9  # in no group
    count, fp, fn = rows[0][3]                                     # two coinciding peaks
    assert count[:4].tolist() == [2, 2, 2, 2] and fp[:4].tolist() == [1, 1, 1, 0]
    assert not count[4:].any() and fn[4:].tolist() == [0, 1, 1, 1, 1]
    assert problem[0, 1].tolist() == [0] * 5
    assert model[1, 0] == model[1, 2] == model[1, 4] > 0 and model[1, 1] == 0   # the empty model


def scenario_label_models(psd, wrap):
    """the moving peak with a `peaks` label on [250, 300) for members 1-3 and a `noPeaks` label
    there for member 0: the penalties' errors differ, and a member that is not up sees no peak
    where its neighbour does"""
    labels = [label_entry([(250, 300, NO_PEAKS), (50, 100, PEAK_START)])] + \
             [label_entry([(250, 300, PEAKS), (50, 100, NO_PEAKS)])] * 3
    pset = psd.ProblemSet.from_dense([wrap(v) for v in moving_peak()], [(c, INF) for c in range(4)])
    try:
        models = pset.joint_path([0] * 4, MOVING_PENALTIES, windows=wrap_windows([[(0, 400)]], wrap))
        model, problem, rows = check_labels(pset, models, labels, wrap)
    finally:
        pset.close()
    errors = dict(zip(MOVING_PENALTIES, model[:, 0].tolist()))
    assert errors == {0.0: 1, 1.5: 1, 46.0: 3, 60.0: 3, 100.0: 3, 150.0: 3, 170.0: 3, 1e4: 4, INF: 4}
    at_46 = rows[0]
    assert at_46[0][0].tolist() == [0, 1] and at_46[1][0].tolist() == [0, 0]   # member 1 is not up
    assert model[:, 3].tolist() == [5] * 10 and model[:, 4].tolist() == [4] * 10


def scenario_label_strides(psd, wrap):
    """257 labels on one problem and 65 windows in one group: past one workgroup of labels and one
    wave of windows"""
    rng = np.random.default_rng(5)
    spans = [(40 * k + 10, 40 * k + 20 + k % 7, 30 + k % 5) for k in range(65)]
    vectors = [bumps(2600, 0, spans), bumps(2600, 0, [(a, b, h + 7) for a, b, h in spans], base=3)]
    windows = [[(40 * k, 40 * k + 40) for k in range(65)]]
    start = rng.integers(0, 2500, 257)
    rows = [(int(a), int(a + w), int(c)) for a, w, c in zip(start, rng.integers(1, 200, 257),
                                                            rng.integers(0, 4, 257))]
    labels = [label_entry(rows), label_entry(rows[:3])]
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors], [(c, INF) for c in range(2)])
    try:
        models = pset.joint_path([0, 0], [0.0, 1e9, 20.0], windows=wrap_windows(windows, wrap))
        model, _, _ = check_labels(pset, models, labels, wrap)
    finally:
        pset.close()
    assert (models[0][0]["joint"]["peakStart"] >= 0).sum() == 65
    assert model[0, 1] > 0 and model[1, 1] == 0 and model[1, 2] == model[1, 4]


def scenario_label_many_problems(psd, wrap):
    """the 260 problems of scenario_members after a path of the maximum number of penalties:
    sum_kernel's threads take a second problem each past 256; one to three labels on a problem,
    none on a few; the problems past 256 have labels that count"""
    vectors, groups = members_set()
    n_problems, threads = len(vectors), 256
    kinds = [[(1060, 1080, PEAK_START)],
             [(1000, 1200, NO_PEAKS), (1100, 1120, PEAK_END)],
             [(1050, 1120, PEAKS), (1120, 1190, NO_PEAKS), (1075, 1100, PEAK_START)]]
    labels = [None if q % 37 == 5 else label_entry(kinds[q % 3]) for q in range(n_problems)]
    assert threads < n_problems < 2 * threads
    assert all(labels[q] is not None for q in range(threads, n_problems))
    assert sum(e is None for e in labels) >= 3
    assert {len(e[0]) for e in labels if e is not None} == {1, 2, 3}
    assert len(LADDER) == _lib().peakseg_hip_joint_path_max_penalties()
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors], [(c, INF) for c in range(n_problems)])
    try:
        windows = wrap_windows([[(1020, 1180)]] * len(MEMBER_SIZES), wrap)
        models = pset.joint_path(groups, LADDER, windows=windows, first_chromStart=[1000] * n_problems)
        model, problem, _ = check_labels(pset, models, labels, wrap)
    finally:
        pset.close()
    for p, penalty in enumerate(LADDER):
        for g in range(len(MEMBER_SIZES)):
            assert models[p][g]["joint"]["peakStart"].tolist() == [1070 if penalty < 1e9 else -1]
    # every total of the problems past 256 differs between a model with peaks and the one without
    full, empty = LADDER.index(25.0), LADDER.index(1e9)
    assert problem[full, threads:, 0].tolist() != problem[empty, threads:, 0].tolist()
    assert problem[:, threads:, 3:].all() and problem[empty, threads:, 0].all()
    assert model[empty, 0] > model[full, 0] > 0 and len({tuple(row) for row in model.tolist()}) >= 3


def scenario_label_full_waves(psd, wrap):
    """count_kernel packs a wave's four sums into the bytes of one word: 192 `peakStart` labels on
    one problem, three whole waves of every penalty, around the start of two windows' coinciding
    peaks: all false positives at penalty 0, all false negatives where there is no peak, so the
    bytes of both kinds and of both possible kinds hold 64; the same labels shuffled on a second
    problem"""
    spans = [(150, 170, 50), (420, 470, 60)]
    vectors = [bumps(600, 0, spans), bumps(600, 0, [(a, b, h - 9) for a, b, h in spans], base=3)]
    windows = [[(100, 229), (120, 200)]]
    ordered = [(150 - j % 48, 151 + j // 48 + j % 5, PEAK_START) for j in range(192)]
    order = np.random.default_rng(15).permutation(len(ordered))
    labels = [label_entry(ordered), label_entry([ordered[j] for j in order])]
    penalties = [0.0, 1e9]
    wave, n_labels = 64, sum(len(e[0]) for e in labels)
    assert len(set(ordered)) == len(ordered) == 3 * wave and order.tolist() != sorted(order.tolist())
    for p in range(len(penalties)):                 # the rows are penalty-major: p * n_labels + row
        assert (p * n_labels) % wave == 0 and (p * n_labels + len(ordered)) % wave == 0
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors], [(c, INF) for c in range(2)])
    try:
        models = pset.joint_path([0, 0], penalties, windows=wrap_windows(windows, wrap))
        model, problem, rows = check_labels(pset, models, labels, wrap)
    finally:
        pset.close()
    assert models[0][0]["joint"]["peakStart"].tolist() == [150, 150] and models[0][0]["up"].all()
    assert models[1][0]["joint"]["peakStart"].tolist() == [-1, -1]
    for q in range(2):                               # (what the yardstick gave, checked above)
        count, fp, fn = rows[0][q]
        assert count.tolist() == [2] * 192 and fp.all() and not fn.any()
        count, fp, fn = rows[1][q]
        assert not count.any() and not fp.any() and fn.all()
    assert problem[0].tolist() == [[192, 192, 0, 192, 192]] * 2
    assert problem[1].tolist() == [[192, 0, 192, 192, 192]] * 2
    assert model.tolist() == [[384, 384, 0, 384, 384], [384, 0, 384, 384, 384]]


def scenario_label_refusals(psd, wrap):
    vectors = moving_peak()
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors], [(c, INF) for c in range(4)])
    try:
        good = label_entry([(250, 300, PEAKS)])
        with pytest.raises(RuntimeError) as ei:                      # no path is packed
            pset.joint_label_errors([good] * 4)
        assert ei.value.status == 13
        assert _lib().peakseg_hip_problem_set_packed_joint_label_errors_download(
            pset._h, *[None] * 5) == -1
        pset.joint_path([0] * 4, [0.0, 60.0], windows=wrap_windows([[(0, 400)]], wrap))
        for bad, text in ((label_entry([(250, 300, PEAKS), (300, 300, PEAKS)]), "problem 2: label 1"),
                          (label_entry([(250, 300, 4)]), "annotation code 4")):
            with pytest.raises(RuntimeError, match=text) as ei:
                pset.joint_label_errors([good, None, bad, good])
            assert ei.value.status == 19
            assert _lib().peakseg_hip_problem_set_packed_joint_label_errors_download(
                pset._h, *[None] * 5) == -1
        with pytest.raises(ValueError, match="one entry per problem"):
            pset.joint_label_errors([good])
        with pytest.raises(ValueError, match="not one of"):
            pset.joint_label_errors([(good[0], good[1], ["peak"])] + [None] * 3)
        model, _, _ = pset.joint_label_errors([(good[0], good[1], ["peaks"])] + [None] * 3)
        assert model[:, 0].tolist() == [1, 1]                        # the set still answers
    finally:
        pset.close()


def scenario_learn(psd, wrap):
    """learn_joint_penalty_dense on the moving-peak samples: the interval holds none of the
    evaluated penalties with more errors, and joint_peaks_dense at .penalty has min_errors errors
    by the yardstick"""
    vectors = moving_peak()
    labels = [label_entry([(250, 300, NO_PEAKS)])] + [label_entry([(250, 300, PEAKS)])] * 3
    result = psd.learn_joint_penalty_dense([wrap(v) for v in vectors], labels, penalties=10.0)
    frame = result.models
    assert list(frame.columns) == ["penalty", "peaks", "samples_up", "errors", "fp", "fn", "round"]
    assert result.min_errors == frame["errors"].min() == 0 and 2 <= result.rounds <= 20
    assert frame["penalty"].is_unique and (frame.groupby("round").size() <= 8).all()
    worse = frame[frame["errors"] > result.min_errors]["penalty"]
    assert len(worse) and (worse > 0).all()
    inside = (np.log(worse) >= result.min_log_lambda) & (np.log(worse) <= result.max_log_lambda)
    assert not inside.any()
    assert result.min_log_lambda == -INF and result.lower_closed and result.upper_closed
    assert result.penalty == pytest.approx(np.exp(result.max_log_lambda - 1.0))
    out = psd.joint_peaks_dense([wrap(v) for v in vectors], penalties=10.0,
                                joint_penalty=result.penalty)
    model = [{"members": out.groups[0]["samples"], "joint": out.groups[0]["joint"],
              "up": out.groups[0]["up"]}]
    assert joint_label_errors_ref([model], labels)[0][0, 0] == result.min_errors
    assert (out.joint["peakStart"] >= 0).sum() == 2


PATH_SCENARIOS = [scenario_moving_peak, scenario_n_penalties, scenario_members, scenario_widths,
                  scenario_groups, scenario_solved, scenario_independence,
                  scenario_penalty_widths_past_slabs, scenario_moving_peak_many_members,
                  scenario_many_windows]
LABEL_SCENARIOS = [scenario_label_relations, scenario_label_models, scenario_label_strides,
                   scenario_label_refusals, scenario_label_many_problems, scenario_label_full_waves]
SCENARIOS = PATH_SCENARIOS + LABEL_SCENARIOS + [scenario_learn]


# ---- MI355X ----------------------------------------------------------------------------------

@GPU
@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__[len("scenario_"):])
def test_gpu_joint_path(psd, scenario):
    scenario(psd, as_numpy)


_CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process
sys.path[:0] = [%(root)r, %(tests)r]
import test_gpu_joint_path as gp
gp.child_main()
print("joint-path-child ok")
"""


def child_main():
    import torch
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd as psd
    scenario_moving_peak(psd, as_cuda)      # windows, coverage and labels in cuda tensors, read in place
    scenario_groups(psd, as_cuda)
    scenario_label_models(psd, as_cuda)
    scenario_label_relations(psd, as_cuda)
    vectors = moving_peak()
    windows = [[(0, 400), (200, 400)]]
    penalties = [60.0, 0.0, 1e4]
    labels = [label_entry([(250, 300, NO_PEAKS)])] + [label_entry([(250, 300, PEAKS)])] * 3
    pset = psd.ProblemSet.from_dense([as_cuda(v) for v in vectors], [(c, INF) for c in range(4)])
    try:
        want = pset.joint_path([0] * 4, penalties, windows=wrap_windows(windows, as_numpy))
        try:                                # a bad label that only the device can see
            bad = [tuple(as_cuda(a) for a in label_entry([(250, 300, PEAKS), (9, 9, PEAKS)]))] + [None] * 3
            pset.joint_label_errors(bad)
            raise AssertionError("a label with chromStart >= chromEnd was accepted")
        except RuntimeError as e:
            assert e.status == 19 and "problem 0: label 1" in str(e), str(e)
        # the torch_device forms: tensors that alias the library's buffers
        out = pset.joint_path([0] * 4, penalties, windows=wrap_windows(windows, as_cuda),
                              torch_device="cuda:0")
        w_off, e_off, tensors = out[0], out[1], out[2:]
        assert w_off.tolist() == [0, 2] and e_off.tolist() == [0, 8]
        assert [tuple(t.shape) for t in tensors] == [(3, 2)] * 7 + [(3, 8)] * 4
        assert [t.dtype for t in tensors] == [torch.int32] * 4 + [torch.float64, torch.int32, torch.int32,
                                                                  torch.float64, torch.int32, torch.int64,
                                                                  torch.int32]
        kept = [t.cpu().numpy() for t in tensors]
        host = pset.joint_label_errors(labels)
        dev = pset.joint_label_errors([tuple(as_cuda(a) for a in e) for e in labels],
                                      torch_device="cuda:0")
        offs, count, fp, fn, problem, model = dev
        assert offs.tolist() == [0, 1, 2, 3, 4] and tuple(count.shape) == (3, 4)
        assert model.dtype == torch.int64 and np.array_equal(model.cpu().numpy(), host[0])
        assert np.array_equal(problem.cpu().numpy(), host[1])
        for p in range(3):
            for q in range(4):
                assert count[p, q].item() == host[2][p][q][0][0] and fn[p, q].item() == host[2][p][q][2][0]
    finally:
        pset.close()
    for p in range(3):
        for a, name in zip(kept[:7], FRAME):
            assert a[p].tobytes() == want[p][0]["joint"][name].to_numpy().tobytes(), name
        for a, name in zip(kept[7:], ("gain", "up", "sum", "bases")):
            assert a[p].tobytes() == want[p][0][name].tobytes(), name


@GPU
def test_gpu_joint_path_cuda_tensors(psd):
    """windows, samples and labels in cuda tensors, the device-side check of the labels, and the
    torch_device forms"""
    import subprocess
    import sys
    from conftest import ROOT
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(p.stdout[-4000:])
    assert p.returncode == 0 and "joint-path-child ok" in p.stdout, p.stdout[-3000:] + p.stderr[-6000:]
