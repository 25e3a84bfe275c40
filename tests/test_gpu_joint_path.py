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
        for p, penalty in enumerate(penalties):
            for g, entry in enumerate(models[p]):
                members = [q for q in range(len(groups)) if groups[q] == g]
                check_group(entry, [vectors[q] for q in members], [firsts[q] for q in members],
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


def scenario_members(psd, wrap):
    """groups of 1, 64, 65 and 130 members with three penalties each: the accumulators of several
    penalties across the boundaries of the slabs of 64 members (and of the smaller slabs of the
    later levels); in the group of 65 an all-zero member, an infeasible one and a weak one"""
    sizes = [1, 64, 65, 130]
    vectors, groups = [], []
    for g, size in enumerate(sizes):
        for k in range(size):
            kind = {3: "zero", 40: "dip", 64: "weak"}.get(k, "peak") if size == 65 else "peak"
            vectors.append(member_vector(k, kind))
            groups.append(g)
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
                  scenario_groups, scenario_solved, scenario_independence]
LABEL_SCENARIOS = [scenario_label_relations, scenario_label_models, scenario_label_strides,
                   scenario_label_refusals]
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
