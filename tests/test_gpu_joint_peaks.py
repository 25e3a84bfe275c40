"""ProblemSet.joint_peaks: one common peak per window for all members of a group, searched level by
level on the device from the resident runs, and joint_peaks_dense / joint_peaks_reads.

The scenario functions are shared with the emulator rehearsal (tests/test_joint_peaks_emu.py).  The
yardstick is joint_ref.joint_peaks_ref(): it asserts on the CPU, before any device result is looked
at, that at every level of every window the best candidate leads the runner-up by more than 4 E (E:
the bound on the device's rounding); then peaks, up, samples_up, sum, bases and levels are compared
for equality, gain and objective within E.  Every call is made twice: the second gives the same
bits.  The shapes are the smallest at which each part can go wrong (each scenario says which)."""
import ctypes
import os

import numpy as np
import pytest

from joint_ref import cluster_window, joint_peaks_ref
from test_gpu_dense import as_cuda, as_numpy

GPU = pytest.mark.gpu
FRAME = ["windowStart", "windowEnd", "peakStart", "peakEnd", "objective", "samples_up", "levels"]


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


def wrap_windows(windows, wrap):
    """a list over groups of lists of (start, end) -> what joint_peaks takes"""
    out = []
    for entry in windows:
        if not entry:
            out.append(None)
            continue
        out.append((wrap(np.array([w[0] for w in entry], np.int32)),
                    wrap(np.array([w[1] for w in entry], np.int32))))
    return out


def same_bits(a, b):
    for x, y in zip(a, b):
        assert x["joint"].equals(y["joint"])
        assert x["joint"]["objective"].to_numpy().tobytes() == y["joint"]["objective"].to_numpy().tobytes()
        assert x["gain"].tobytes() == y["gain"].tobytes()
        assert all(np.array_equal(x[n], y[n]) for n in ("up", "sum", "bases"))


def check_group(entry, vectors, firsts, windows, penalty, what=""):
    """one group of joint_peaks() against the yardstick -> the yardstick's results"""
    frame = entry["joint"]
    assert list(frame.columns) == FRAME
    assert all(frame[n].dtype == np.int32 for n in FRAME if n != "objective")
    assert frame["objective"].dtype == np.float64 and len(frame) == len(windows)
    m = len(vectors)
    assert entry["gain"].dtype == np.float64 and entry["sum"].dtype == np.int64
    assert entry["up"].dtype == entry["bases"].dtype == np.int32
    assert all(entry[n].shape == (len(windows), m) for n in ("gain", "up", "sum", "bases"))
    refs = []
    for k, window in enumerate(windows):
        ref = joint_peaks_ref(vectors, firsts, window, penalty)      # (asserts the margins)
        refs.append(ref)
        row = frame.iloc[k]
        got = [int(row[n]) for n in FRAME if n != "objective"]
        want = [ref[n] for n in FRAME if n != "objective"]
        assert got == want, (what, k, window, got, want, ref["trace"])
        assert abs(np.longdouble(row["objective"]) - ref["objective"]) <= ref["E"], (what, k)
        assert np.all(abs(entry["gain"][k].astype(np.longdouble) - ref["gain"]) <= ref["E"]), (what, k)
        for name in ("up", "sum", "bases"):
            assert np.array_equal(entry[name][k], ref[name]), (what, k, name, entry[name][k], ref[name])
        assert int(entry["up"][k].sum()) == int(row["samples_up"])
    return refs


def run_case(psd, wrap, vectors, firsts, groups, windows, penalty, what=""):
    """A set of one problem per vector (never solved), joint_peaks on `windows` (a list over groups
    of lists of (start, end)), twice, and every group against the yardstick.  -> (result, refs)"""
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors],
                                     [(c, float("inf")) for c in range(len(vectors))])
    try:
        result = pset.joint_peaks(groups, penalty=penalty, windows=wrap_windows(windows, wrap),
                                  first_chromStart=firsts)
        again = pset.joint_peaks(groups, penalty=penalty, windows=wrap_windows(windows, wrap),
                                 first_chromStart=firsts)
        ms = ctypes.c_float(-1.0)
        assert _lib().peakseg_hip_joint_peaks_last_ms(ctypes.byref(ms)) == 0 and ms.value >= 0.0
    finally:
        pset.close()
    same_bits(result, again)
    assert len(result) == len(windows)
    refs = []
    for g, entry in enumerate(result):
        members = [p for p in range(len(groups)) if groups[p] == g]
        assert entry["members"].tolist() == members
        refs.append(check_group(entry, [vectors[p] for p in members], [firsts[p] for p in members],
                                windows[g], penalty, "%s group %d" % (what, g)))
    return result, refs


def bumps(length, first, spans, base=2, ripple=False):
    """per-base coverage: `base` everywhere and (start, end, height) bumps in genomic coordinates;
    with ripple every other base is one higher: a run per base"""
    v = np.full(length, base, dtype=np.int32)
    for a, b, h in spans:
        v[a - first:b - first] = h
    if ripple:
        v[1::2] += 1
    return v


# ---- the scenarios ---------------------------------------------------------------------------

def scenario_widths(psd, wrap):
    """W = 2 (no peak), 3 (one candidate), 64 (b = 1, n = 64), 65 (b = 2, n = 33, a last bin of one
    base), 128 and 129; two members"""
    spans = [(150, 170, 50), (300, 301, 90), (420, 470, 60)]
    vectors = [bumps(600, 0, spans), bumps(600, 0, [(a, b, h - 9) for a, b, h in spans], base=3)]
    windows = [[(140, 142), (299, 302), (128, 192), (128, 193), (100, 228), (100, 229), (400, 529)]]
    result, refs = run_case(psd, wrap, vectors, [0, 0], [0, 0], windows, 0.0, "widths")
    frame = result[0]["joint"]
    assert frame["levels"].tolist() == [0, 1, 1, 2, 2, 3, 3]
    assert frame["peakStart"].tolist() == [-1, 300, 150, 150, 150, 150, 420]
    assert frame["peakEnd"].tolist() == [-1, 301, 170, 170, 170, 170, 470]
    assert frame["samples_up"].tolist() == [0, 2, 2, 2, 2, 2, 2] and frame["objective"][0] == 0.0
    assert result[0]["sum"][1].tolist() == [90, 81] and result[0]["bases"][0].tolist() == [0, 0]


def scenario_wide(psd, wrap):
    """W = 2^20 + 1 on contigs of a few hundred runs: b = 2^15 at level 0, sixteen levels, a short
    last bin at every level; the peak's ends are odd coordinates"""
    rng = np.random.default_rng(7)
    n = 2 ** 20 + 1
    vectors = []
    for k in range(2):
        cuts = np.sort(rng.choice(np.arange(1, n), 300, replace=False))
        v = np.repeat(rng.integers(3, 7, 301), np.diff(np.concatenate([[0], cuts, [n]]))).astype(np.int32)
        v[333333:777778] += 100 + 20 * k
        vectors.append(v)
    result, refs = run_case(psd, wrap, vectors, [5000, 5000], [0, 0], [[(5000, 5000 + n)]], 0.0, "wide")
    assert result[0]["joint"]["levels"].tolist() == [16]
    assert result[0]["joint"]["peakStart"].tolist() == [5000 + 333333]
    assert result[0]["joint"]["peakEnd"].tolist() == [5000 + 777778]
    assert [t["b"] for t in refs[0][0]["trace"]] == [2 ** k for k in range(15, -1, -1)]


def scenario_peak_ends(psd, wrap):
    """W = 1024 (b = 16): the true ends on level 0's boundaries, one base off them, within four
    half-bins of ws and of we (candidates clipped by ws < s, e < we), and a peak whose level-0
    choice the refinement must move by four half-bins (asserted from the yardstick's trace)"""
    placed = [(320, 640), (321, 639), (3, 1021), (5, 40), (990, 1020)]
    windows = [(2000 * k + 100, 2000 * k + 1124) for k in range(len(placed))]
    spans = [(ws + a, ws + c, 40 + k) for k, ((ws, _), (a, c)) in enumerate(zip(windows, placed))]
    vectors = [bumps(11000, 0, spans), bumps(11000, 0, [(a, b, h + 5) for a, b, h in spans])]
    # a group of its own: a core [559, 633) with a separate low bump [527, 537) to its left: level 0
    # takes the bump's bin in (s = 528), the next level drops it (s = 560): four half-bins of 8
    vectors.append(bumps(1024, 0, [(559, 633, 80), (527, 537, 51)], base=1))
    result, refs = run_case(psd, wrap, vectors, [0, 0, 0], [0, 0, 1], [windows, [(0, 1024)]], 0.0,
                            "peak ends")
    frame = result[0]["joint"]
    for k, ((ws, _), (a, c)) in enumerate(zip(windows, placed)):
        assert (frame["peakStart"][k], frame["peakEnd"][k]) == (ws + a, ws + c), k
    assert frame["levels"].tolist() == [5] * len(windows)
    trace = refs[1][0]["trace"]
    assert [(t["b"], t["s"]) for t in trace[:2]] == [(16, 528), (8, 560)]
    assert (result[1]["joint"]["peakStart"][0], result[1]["joint"]["peakEnd"][0]) == (559, 633)


def member_vector(k, kind="peak"):
    v = np.full(200, 3 + k % 4, dtype=np.int32)
    if kind == "peak":
        v[70:110] = 40 + (k * 7) % 23
    elif kind == "dip":
        v[:] = 30
        v[70:110] = 4
    elif kind == "weak":
        v[70:110] = 5 + k % 4
    elif kind == "zero":
        v[:] = 0
    return v


def scenario_members(psd, wrap):
    """groups of 1, 2, 64, 65 and 257 members (past a wave's members and an LDS slab), W = 160
    (b = 4); in the group of 65 an all-zero member, a member with a dip where the others peak
    (infeasible: gain 0, up 0) and one whose peak is weaker than the penalty (feasible, up 0);
    then a penalty so large that no member is up: no joint peak anywhere"""
    sizes = [1, 2, 64, 65, 257]
    vectors, groups = [], []
    for g, size in enumerate(sizes):
        for k in range(size):
            kind = {3: "zero", 40: "dip", 64: "weak"}.get(k, "peak") if size == 65 else "peak"
            vectors.append(member_vector(k, kind))
            groups.append(g)
    firsts = [1000] * len(vectors)
    windows = [[(1020, 1180)]] * len(sizes)
    result, refs = run_case(psd, wrap, vectors, firsts, groups, windows, 25.0, "members")
    for g, size in enumerate(sizes):
        row = result[g]["joint"].iloc[0]
        assert (row["peakStart"], row["peakEnd"], row["levels"]) == (1070, 1110, 3), g
        assert row["samples_up"] == (size - 3 if size == 65 else size)
    special = result[3]
    assert special["up"][0, [3, 40, 64]].tolist() == [0, 0, 0]
    assert special["gain"][0, 3] == 0.0 and special["gain"][0, 40] == 0.0     # zero, infeasible
    assert 0.0 < special["gain"][0, 64] < 25.0                                  # feasible, not up
    assert special["sum"][0, 3] == 0 and special["sum"][0, 40] == 160
    result, _ = run_case(psd, wrap, vectors, firsts, groups, windows, 1e9, "large penalty")
    for entry in result:
        assert entry["joint"]["peakStart"].tolist() == [-1] and entry["joint"]["objective"][0] == 0.0
        assert not entry["gain"].any() and not entry["up"].any() and not entry["sum"].any()


def scenario_runs(psd, wrap):
    """contigs of a run per base, the second one's runs not 16-byte aligned: windows whose pieces
    straddle run ends, the 1024-run tile boundaries, and the 16-run threshold below which a piece is
    folded by its own thread (bins of 1, 8, 16, 32 and 64 runs)"""
    tile = _lib().peakseg_hip_region_stats_tile_runs()
    assert tile == 1024
    spans = [(1010, 1040, 60), (2040, 2060, 80)]
    vectors = [bumps(2601, 0, spans, ripple=True), bumps(2600, 0, spans, base=4, ripple=True)]
    windows = [[(1000, 1064), (900, 1200), (512, 1536), (512, 1537), (0, 2600), (2030, 2070),
                (2036, 2064)]]
    result, _ = run_case(psd, wrap, vectors, [0, 0], [0, 0], windows, 0.0, "runs")
    assert result[0]["joint"]["peakStart"].tolist() == [1010, 1010, 1010, 1010, 1010, 2040, 2040]
    half = np.array([60, 61] * 15, np.int64).sum()
    assert result[0]["sum"][1].tolist() == [half, half]


def scenario_clipping(psd, wrap):
    """members with different first and length: the windows are clipped to the intersection
    [1100, 1600); windows partly and wholly outside it"""
    spans = [(1150, 1200, 50), (1530, 1570, 70), (1593, 1596, 90)]
    vectors = [bumps(600, 1000, spans), bumps(700, 1100, spans, base=3)]
    windows = [[(900, 1300), (1500, 2000), (100, 200), (1590, 1700), (1700, 1800), (1598, 2000)]]
    result, _ = run_case(psd, wrap, vectors, [1000, 1100], [0, 0], windows, 0.0, "clipping")
    frame = result[0]["joint"]
    assert frame["windowStart"].tolist() == [1100, 1500, 1100, 1590, 1700, 1598]
    assert frame["windowEnd"].tolist() == [1300, 1600, 1100, 1600, 1700, 1600]
    assert frame["peakStart"].tolist() == [1150, 1530, -1, 1593, -1, -1]


def scenario_big_counts(psd, wrap):
    """counts near 2^31 - 1 on W = 2^20: sums near 2^51, feasibility products past 2^64; a 1 : 2
    step keeps the margins"""
    n = 2 ** 20
    top = 2 ** 31 - 1
    vectors = []
    for k in range(2):
        v = np.full(n, top // 2 - k, dtype=np.int32)
        v[300001:700000] = top - 3 * k
        vectors.append(v)
    result, refs = run_case(psd, wrap, vectors, [0, 0], [0, 0], [[(0, n)]], 0.0, "big counts")
    assert result[0]["joint"]["peakStart"].tolist() == [300001]
    assert result[0]["joint"]["peakEnd"].tolist() == [700000]
    s2 = int(result[0]["sum"][0, 0])
    assert s2 == 399999 * top and s2 * 300001 > 2 ** 64 and int(vectors[0].astype(np.int64).sum()) > 2 ** 50


def scenario_groups(psd, wrap):
    """a group without members (its window has no joint peak) and a group without windows between
    groups with some"""
    spans = [(150, 170, 50)]
    vectors = [bumps(400, 0, spans, base=2 + k) for k in range(6)]
    groups = [0, 0, 2, 2, 3, 3]
    windows = [[(100, 228)], [(100, 228), (0, 50)], [], [(120, 200), (140, 180)]]
    result, _ = run_case(psd, wrap, vectors, [0] * 6, groups, windows, 0.0, "groups")
    assert result[1]["joint"]["peakStart"].tolist() == [-1, -1] and result[1]["gain"].shape == (2, 0)
    assert len(result[2]["joint"]) == 0 and result[2]["gain"].shape == (0, 2)
    assert result[3]["joint"]["peakStart"].tolist() == [150, 150]
    # no group at all
    pset = psd.ProblemSet.from_dense([wrap(vectors[0])], [(0, 1.0)])
    try:
        assert pset.joint_peaks([-1], windows=[]) == []
    finally:
        pset.close()


def raw_joint(pset, n_groups, group, penalty, counts, starts, ends):
    out = [ctypes.c_void_p() for _ in range(11)]
    g = as_numpy(group)
    keep = [as_numpy(a) for a in starts + ends]
    k = len(starts)
    tables = [(ctypes.c_longlong * max(k, 1))(*counts),
              (ctypes.c_void_p * max(k, 1))(*[a.ctypes.data for a in keep[:k]]),
              (ctypes.c_void_p * max(k, 1))(*[a.ctypes.data for a in keep[k:]])]
    return _lib().peakseg_hip_problem_set_pack_joint_peaks(
        pset._h, None, n_groups, g.ctypes.data, penalty, *[ctypes.addressof(a) for a in tables],
        0, None, None, *[ctypes.byref(q) for q in out])


def nothing_packed(pset):
    out = [np.zeros(64, dt) for dt in (np.int32,) * 4 + (np.float64, np.int32, np.int32, np.float64,
                                                         np.int32, np.int64, np.int32)]
    return _lib().peakseg_hip_problem_set_packed_joint_peaks_download(
        pset._h, *[a.ctypes.data for a in out]) == -1


def scenario_refusals(psd, wrap):
    from peaksegdisk_amd import _native
    from test_gpu_dense import rle
    vectors = [bumps(400, 0, [(150, 170, 50)], base=2 + k) for k in range(4)]
    groups = [0, 0, 1, 1]
    good = [[(100, 228)], [(100, 228), (120, 200)]]
    pset = psd.ProblemSet.from_dense([as_numpy(v) for v in vectors], [(c, 10.0) for c in range(4)])
    try:
        with pytest.raises(RuntimeError, match="group 1: window 1") as ei:
            pset.joint_peaks(groups, windows=wrap_windows([good[0], [(100, 228), (200, 200)]], wrap))
        assert ei.value.status == 22 and nothing_packed(pset)
        for penalty in (-1.0, float("nan")):
            with pytest.raises(RuntimeError, match="penalty") as ei:
                pset.joint_peaks(groups, penalty=penalty, windows=wrap_windows(good, wrap))
            assert ei.value.status == 22 and nothing_packed(pset)
        with pytest.raises(RuntimeError) as ei:                       # no windows: needs a solve
            pset.joint_peaks(groups)
        assert ei.value.status == 13
        assert raw_joint(pset, 2, groups, 0.0, [-1, 0], [[0], [0]], [[1], [1]]) == -22
        assert "group 0 has -1 windows" in _lib().peakseg_hip_last_error().decode()
        assert raw_joint(pset, 2, [0, 0, 1, 2], 0.0, [0, 0], [[0], [0]], [[1], [1]]) == -22
        assert "problem 3" in _lib().peakseg_hip_last_error().decode()
        with pytest.raises(ValueError, match="one group per problem"):
            pset.joint_peaks([0], windows=[None])
        with pytest.raises(ValueError, match="one entry of windows per group"):
            pset.joint_peaks(groups, windows=[None])
        with pytest.raises(RuntimeError, match="32-bit"):
            pset.joint_peaks(groups, windows=wrap_windows(good, wrap),
                             first_chromStart=[0, 0, 0, 2147483647 - 10])
        answer = pset.joint_peaks(groups, windows=wrap_windows(good, wrap))   # the set still answers
        assert answer[1]["joint"]["peakStart"].tolist() == [150, 150] and not nothing_packed(pset)
        room = pset.hbm_bytes
    finally:
        pset.close()
    count, weight, _ = rle(vectors[0])
    plain = psd.ProblemSet([(count, weight)], [(0, 10.0)])
    try:
        with pytest.raises(RuntimeError, match="dense"):
            plain.joint_peaks([0], windows=wrap_windows([[(100, 228)]], wrap))
    finally:
        plain.close()
    # tables that do not fit: the same set again, allowed 8 bytes less than everything it held
    # after its tables were there: status 14, and nothing was allocated
    os.environ["PEAKSEG_HIP_MAX_BYTES"] = str(room - 8)
    try:
        capped = psd.ProblemSet.from_dense([as_numpy(v) for v in vectors], [(c, 10.0) for c in range(4)])
    finally:
        del os.environ["PEAKSEG_HIP_MAX_BYTES"]
    try:
        before = capped.hbm_bytes
        with pytest.raises(RuntimeError, match="do not fit") as ei:
            capped.joint_peaks(groups, windows=wrap_windows(good, wrap))
        assert ei.value.status == _native.ERROR_DEVICE_MEMORY == 14
        assert capped.hbm_bytes == before and nothing_packed(capped)
    finally:
        capped.close()


def scenario_solved(psd, wrap):
    """the solved set of the cluster tests (six step-function contigs in two groups), windows=None:
    the clusters are the expected ones, the joint peak of each equals the yardstick's on the
    cluster's window, and it lies inside that window"""
    from consensus_ref import cluster_ref
    from test_gpu_peak_clusters import GROUPS, PROBLEMS, SAMPLES, member_peaks, steps
    firsts = [s[0] for s in SAMPLES]
    vectors = [steps(length, first, spans) for first, length, spans in SAMPLES]
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors], PROBLEMS)
    try:
        pset.solve()
        columns = pset.segment_columns(first_chromStart=firsts)
        clusters = pset.peak_clusters(GROUPS, first_chromStart=firsts)
        result = pset.joint_peaks(GROUPS, penalty=5.0, first_chromStart=firsts)
        again = pset.joint_peaks(GROUPS, penalty=5.0, first_chromStart=firsts)
        after = pset.peak_clusters(GROUPS, first_chromStart=firsts)
    finally:
        pset.close()
    same_bits(result, again)
    for g in range(2):
        members = [p for p in range(len(GROUPS)) if GROUPS[p] == g]
        want_table, _ = cluster_ref([member_peaks(columns[p]) for p in members])
        table = clusters[g]["clusters"].to_numpy().astype(np.int64).reshape(-1, 4)
        assert np.array_equal(table, want_table) and len(table) >= 2
        assert clusters[g]["clusters"].equals(after[g]["clusters"])
        windows = [cluster_window(cs, ce) for cs, ce in table[:, :2].tolist()]
        contigs = [PROBLEMS[p][0] for p in members]
        check_group(result[g], [vectors[c] for c in contigs], [firsts[c] for c in contigs], windows,
                    5.0, "solved group %d" % g)
        frame = result[g]["joint"]
        assert (frame["peakStart"] >= 0).any()
        for k, (ws, we) in enumerate(windows):
            if frame["peakStart"][k] >= 0:
                assert ws < frame["peakStart"][k] < frame["peakEnd"][k] < we


def scenario_api(psd, wrap):
    """joint_peaks_dense on three samples x two regions equals the composition of its parts, and
    joint_peaks_reads on the same coverage as reads equals it"""
    firsts = [1000, 1500, 500, 0, 200, 0]
    spans = [[(2000, 2500, 50), (5000, 5400, 50)], [(2100, 2400, 40), (5100, 5500, 45)],
             [(2050, 2450, 30), (5050, 5350, 60)], [(1000, 1400, 50)], [(1100, 1500, 50)],
             [(1050, 1450, 45)]]
    lengths = [6000, 5000, 6500, 3000, 2500, 3000]
    vectors = [bumps(n, f, s) for n, f, s in zip(lengths, firsts, spans)]
    groups = [0, 0, 0, 1, 1, 1]
    out = psd.joint_peaks_dense([wrap(v) for v in vectors], penalties=10.0, groups=groups,
                                joint_penalty=3.0, chrom=["chrA", "chrB"], chrom_starts=firsts)
    assert len(out.groups) == 2 and len(out.fits) == 6
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors], [(c, 10.0) for c in range(6)])
    try:
        pset.solve()
        clusters = pset.peak_clusters(groups, first_chromStart=firsts)
        joint = pset.joint_peaks(groups, penalty=3.0, first_chromStart=firsts)
    finally:
        pset.close()
    for g in range(2):
        entry = out.groups[g]
        assert list(entry["joint"].columns) == ["chrom"] + FRAME
        assert set(entry["joint"]["chrom"]) == {["chrA", "chrB"][g]}
        assert entry["joint"].iloc[:, 1:].equals(joint[g]["joint"])
        assert entry["clusters"].iloc[:, 1:].equals(clusters[g]["clusters"])
        assert entry["gain"].tobytes() == joint[g]["gain"].tobytes()
        assert np.array_equal(entry["up"], joint[g]["up"])
        assert np.array_equal(entry["joint_sum"], joint[g]["sum"])
        assert np.array_equal(entry["joint_bases"], joint[g]["bases"])
        members = [p for p in range(6) if groups[p] == g]
        windows = [cluster_window(cs, ce) for cs, ce in
                   clusters[g]["clusters"][["clusterStart", "clusterEnd"]].to_numpy().tolist()]
        check_group(joint[g], [vectors[p] for p in members], [firsts[p] for p in members], windows,
                    3.0, "api group %d" % g)
        assert (joint[g]["joint"]["samples_up"] == 3).all() and len(windows) == (2, 1)[g]
    with pytest.raises(ValueError, match="2 groups"):
        out.joint
    with pytest.raises(ValueError, match="joint_penalty"):
        psd.joint_peaks_dense([wrap(v) for v in vectors], penalties=10.0, joint_penalty=-1.0)
    reads = []
    for v, first in zip(vectors[3:], firsts[3:]):
        at = np.arange(len(v), dtype=np.int64) + first
        reads.append(tuple(wrap(as_numpy(a)) for a in (at, at + 1, v)))
    one = psd.joint_peaks_reads(reads, penalties=10.0, joint_penalty=3.0, chrom="chrB")
    assert one.joint.equals(out.groups[1]["joint"]) and one.gain.tobytes() == out.groups[1]["gain"].tobytes()
    assert np.array_equal(one.up, out.groups[1]["up"])


def many_windows_case():
    """300 windows of 40 bases (b = 1, one level) side by side on three contigs of 12 040 bases,
    a bump in each whose end and height move with the window; two members in the first group with
    259 windows, one in the second with 41 -> (vectors, firsts, groups, windows, peaks)"""
    first, n = 20, 300
    spans = [(first + 40 * k + 10, first + 40 * k + 20 + k % 7, 30 + k % 5) for k in range(n)]
    vectors = [bumps(12040, first, [(a, b, h + 7 * c) for a, b, h in spans], base=2 + c)
               for c in range(3)]
    every = [(first + 40 * k, first + 40 * k + 40) for k in range(n)]
    return vectors, [first] * 3, [0, 0, 1], [every[:259], every[259:]], [s[:2] for s in spans]


def scenario_many_windows(psd, wrap):
    """300 windows in two groups: setup_kernel has a thread per window, so it needs a second
    workgroup of 256, and the second workgroup holds the last windows of the first group and all
    of the second's (its search of win_off gives both answers within one workgroup)"""
    vectors, firsts, groups, windows, peaks = many_windows_case()
    threads = 256                                    # joint_peaks.h's THREADS
    assert threads < len(windows[0]) < len(windows[0]) + len(windows[1]) < 2 * threads
    assert len(windows[0]) % threads != 0 and len(windows[1]) > 0
    result, _ = run_case(psd, wrap, vectors, firsts, groups, windows, 20.0, "many windows")
    found = [(int(a), int(b)) for entry in result
             for a, b in zip(entry["joint"]["peakStart"], entry["joint"]["peakEnd"])]
    assert found == peaks
    assert all(entry["joint"]["levels"].tolist() == [1] * len(entry["joint"]) for entry in result)
    assert result[0]["up"].all() and result[1]["up"].all()


SCENARIOS = [scenario_widths, scenario_wide, scenario_peak_ends, scenario_members, scenario_runs,
             scenario_clipping, scenario_big_counts, scenario_groups, scenario_refusals,
             scenario_solved, scenario_api, scenario_many_windows]


# ---- MI355X ----------------------------------------------------------------------------------

@GPU
@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__[len("scenario_"):])
def test_gpu_joint_peaks(psd, scenario):
    scenario(psd, as_numpy)


def parity_case():
    """a small call with every kind of window: (vectors, firsts, groups, windows, penalty)"""
    spans = [(150, 170, 50), (300, 301, 90), (420, 470, 60)]
    vectors = [bumps(600, 0, [(a, b, h + 3 * k) for a, b, h in spans], base=2 + k % 3, ripple=k % 2 == 1)
               for k in range(67)]
    groups = [0] * 65 + [1] * 2
    windows = [[(100, 229), (299, 302), (380, 600)], [(0, 600), (140, 142)]]
    return vectors, [0] * 67, groups, windows, 7.5


def joint_bits(psd, lib=None):
    """the columns of parity_case() as bytes, from the library in use or from `lib`"""
    from peaksegdisk_amd import _native
    vectors, firsts, groups, windows, penalty = parity_case()
    real = _native.lib
    if lib is not None:
        _native.lib = lib
    try:
        pset = psd.ProblemSet.from_dense([as_numpy(v) for v in vectors],
                                         [(c, float("inf")) for c in range(len(vectors))])
        try:
            result = pset.joint_peaks(groups, penalty=penalty, windows=wrap_windows(windows, as_numpy))
        finally:
            pset.close()
    finally:
        _native.lib = real
    return [(e["joint"].to_numpy().tobytes(), e["gain"].tobytes(), e["up"].tobytes(),
             e["sum"].tobytes(), e["bases"].tobytes()) for e in result]


@GPU
def test_gpu_joint_peaks_equal_the_emulator_bit_for_bit(psd):
    """objective and gain are fixed sequences of IEEE operations, the deterministic log and the
    repaired division: the emulator's digits are the device's"""
    import subprocess
    from conftest import ROOT
    from peaksegdisk_amd import _native
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["make", "-s", "-C", emu_dir], check=True)
    emu = _native.declare(ctypes.CDLL(os.path.join(emu_dir, "_build", "libpeaksegdisk_emu.so")))
    device, emulator = joint_bits(psd), joint_bits(psd, emu)
    assert device == emulator
    assert any(np.frombuffer(g[1], np.float64).any() for g in device)


_CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process
sys.path[:0] = [%(root)r, %(tests)r]
import test_gpu_joint_peaks as gj
gj.child_main()
print("joint-child ok")
"""


def child_main():
    import torch
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd as psd
    scenario_widths(psd, as_cuda)           # windows and coverage in cuda tensors, read in place
    scenario_groups(psd, as_cuda)
    scenario_api(psd, as_cuda)
    vectors, firsts, groups, windows, penalty = parity_case()
    pset = psd.ProblemSet.from_dense([as_cuda(v) for v in vectors],
                                     [(c, float("inf")) for c in range(len(vectors))])
    try:
        # a bad window that only the device can see: the first launch's check word
        bad = [windows[0], [(0, 600), (142, 140)]]
        try:
            pset.joint_peaks(groups, penalty=penalty, windows=wrap_windows(bad, as_cuda))
            raise AssertionError("a window with start >= end was accepted")
        except RuntimeError as e:
            assert e.status == 22 and "group 1: window 1" in str(e), str(e)
        try:                                # one call takes one kind of memory
            mixed = wrap_windows(windows, as_cuda)
            mixed[1] = wrap_windows(windows, as_numpy)[1]
            pset.joint_peaks(groups, penalty=penalty, windows=mixed)
            raise AssertionError("host and device windows in one call were accepted")
        except ValueError as e:
            assert "one call takes one kind" in str(e)
        want = pset.joint_peaks(groups, penalty=penalty, windows=wrap_windows(windows, as_numpy))
        from_device = pset.joint_peaks(groups, penalty=penalty, windows=wrap_windows(windows, as_cuda))
        same_bits(want, from_device)
        # the torch_device form: tensors that alias the library's buffers
        out = pset.joint_peaks(groups, penalty=penalty, windows=wrap_windows(windows, as_cuda),
                               torch_device="cuda:0")
        w_off, e_off, tensors = out[0], out[1], out[2:]
        assert [t.dtype for t in tensors] == [torch.int32] * 4 + [torch.float64, torch.int32, torch.int32,
                                                                  torch.float64, torch.int32, torch.int64,
                                                                  torch.int32]
        assert w_off.tolist() == [0, 3, 5] and e_off.tolist() == [0, 195, 199]
        kept = [t.cpu().numpy() for t in tensors]
        again = pset.joint_peaks(groups, penalty=penalty, windows=wrap_windows(windows, as_cuda),
                                 torch_device="cuda:0")
        assert [t.data_ptr() for t in again[2:]] == [t.data_ptr() for t in tensors]
    finally:
        pset.close()
    for g in (0, 1):
        rows, cells = slice(w_off[g], w_off[g + 1]), slice(e_off[g], e_off[g + 1])
        for a, name in zip(kept[:7], FRAME):
            assert a[rows].tobytes() == want[g]["joint"][name].to_numpy().tobytes(), name
        for a, name in zip(kept[7:], ("gain", "up", "sum", "bases")):
            assert a[cells].tobytes() == want[g][name].tobytes(), name


@GPU
def test_gpu_joint_peaks_cuda_tensors(psd):
    """windows and samples in cuda tensors, the device-side check of the windows, and the
    torch_device form"""
    import subprocess
    import sys
    from conftest import ROOT
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(p.stdout[-4000:])
    assert p.returncode == 0 and "joint-child ok" in p.stdout, p.stdout[-3000:] + p.stderr[-6000:]
