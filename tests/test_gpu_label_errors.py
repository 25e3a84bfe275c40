"""ProblemSet.label_errors: the label errors of every model of a solved set, counted on the device
from the resident segment tables.

The scenario functions are shared with the emulator rehearsal (tests/test_label_errors_emu.py),
which runs them without a GPU on host arrays; the tests marked gpu run them on the MI355X with the
labels once as numpy arrays (in this process) and once as cuda tensors (in a child process that
imports torch first, as tests/test_gpu_dense.py does).

The yardstick never comes from the library: brute_force() takes the segment_columns() rows of a
model and the labels, looks at every (peak, label) pair and applies the three definitions of
include/peaksegdisk_hip.h as they are written -- no closed form, no search.  Everything is integer
arithmetic, so the comparisons are for equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_dense import as_cuda, as_numpy, mono27ac_dense, rle

GPU = pytest.mark.gpu
NO_PEAKS, PEAK_START, PEAK_END, PEAKS = 0, 1, 2, 3


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


# ---- the yardstick ---------------------------------------------------------------------------

def peaks_of(columns):
    """the peaks [ps, pe) of a model: the odd rows of its segment_columns()"""
    start, end = np.asarray(columns[0], np.int64), np.asarray(columns[1], np.int64)
    return start[1::2], end[1::2]


def brute_force(columns, labels):
    """(count, fp, fn int32 arrays, [errors, fp, fn, possible_fp, possible_fn]) of one model"""
    ps, pe = peaks_of(columns)
    starts, ends, codes = (np.asarray(a, np.int64) for a in labels)
    n = len(starts)
    count, fp, fn = (np.zeros(n, np.int32) for _ in range(3))
    for i in range(n):
        ls, le, a = int(starts[i]), int(ends[i]), int(codes[i])
        overlapping = int(np.sum((ps < le) & (ls < pe)))
        starts_in = int(np.sum((ls <= ps) & (ps < le)))
        ends_in = int(np.sum((ls < pe) & (pe <= le)))
        if a == NO_PEAKS:
            count[i], fp[i] = overlapping, overlapping >= 1
        elif a == PEAKS:
            count[i], fn[i] = overlapping, overlapping == 0
        elif a == PEAK_START:
            count[i], fp[i], fn[i] = starts_in, starts_in >= 2, starts_in == 0
        else:
            assert a == PEAK_END
            count[i], fp[i], fn[i] = ends_in, ends_in >= 2, ends_in == 0
    totals = [int(fp.sum() + fn.sum()), int(fp.sum()), int(fn.sum()), int(np.sum(codes != PEAKS)),
              int(np.sum(codes != NO_PEAKS))]
    return count, fp, fn, totals


EMPTY = tuple(np.zeros(0, np.int32) for _ in range(3))


def wrap_labels(labels, wrap):
    return [None if e is None or len(e[0]) == 0 else tuple(wrap(a) for a in e) for e in labels]


def check_set(pset, labels, firsts, wrap, what=""):
    """every problem's columns and totals against the yardstick; -> (totals, per_label, columns)"""
    columns = pset.segment_columns(first_chromStart=firsts)
    totals, per_label = pset.label_errors(wrap_labels(labels, wrap), first_chromStart=firsts)
    assert totals.dtype == np.int32 and totals.shape == (len(pset.problems), 5)
    assert len(per_label) == len(pset.problems)
    for k, (c, pen) in enumerate(pset.problems):
        entry = EMPTY if labels[c] is None else labels[c]
        want = brute_force(columns[k], entry)
        for name, g, w in zip(("count", "fp", "fn"), per_label[k], want[:3]):
            assert g.dtype == np.int32 and len(g) == len(entry[0]), (what, k, name)
            bad = np.flatnonzero(g != w)
            assert len(bad) == 0, (what, k, pen, name, bad[:5].tolist(), g[bad[:5]].tolist(),
                                   w[bad[:5]].tolist(), [entry[j][bad[:5]].tolist() for j in range(3)])
        assert totals[k].tolist() == want[3], (what, k, pen, totals[k].tolist(), want[3])
    return totals, per_label, columns


def golden_labels():
    from peaksegdisk_amd import read_labels_bed
    return read_labels_bed(os.path.join(GOLDEN, "Mono27ac.labels.bed"))


# ---- scenario 1: Mono27ac with its golden labels ---------------------------------------------

def scenario_mono27ac(psd, wrap):
    dense = mono27ac_dense()
    labels, chrom = golden_labels()
    assert len(labels[0]) == 6 and set(chrom) == {"chr11"}
    pens = [0.0, 1952.6, 10000.0, float("inf")]
    pset = psd.ProblemSet.from_dense([as_numpy(dense)], [(0, p) for p in pens])
    try:
        pset.solve()
        totals, per_label, columns = check_set(pset, [labels], [60000], wrap, "Mono27ac")
        assert len(columns[3][0]) == 1
        # no peaks: only peakStart and peakEnd fail
        assert totals[3].tolist() == [2, 0, 2, 6, 2]
        assert per_label[3][2].tolist() == [0, 1, 1, 0, 0, 0]
    finally:
        pset.close()


# ---- scenario 2: ties by construction --------------------------------------------------------

def tie_contigs():
    """12 contigs of 300-3000 bases of synthetic coverage, trimmed so that the contigs' first runs
    lie at all four offsets modulo 4 in the set's run arrays"""
    from peaksegdisk_amd import synthetic
    lengths = [300, 3000, 777, 1500, 2048, 333, 1025, 2999, 450, 1800, 640, 1234]
    vectors, offset = [], 0
    for k, n in enumerate(lengths):
        v = synthetic.poisson_coverage(n, seed=20 + k)[2].astype(np.int32)
        # the NEXT contig shall begin at run offset (k + 1) % 4
        while (offset + len(rle(v)[0])) % 4 != (k + 1) % 4:
            v = v[:-1]
        assert 290 <= len(v) <= 3000
        vectors.append(v)
        offset += len(rle(v)[0])
    return vectors


def tie_labels(columns, n_bases, first, rng):
    """labels around the boundaries of the model `columns`, beyond both ends of the contig, and
    50 random ones"""
    ps, pe = (x[::-1] for x in peaks_of(columns))    # in genomic order
    assert len(ps) >= 2
    rows = []
    for b in (int(ps[len(ps) // 2]), int(pe[len(pe) // 2])):   # a peak start, a peak end
        for ls, le in ((b, b + 1), (b - 1, b), (b - 1, b + 1)):
            rows += [(ls, le, a) for a in range(4)]
    rows += [(int(ps[0]) - 3, int(ps[1]) + 2, a) for a in range(4)]    # spans two starts
    last = first + n_bases
    for ls, le in ((first - 50, first - 10), (first - 7, first), (last, last + 9), (last + 5, last + 60),
                   (first - 20, first + 30), (last - 30, last + 20), (first - 5, last + 5)):
        rows += [(ls, le, a) for a in range(4)]
    for _ in range(50):
        ls = int(rng.integers(first - 20, last + 10))
        rows.append((ls, ls + int(rng.integers(1, 400)), int(rng.integers(0, 4))))
    order = rng.permutation(len(rows))
    cols = np.array(rows, dtype=np.int64)[order]
    return tuple(np.ascontiguousarray(cols[:, j], dtype=np.int32) for j in range(3))


def scenario_ties(psd, wrap):
    vectors = tie_contigs()
    firsts = [1000 * (k % 3) + 17 * k for k in range(len(vectors))]
    pens = [0.5, 3.0]
    problems = [(c, p) for c in range(len(vectors)) for p in pens]
    rng = np.random.default_rng(11)
    pset = psd.ProblemSet.from_dense([as_numpy(v) for v in vectors], problems)
    try:
        pset.solve()
        offsets = np.concatenate([[0], np.cumsum([len(rle(v)[0]) for v in vectors])])[:-1]
        assert set((offsets % 4).tolist()) == {0, 1, 2, 3}
        columns = pset.segment_columns(first_chromStart=firsts)
        for k in range(len(problems)):
            assert (len(columns[k][0]) - 1) // 2 >= 2, (k, len(columns[k][0]))
        labels = [tie_labels(columns[2 * c], len(vectors[c]), firsts[c], rng)
                  for c in range(len(vectors))]
        # a condition on the input: every equality between a peak's end and a label's occurs
        for c in range(len(vectors)):
            ps, pe = peaks_of(columns[2 * c])
            ls, le = labels[c][0].astype(np.int64), labels[c][1].astype(np.int64)
            for name, x, y in (("ps == ls", ps, ls), ("ps == le", ps, le), ("pe == ls", pe, ls),
                               ("pe == le", pe, le)):
                assert np.intersect1d(x, y).size >= 1, (c, name)
        check_set(pset, labels, firsts, wrap, "ties")
    finally:
        pset.close()


# ---- scenario 3: labels shared by problems ---------------------------------------------------

def random_labels(rng, n, lo, hi, longest):
    ls = rng.integers(lo, hi, n)
    return (ls.astype(np.int32), (ls + rng.integers(1, longest + 1, n)).astype(np.int32),
            rng.integers(0, 4, n).astype(np.int32))


def scenario_shared(psd, wrap):
    from peaksegdisk_amd import synthetic
    a = synthetic.poisson_coverage(2500, seed=3)[2].astype(np.int32)
    b = synthetic.poisson_coverage(400, seed=4)[2].astype(np.int32)
    pens = [0.0, 0.3, 1.0, 3.0, 10.0, 30.0, 100.0, float("inf")]
    rng = np.random.default_rng(5)
    labels = [random_labels(rng, 40, 90, 2650, 300), None]
    pset = psd.ProblemSet.from_dense([as_numpy(a), as_numpy(b)],
                                     [(0, p) for p in pens] + [(1, 2.0)])
    try:
        pset.solve()
        totals, per_label, _ = check_set(pset, labels, [100, 0], wrap, "shared")
        assert totals[8].tolist() == [0, 0, 0, 0, 0]
        assert [len(x) for x in per_label[8]] == [0, 0, 0]
        assert len({tuple(t) for t in totals[:8].tolist()}) > 1   # (the models do differ)
    finally:
        pset.close()


# ---- scenario 4: many rows per problem -------------------------------------------------------

def scenario_many_rows(psd, wrap):
    from peaksegdisk_amd import synthetic
    v = synthetic.poisson_coverage(20000, seed=9)[2].astype(np.int32)
    rng = np.random.default_rng(6)
    labels = [random_labels(rng, 2000, -100, 20100, 5000)]
    pset = psd.ProblemSet.from_dense([as_numpy(v)], [(0, 0.0)])
    try:
        pset.solve()
        totals, _, columns = check_set(pset, labels, None, wrap, "many rows")
        assert (len(columns[0][0]) - 1) // 2 >= 1000
        assert totals[0][0] > 64     # (more than a wave's worth of errors in one word)
    finally:
        pset.close()


# ---- scenario 5: waves whose 64 lanes all count for one problem -------------------------------

def full_wave_labels(ps, pe):
    """3 x 64 labels around the peaks [ps[i], pe[i]) of a model (in genomic order, at least 20 bases
    wide and 40 apart): 64 peakStart / peakEnd labels that hold two starts or two ends (false
    positives that could also have been false negatives), 64 noPeaks labels over a peak, 64 labels
    that find nothing (peaks between two peaks, peakStart and peakEnd inside one)"""
    n = len(ps)
    assert n >= 3 and np.all(pe - ps >= 20) and np.all(ps[1:] - pe[:-1] >= 40)
    rows = []
    for k in range(64):
        i, a, b = k % (n - 1), 1 + k % 7, 1 + (k // 7) % 9
        if k % 2:
            rows.append((ps[i] - a, ps[i + 1] + b, PEAK_START))
        else:
            rows.append((pe[i] - a, pe[i + 1] + b, PEAK_END))
    for k in range(64):
        i, a = k % n, k % 13
        rows.append([(ps[i] + a, ps[i] + a + 3), (ps[i] - 5, ps[i] + 1 + a), (pe[i] - 1, pe[i] + 30),
                     (ps[0] - 9, pe[n - 1] + a)][k % 4] + (NO_PEAKS,))
    for k in range(64):
        i, a = k % (n - 1), k % 11
        rows.append([(pe[i] + a, pe[i] + a + 20, PEAKS), (ps[i] + 1, ps[i] + 9 + a, PEAK_START),
                     (ps[i], ps[i] + 10 + a, PEAK_END), (pe[i], pe[i] + 25 + a, PEAK_START)][k % 4])
    cols = np.array(rows, dtype=np.int64)
    return tuple(np.ascontiguousarray(cols[:, j], dtype=np.int32) for j in range(3))


def scenario_full_waves(psd, wrap):
    """count_kernel packs a wave's four sums into the bytes of one word: here the 64 lanes of a wave
    all belong to one problem and all count, so a byte holds 64.  The second problem has the same
    labels shuffled: its waves mix the three kinds."""
    v = np.full(9000, 2, dtype=np.int32)
    for j, a in enumerate(range(500, 8500, 1000)):
        v[a:a + 300 + 20 * j] = 40 + 5 * j
    first = 700
    pset = psd.ProblemSet.from_dense([as_numpy(v), as_numpy(v)], [(0, 10.0), (1, 10.0)])
    try:
        pset.solve()
        columns = pset.segment_columns(first_chromStart=[first, first])
        ps, pe = (x[::-1] for x in peaks_of(columns[0]))
        assert len(ps) == 8 and np.array_equal(ps, first + np.arange(500, 8500, 1000))
        ordered = full_wave_labels(ps, pe)
        order = np.random.default_rng(15).permutation(len(ordered[0]))
        shuffled = tuple(np.ascontiguousarray(a[order]) for a in ordered)
        # what the scenario is for did occur, from the yardstick's columns: packed rows 0-63, 64-127
        # and 128-191 are waves of problem 0 whose lanes all count in the same bytes
        _, fp, fn, totals = brute_force(columns[0], ordered)
        codes = ordered[2]
        possible_fp, possible_fn = codes != PEAKS, codes != NO_PEAKS
        assert len(codes) == 192 and pset.problems[0][0] == 0
        assert fp[:64].all() and possible_fp[:64].all() and possible_fn[:64].all() and not fn[:64].any()
        assert fp[64:128].all() and possible_fp[64:128].all() and not possible_fn[64:128].any()
        assert fn[128:].all() and possible_fn[128:].all() and not fp[128:].any()
        assert totals == [192, 128, 64, 128 + int(np.sum(codes[128:] != PEAKS)), 128]
        mixed = brute_force(columns[1], shuffled)
        assert mixed[3] == totals and 0 < mixed[1][:64].sum() < 64
        got, _, _ = check_set(pset, [ordered, shuffled], [first, first], wrap, "full waves")
        assert got[0].tolist() == totals and got[1].tolist() == totals
    finally:
        pset.close()


# ---- scenario 6: refusals --------------------------------------------------------------------

BAD_CASES = [   # (labels of contig 1, what the text must hold)
    ("count", None, "contig 1"),
    ("null", None, "contig 1"),
    ("order", (np.array([5, 9, 30], np.int32), np.array([8, 9, 40], np.int32),
               np.array([0, 1, 2], np.int32)), "label 1"),
    ("code", (np.array([5, 9, 30], np.int32), np.array([8, 19, 40], np.int32),
              np.array([0, 1, 4], np.int32)), "label 2"),
]


def raw_pack(pset, n_labels, arrays, on_device):
    """the C entry as it is: arrays[c] = three addresses; -> its return value"""
    nc = len(n_labels)
    out = [ctypes.c_void_p() for _ in range(4)]
    cols = [(ctypes.c_void_p * nc)(*[arrays[c][j] for c in range(nc)]) for j in range(3)]
    return _lib().peakseg_hip_problem_set_pack_label_errors(
        pset._h, None, (ctypes.c_longlong * nc)(*n_labels), *cols, on_device, None,
        *[ctypes.byref(q) for q in out])


def scenario_refusals(psd, wrap, device_side):
    """device_side(array) -> (address the library may read as device memory, what keeps it alive),
    or None where there is no such memory at hand"""
    from peaksegdisk_amd import _native, synthetic
    assert _native.ERROR_LABEL_ARGUMENTS == 19
    text = _native.status_message(19, "f", "1", "d")
    assert text.startswith("error code 19") and "annotation" in text
    vectors = [synthetic.poisson_coverage(600, seed=k)[2].astype(np.int32) for k in (1, 2)]
    good = (np.array([5, 50], np.int32), np.array([8, 90], np.int32), np.array([0, 3], np.int32))
    pset = psd.ProblemSet.from_dense([as_numpy(v) for v in vectors], [(0, 1.0), (1, 1.0)])
    try:
        with pytest.raises(RuntimeError):                        # not solved
            pset.label_errors([good, good])
        assert raw_pack(pset, [0, 0], [(0, 0, 0)] * 2, 0) == -1
        pset.solve()
        stats_before = pset.segment_stats()
        sides = [0] + ([1] if device_side is not None else [])
        for on_device in sides:
            def address(a):
                if not on_device:
                    return a.ctypes.data, a
                return device_side(a)
            keep = [address(a) for a in good]
            for name, entry, needle in BAD_CASES:
                if name == "count":
                    st = raw_pack(pset, [2, -1], [[k[0] for k in keep], (0, 0, 0)], on_device)
                elif name == "null":
                    st = raw_pack(pset, [2, 2], [[k[0] for k in keep], (keep[0][0], 0, keep[2][0])],
                                  on_device)
                else:
                    bad = [address(a) for a in entry]
                    st = raw_pack(pset, [2, 3], [[k[0] for k in keep], [k[0] for k in bad]],
                                  on_device)
                message = _lib().peakseg_hip_last_error().decode()
                assert st == -19, (name, on_device, st, message)
                assert "contig 1" in message and needle in message, (name, on_device, message)
                out = [np.zeros(8, np.int32) for _ in range(3)]   # nothing packed: no old numbers
                assert _lib().peakseg_hip_problem_set_packed_label_errors_download(
                    pset._h, *[a.ctypes.data for a in out], None) == -1
            if on_device:   # an address that is no multiple of 4
                st = raw_pack(pset, [2, 0], [(keep[0][0] + 2, keep[1][0], keep[2][0]), (0, 0, 0)], 1)
                assert st == -19 and "multiple of 4" in _lib().peakseg_hip_last_error().decode()
        # the Python entry names the status, and its own checks the annotation
        with pytest.raises(RuntimeError, match="label 1") as ei:
            pset.label_errors(wrap_labels([good, BAD_CASES[2][1]], wrap))
        assert ei.value.status == 19
        with pytest.raises(ValueError, match="label 1"):
            pset.label_errors([good, (good[0], good[1], ["noPeaks", "peak"])])
        # after the refusals the set still answers
        stats_after = pset.segment_stats()
        assert all(np.array_equal(x, y) for x, y in zip(stats_before[0], stats_after[0]))
        check_set(pset, [good, (good[0], good[1], np.array([1, 2], np.int32))], None, wrap, "after")
        totals, _ = pset.label_errors([good, (good[0], good[1], ["peakStart", "peakEnd"])])
        assert totals[1].tolist()[3:] == [2, 2]
        ms = ctypes.c_float(-1.0)
        assert _lib().peakseg_hip_label_errors_last_ms(ctypes.byref(ms)) == 0 and ms.value >= 0.0
    finally:
        pset.close()
    count, weight, _ = rle(vectors[1])
    plain = psd.ProblemSet([(count, weight)], [(0, 1.0)])
    try:
        plain.solve()
        with pytest.raises(RuntimeError, match="dense"):
            plain.label_errors([good])
    finally:
        plain.close()


# ---- scenario 7: the torch_device form (GPU only) --------------------------------------------

def scenario_torch_device(psd, wrap):
    """the tensors alias the packed buffers and hold what the download returns"""
    import torch
    dense = mono27ac_dense()
    labels = wrap_labels([golden_labels()[0]], wrap)
    pset = psd.ProblemSet.from_dense([as_numpy(dense)], [(0, 1952.6), (0, 0.0)])
    try:
        pset.solve()
        totals, per_label = pset.label_errors(labels, first_chromStart=[60000])
        offs, t_count, t_fp, t_fn, t_totals = pset.label_errors(
            labels, first_chromStart=[60000], torch_device="cuda:0")
        assert offs.tolist() == [0, 6, 12]
        assert [t.dtype for t in (t_count, t_fp, t_fn, t_totals)] == [torch.int32] * 4
        assert t_count.device.type == "cuda" and tuple(t_totals.shape) == (2, 5)
        kept = [t.cpu().numpy() for t in (t_count, t_fp, t_fn)]
        kept_totals = t_totals.cpu().numpy()
        addresses = [t.data_ptr() for t in (t_count, t_fp, t_fn, t_totals)]
        again = pset.label_errors(labels, first_chromStart=[60000], torch_device="cuda:0")
        assert [t.data_ptr() for t in again[1:]] == addresses     # the library's own buffers
    finally:
        pset.close()
    assert np.array_equal(kept_totals, totals)
    for k in (0, 1):
        for got, want in zip(kept, per_label[k]):
            assert np.array_equal(got[int(offs[k]):int(offs[k + 1])], want)


# ---- scenario 8: PeakSegFPOP_dense(..., labels=...) ------------------------------------------

def scenario_api(psd, wrap):
    dense = mono27ac_dense()
    labels, _ = golden_labels()
    pens = [0, 1952.6, 10000, float("inf")]
    names = [["noPeaks", "peakStart", "peakEnd", "peaks"][a] for a in labels[2]]
    bare = psd.PeakSegFPOP_dense(as_numpy(dense), pens, chrom="chr11", chrom_starts=[60000])
    fits = psd.PeakSegFPOP_dense(as_numpy(dense), pens, chrom="chr11", chrom_starts=[60000],
                                 labels=(labels[0], labels[1], names))
    assert len(fits) == len(bare) == 4
    for fit, plain in zip(fits, bare):
        assert not hasattr(plain, "label_errors")
        assert sorted(vars(plain)) == ["classes", "data", "loss", "others", "segments"]
        assert sorted(vars(fit)) == sorted(set(vars(plain)) | {"label_errors"})
        assert fit.segments.equals(plain.segments)
        assert list(plain.loss.columns) == psd.col_name_list["loss"] + ["megabytes", "seconds"]
        keep = [n for n in plain.loss.columns if n != "seconds"]
        assert fit.loss[keep].equals(plain.loss[keep])
        assert list(fit.loss.columns) == list(plain.loss.columns) + [
            "errors", "fp", "fn", "possible.fp", "possible.fn"]
        frame = fit.label_errors
        assert list(frame.columns) == ["chrom", "chromStart", "chromEnd", "annotation", "count",
                                       "fp", "fn", "status"]
        assert frame["annotation"].tolist() == names and set(frame["chrom"]) == {"chr11"}
        want = brute_force((fit.segments["chromStart"].to_numpy(), fit.segments["chromEnd"].to_numpy()),
                           labels)
        for name, w in zip(("count", "fp", "fn"), want[:3]):
            assert frame[name].tolist() == w.tolist(), name
        assert frame["status"].tolist() == [
            "false positive" if p else "false negative" if n else "correct"
            for p, n in zip(want[1].tolist(), want[2].tolist())]
        assert fit.loss[["errors", "fp", "fn", "possible.fp", "possible.fn"]].iloc[0].tolist() == want[3]
    assert fits[3].label_errors["status"].tolist() == [
        "correct", "false negative", "false negative", "correct", "correct", "correct"]
    assert "false positive" in fits[0].label_errors["status"].tolist()


SCENARIOS = [scenario_mono27ac, scenario_ties, scenario_shared, scenario_many_rows,
             scenario_full_waves, scenario_api]


# ---- MI355X ----------------------------------------------------------------------------------

def cuda_side(a):
    t = as_cuda(a)
    return t.data_ptr(), t


_CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process
sys.path[:0] = [%(root)r, %(tests)r]
import test_gpu_label_errors as gl
gl.child_main()
print("labels-child ok")
"""


def child_main():
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd as psd
    for scenario in SCENARIOS:
        scenario(psd, as_cuda)
    scenario_refusals(psd, as_cuda, cuda_side)
    scenario_torch_device(psd, as_cuda)
    scenario_torch_device(psd, as_numpy)


@GPU
@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__[len("scenario_"):])
def test_gpu_label_errors_numpy(psd, scenario):
    scenario(psd, as_numpy)


@GPU
def test_gpu_label_errors_refusals_host_arrays(psd):
    scenario_refusals(psd, as_numpy, None)


@GPU
def test_gpu_label_errors_cuda_tensors(psd):
    """every scenario again with the labels in cuda tensors, the refusals of device arrays, and the
    torch_device form of label_errors()"""
    import sys
    from conftest import ROOT
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(p.stdout[-4000:])
    assert p.returncode == 0 and "labels-child ok" in p.stdout, p.stdout[-3000:] + p.stderr[-6000:]
