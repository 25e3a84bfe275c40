"""ProblemSet.coverage_order_statistics / coverage_moments / coverage_quantiles / coverage_features
and the learned-penalty path of PeakSegFPOP_dense / PeakSegFPOP_reads: order statistics and moments
of every contig's per-base coverage, selected and summed on the device from the resident runs.

The scenario functions are shared with the emulator rehearsal (tests/test_coverage_features_emu.py),
which runs them without a GPU on host arrays; the tests marked gpu run them on the MI355X with the
coverage once as numpy arrays (in this process) and once as cuda tensors (in a child process that
imports torch first, as tests/test_gpu_label_errors.py does).

The yardstick never comes from the library: np.sort, np.quantile and Python integers on the
EXPANDED per-base vector.  All comparisons are for equality -- integers and the quartile features
bit for bit, mean and sd against the exact quotient of Python integers rounded once -- but
np.std(ddof=1), whose own summation rounds: 1e-9 relative."""
import ctypes
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_gpu_dense import as_cuda, as_numpy, mono27ac_dense, rle
from test_gpu_label_errors import golden_labels
from test_gpu_reads import fixture_reads, numpy_pileup

GPU = pytest.mark.gpu
BASE = ["quartile.0%", "quartile.25%", "quartile.50%", "quartile.75%", "quartile.100%", "mean", "sd",
        "bases", "data"]
NAMES = BASE + ["log+1." + n for n in BASE] + ["log." + n for n in BASE] + ["log.log." + n for n in BASE]
SHORT, LONG = 1, 4     # digit passes: counts below 256, full-range counts


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


def last_passes():
    n = ctypes.c_int(-1)
    assert _lib().peakseg_hip_coverage_stats_last_passes(ctypes.byref(n)) == 0
    return n.value


# ---- the yardstick ---------------------------------------------------------------------------

def yard_moments(x):
    """(bases, runs, sum, sum of squares) of the expanded vector, Python integers"""
    values, times = np.unique(np.asarray(x, np.int64), return_counts=True)
    s1 = sum(int(v) * int(t) for v, t in zip(values.tolist(), times.tolist()))
    s2 = sum(int(v) * int(v) * int(t) for v, t in zip(values.tolist(), times.tolist()))
    return len(x), 1 + int(np.count_nonzero(np.diff(x))), s1, s2


def yard_features(x):
    x = np.asarray(x, np.int64)
    bases, runs, s1, s2 = yard_moments(x)
    sd = math.sqrt(float(Fraction(bases * s2 - s1 * s1, bases * (bases - 1)))) if bases > 1 else math.nan
    if bases > 1:   # numpy's own mean and sd round in their sums
        assert abs(sd - np.std(x.astype(np.float64), ddof=1)) <= 1e-9 * max(sd, 1e-300)
        assert abs(float(Fraction(s1, bases)) - np.mean(x)) <= 1e-9 * max(np.mean(x), 1e-300)
    base = np.array(np.quantile(x, [0, .25, .5, .75, 1]).tolist() +
                    [float(Fraction(s1, bases)), sd, float(bases), float(runs)], dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.concatenate([base, np.log(base + 1), np.log(base), np.log(np.log(base))])


def same(got, want):
    """equal bit for bit, NaN where NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64))


def check_features(pset, vectors, what):
    """coverage_features, coverage_quantiles and coverage_moments of every contig; -> the frame"""
    moments = pset.coverage_moments()
    quantiles = pset.coverage_quantiles()
    frame = pset.coverage_features()      # (the last call: what last_passes() tells of)
    assert list(frame.columns) == NAMES and len(frame) == len(vectors), what
    assert quantiles.dtype == np.float64 and quantiles.shape == (len(vectors), 5)
    assert [moments[k].dtype for k in ("bases", "runs", "sum", "sum_sq")] == [
        np.int64, np.int64, np.int64, np.dtype(object)]
    for c, x in enumerate(vectors):
        want = yard_features(x)
        got = frame.iloc[c].to_numpy(dtype=np.float64)
        bad = [NAMES[j] for j in range(len(NAMES)) if not same(got[j:j + 1], want[j:j + 1])]
        assert not bad, (what, c, bad, got[:9].tolist(), want[:9].tolist())
        assert same(quantiles[c], want[:5]), (what, c)
        assert (int(moments["bases"][c]), int(moments["runs"][c]), int(moments["sum"][c]),
                moments["sum_sq"][c]) == yard_moments(x), (what, c)
        assert type(moments["sum_sq"][c]) is int
    return frame


def check_ranks(pset, vectors, ranks, what):
    got = pset.coverage_order_statistics(ranks)
    assert got.dtype == np.int32 and got.shape == (len(vectors), len(ranks[0])), what
    for c, x in enumerate(vectors):
        want = np.sort(np.asarray(x, np.int64))[np.asarray(ranks[c], np.int64)]
        assert got[c].tolist() == want.tolist(), (what, c, list(ranks[c]), got[c].tolist(), want.tolist())
    return got


def make_set(psd, vectors, wrap, problems=None):
    if problems is None:
        problems = [(c, float("inf")) for c in range(len(vectors))]
    return psd.ProblemSet.from_dense([wrap(v) for v in vectors], problems)


# ---- scenario 1: known data -------------------------------------------------------------------

def scenario_known(psd, wrap):
    example = np.array([1, 3, 0, 4, 2], np.int32)
    dense = mono27ac_dense()
    assert len(rle(dense)[0]) == 6921 and len(dense) == 520000 and int(dense.max()) == 42
    pset = make_set(psd, [example, dense], wrap)
    try:
        frame = check_features(pset, [example, dense], "known")
        assert last_passes() == SHORT
        assert frame.iloc[0][BASE].tolist() == [0, 1, 2, 3, 4, 2, math.sqrt(2.5), 5, 5]
        ms = ctypes.c_float(-1.0)
        assert _lib().peakseg_hip_coverage_stats_last_ms(ctypes.byref(ms)) == 0 and ms.value >= 0.0
        pset.coverage_moments()
        assert last_passes() == 0       # moments only: no digit pass
    finally:
        pset.close()


# ---- scenario 2: tile edges -------------------------------------------------------------------

def distinct_neighbours(rng, n, top):
    """n counts below `top`, neighbours different"""
    c = rng.integers(0, top, n).astype(np.int64)
    for i in range(1, n):
        if c[i] == c[i - 1]:
            c[i] = (c[i] + 1) % top
    return c


def edge_ranks(bases):
    from peaksegdisk_amd.grid import quartile_ranks
    lo, hi, _ = quartile_ranks(bases)
    extra = [min(max(r, 0), bases - 1) for r in (0, 1, bases - 2, bases - 1)]
    return lo + hi + extra


def scenario_tile_edges(psd, wrap):
    T = _lib().peakseg_hip_coverage_stats_tile_runs()
    assert T >= 64 and _lib().peakseg_hip_coverage_stats_max_ranks() >= 10
    rng = np.random.default_rng(2024)
    runs = [1, 2, 3, T - 1, T, T + 1, 2 * T + 3]
    vectors = []
    for k, r in enumerate(runs):
        counts = distinct_neighbours(rng, r, 70000 if k % 2 else 200)
        vectors.append(np.repeat(counts, rng.choice([1, 2, 7], r)).astype(np.int32))
        assert len(rle(vectors[-1])[0]) == r
    offsets = np.concatenate([[0], np.cumsum(runs)])[:-1]
    assert (offsets % 4).tolist() == [0, 1, 3, 2, 1, 1, 2]
    pset = make_set(psd, vectors, wrap)
    try:
        check_ranks(pset, vectors, [edge_ranks(len(v)) for v in vectors], "tile edges")
        assert last_passes() == 3
        check_features(pset, vectors, "tile edges")
    finally:
        pset.close()


# ---- scenario 3: cumulative boundaries over every digit ---------------------------------------

def scenario_boundaries(psd, wrap):
    values = [0, 1, 255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24, 2 ** 31 - 1]
    rng = np.random.default_rng(7)
    order = rng.permutation(len(values))
    weights = rng.integers(5, 10, len(values))
    weights[order.tolist().index(len(values) - 1)] = 5
    x = np.repeat(np.array(values, np.int64)[order], weights).astype(np.int32)
    srt = np.sort(x.astype(np.int64))
    ranks = []
    for v in values:
        w = int(np.count_nonzero(srt <= v))       # cumulative weight
        ranks += [w - 1] + ([w] if w < len(x) else [])
    assert len(ranks) == 2 * len(values) - 1
    pset = make_set(psd, [x], wrap)
    try:
        got = check_ranks(pset, [x], [ranks], "boundaries")     # (17 ranks: two calls)
        assert last_passes() == LONG
        assert sorted(set(got[0].tolist())) == values
        check_features(pset, [x], "boundaries")
        sum_sq = pset.coverage_moments()["sum_sq"][0]
        assert sum_sq >> 64 != 0
    finally:
        pset.close()


# ---- scenario 4: many contigs -----------------------------------------------------------------

def scenario_many_contigs(psd, wrap):
    T = _lib().peakseg_hip_coverage_stats_tile_runs()
    rng = np.random.default_rng(99)
    vectors = []
    for k in range(302):
        if k == 150:
            counts = distinct_neighbours(rng, 3 * T + 1, 300)
            weights = rng.integers(1, 4, 3 * T + 1)
        elif k == 200:
            counts, weights = np.array([6]), np.array([9])          # all equal: a single run
        else:
            r = int(rng.integers(1, 6))
            counts = distinct_neighbours(rng, r, int(rng.choice([5, 300, 2 ** 31])))
            weights = rng.integers(1, 6, r)
        vectors.append(np.repeat(counts, weights).astype(np.int32))
    # two problems on some contigs, none on others: the problems play no part
    problems = [(c, p) for c in range(0, 302, 3) for p in (1.0, float("inf"))]
    ranks = np.array([rng.integers(0, len(v), 3) for v in vectors], dtype=np.int64)
    pset = make_set(psd, vectors, wrap, problems)
    try:
        check_ranks(pset, vectors, ranks.tolist(), "many contigs")
        assert last_passes() == LONG
        check_features(pset, vectors, "many contigs")
        # one row of ranks for all contigs
        got = pset.coverage_order_statistics([0])
        assert got[:, 0].tolist() == [int(v.min()) for v in vectors]
    finally:
        pset.close()


# ---- scenario 5: reads ------------------------------------------------------------------------

def scenario_reads(psd, wrap):
    start, end, count = fixture_reads()
    table = psd.coverage_from_reads(as_numpy(start), as_numpy(end), as_numpy(count))
    dense = np.repeat(table["count"].to_numpy(), (table["chromEnd"] - table["chromStart"]).to_numpy())
    dense = dense.astype(np.int32)
    lo, hi = int(start.min()), int(end.max())
    assert np.array_equal(dense, numpy_pileup(start, end, count, lo, hi))
    reads = [tuple(wrap(a) for a in (start, end, count))]
    from_reads = psd.ProblemSet.from_reads(reads, [(0, float("inf"))])
    from_dense = make_set(psd, [dense], wrap)
    try:
        a = check_features(from_reads, [dense], "reads")
        b = from_dense.coverage_features()
        assert same(a.to_numpy(), b.to_numpy())
    finally:
        from_reads.close()
        from_dense.close()
    assert same(psd.problem_features_reads(reads[0]).to_numpy(), a.to_numpy())
    assert same(psd.problem_features_dense(wrap(dense)).to_numpy(), a.to_numpy())


# ---- scenario 6: a solve is not disturbed -----------------------------------------------------

def scenario_solve_undisturbed(psd, wrap):
    dense = mono27ac_dense()
    labels = [golden_labels()[0]]
    problems = [(0, 0.0), (0, 1952.6)]
    with_features = make_set(psd, [dense], wrap, problems)
    without = make_set(psd, [dense], wrap, problems)
    try:
        before = with_features.coverage_features()
        with_features.solve()
        without.solve()
        between = with_features.coverage_features()
        assert same(before.to_numpy(), between.to_numpy())
        assert same(before.iloc[0].to_numpy(), yard_features(dense))
        tables = []
        for pset in (with_features, without):
            columns = pset.segment_columns(first_chromStart=[60000])
            if pset is with_features:
                pset.coverage_order_statistics([0, 5, 519999])
            stats = pset.segment_stats(first_chromStart=[60000])
            if pset is with_features:
                pset.coverage_moments()
            totals, per_label = pset.label_errors(labels, first_chromStart=[60000])
            tables.append((columns, stats, totals, per_label,
                           [pset.loss(p) for p in range(2)], [pset.segments(p) for p in range(2)]))
        a, b = tables
        for p in range(2):
            for k in (0, 1, 3, 5):
                assert all(np.array_equal(x, y) for x, y in zip(a[k][p], b[k][p])), (p, k)
            assert np.array_equal(a[4][p], b[4][p])
        assert np.array_equal(a[2], b[2])
        assert len(a[0][0][0]) > len(a[0][1][0]) > 1
    finally:
        with_features.close()
        without.close()


# ---- scenario 7: refusals ---------------------------------------------------------------------

def raw_pack(pset, n_ranks, ranks):
    ranks = np.ascontiguousarray(ranks, dtype=np.int64)
    value, moments = ctypes.c_void_p(), ctypes.c_void_p()
    return _lib().peakseg_hip_problem_set_pack_coverage_stats(
        pset._h, n_ranks, ranks.ctypes.data, ctypes.byref(value), ctypes.byref(moments))


def scenario_refusals(psd, wrap):
    from peaksegdisk_amd import _native
    assert _native.ERROR_FEATURE_ARGUMENTS == 20
    text = _native.status_message(20, "f", "1", "d")
    assert text.startswith("error code 20") and "rank" in text
    rng = np.random.default_rng(3)
    vectors = [rng.integers(0, 9, n).astype(np.int32) for n in (40, 25)]
    most = _lib().peakseg_hip_coverage_stats_max_ranks()
    pset = make_set(psd, vectors, wrap)
    try:
        good = [[0, 39, 20], [24, 0, 7]]
        for bad, needle in (([[0, 39, 20], [24, -1, 7]], "rank -1"),
                            ([[0, 39, 20], [24, 25, 7]], "rank 25"),
                            ([[0, 40, 20], [24, 0, 7]], "rank 40")):
            with pytest.raises(RuntimeError) as ei:
                pset.coverage_order_statistics(bad)
            assert ei.value.status == 20, ei.value
            contig = "contig 1" if needle != "rank 40" else "contig 0"
            assert contig in str(ei.value) and needle in str(ei.value), str(ei.value)
            assert raw_pack(pset, 3, bad) == -20
            # nothing packed: no old numbers
            out = np.zeros(6, np.int32)
            assert _lib().peakseg_hip_problem_set_packed_coverage_stats_download(
                pset._h, out.ctypes.data, None) == -1
            check_ranks(pset, vectors, good, "after " + needle)
        for n_ranks in (most + 1, -1):
            assert raw_pack(pset, n_ranks, np.zeros((2, most + 1), np.int64)) == -20
            assert "ranks" in _lib().peakseg_hip_last_error().decode()
            check_ranks(pset, vectors, good, "after n_ranks %d" % n_ranks)
        assert raw_pack(pset, most, np.zeros((2, most), np.int64)) == 2 * most
        with pytest.raises(ValueError):
            pset.coverage_quantiles([0.5, float("nan")])
        with pytest.raises(ValueError):
            pset.coverage_quantiles([1.5])
        with pytest.raises(ValueError):
            pset.coverage_quantiles([-0.1])
        check_features(pset, vectors, "after the refusals")
        # a prob that is no multiple of 1/4: the definition in floating point
        q = pset.coverage_quantiles([0.1, 0.9])
        for c, v in enumerate(vectors):
            srt = np.sort(v).astype(np.float64)
            for j, p in enumerate((0.1, 0.9)):
                h = (len(v) - 1) * p
                lo = int(math.floor(h))
                assert q[c, j] == srt[lo] + (srt[min(lo + 1, len(v) - 1)] - srt[lo]) * (h - lo)
    finally:
        pset.close()
    count, weight, _ = rle(vectors[1])
    plain = psd.ProblemSet([(count, weight)], [(0, 1.0)])
    try:
        assert raw_pack(plain, 1, np.zeros((1, 1), np.int64)) == -1
        assert "dense" in _lib().peakseg_hip_last_error().decode()
        for call in (plain.coverage_features, plain.coverage_moments,
                     lambda: plain.coverage_order_statistics([0])):
            with pytest.raises(RuntimeError, match="dense"):
                call()
    finally:
        plain.close()


# ---- scenario 8: the learned penalty, end to end ----------------------------------------------

MODEL = {"intercept": 0.5, "weights": {"log.log.bases": 1.0, "log+1.quartile.75%": 0.7, "log.mean": -0.5}}


def yard_frame(vectors):
    import pandas as pd
    return pd.DataFrame(np.array([yard_features(v) for v in vectors]), columns=NAMES)


def same_fit(a, b):
    assert a.segments.equals(b.segments)
    keep = [n for n in a.loss.columns if n != "seconds"]
    assert list(a.loss.columns) == list(b.loss.columns) and a.loss[keep].equals(b.loss[keep])
    assert a.stats.equals(b.stats)


def scenario_learned_penalty(psd, wrap, n=1500):
    from peaksegdisk_amd import synthetic
    vectors = [synthetic.poisson_coverage(n + 37 * k, seed=40 + k)[2].astype(np.int32) for k in range(3)]
    assert any(int(v.min()) == 0 for v in vectors)
    wanted = yard_frame(vectors)
    predicted = psd.predict_penalties(wanted, MODEL)
    assert len(set(predicted.tolist())) == 3 and all(0 < p < math.inf for p in predicted)
    assert [float(psd.paste(float(p))) for p in predicted] == predicted.tolist()
    fits = psd.PeakSegFPOP_dense([wrap(v) for v in vectors], penalty_model=MODEL, stats=True)
    by_hand = psd.PeakSegFPOP_dense([wrap(v) for v in vectors], [[float(p)] for p in predicted],
                                    stats=True)
    assert [len(f) for f in fits] == [1, 1, 1] == [len(f) for f in by_hand]
    for c in range(3):
        same_fit(fits[c][0], by_hand[c][0])
        assert float(fits[c][0].loss["penalty"].iloc[0]) == predicted[c]
        assert list(fits[c][0].features.index) == NAMES
        assert same(fits[c][0].features.to_numpy(dtype=np.float64), wanted.iloc[c].to_numpy())
        assert not hasattr(by_hand[c][0], "features")
    assert any(int(f[0].loss["peaks"].iloc[0]) >= 1 for f in fits)
    # a single vector: a list of one result
    one = psd.PeakSegFPOP_dense(wrap(vectors[1]), penalty_model=MODEL, stats=True)
    assert len(one) == 1
    same_fit(one[0], by_hand[1][0])
    # a feature that is -inf where a vector has a zero base
    with pytest.raises(ValueError) as ei:
        psd.PeakSegFPOP_dense([wrap(v) for v in vectors],
                              penalty_model={"intercept": 0.0, "weights": {"log.quartile.0%": 1.0}})
    assert "log.quartile.0%" in str(ei.value) and "contig" in str(ei.value)
    # once through the reads
    rng = np.random.default_rng(8)
    starts = rng.integers(100, 100 + n, 300).astype(np.int32)
    ends = (starts + rng.integers(20, 120, 300)).astype(np.int32)
    coverage = numpy_pileup(starts, ends, None, int(starts.min()), int(ends.max()))
    p = psd.predict_penalties(yard_frame([coverage]), MODEL)
    reads = (wrap(starts), wrap(ends))
    fit = psd.PeakSegFPOP_reads(reads, penalty_model=MODEL, stats=True)
    hand = psd.PeakSegFPOP_reads(reads, [float(p[0])], stats=True)
    assert len(fit) == 1 == len(hand)
    same_fit(fit[0], hand[0])
    assert same(fit[0].features.to_numpy(dtype=np.float64), yard_features(coverage))


SCENARIOS = [scenario_known, scenario_tile_edges, scenario_boundaries, scenario_many_contigs,
             scenario_reads, scenario_solve_undisturbed, scenario_refusals, scenario_learned_penalty]


# ---- the torch_device form (GPU only) ---------------------------------------------------------

def scenario_torch_device(psd, wrap):
    """the tensor aliases the library's buffer and holds what the download returns"""
    import torch
    vectors = [np.array([1, 3, 0, 4, 2], np.int32), np.array([9, 9, 2, 70000], np.int32)]
    pset = make_set(psd, vectors, wrap)
    try:
        ranks = [[0, 2, 4], [3, 0, 1]]
        host = check_ranks(pset, vectors, ranks, "torch_device")
        t = pset.coverage_order_statistics(ranks, torch_device="cuda:0")
        assert t.dtype == torch.int32 and t.device.type == "cuda" and tuple(t.shape) == (2, 3)
        kept, address = t.cpu().numpy(), t.data_ptr()
        again = pset.coverage_order_statistics(ranks, torch_device="cuda:0")
        assert again.data_ptr() == address        # the library's own buffer
    finally:
        pset.close()
    assert np.array_equal(kept, host)


# ---- MI355X ----------------------------------------------------------------------------------

_CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process
sys.path[:0] = [%(root)r, %(tests)r]
import test_gpu_coverage_features as cf
cf.child_main()
print("features-child ok")
"""


def child_main():
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd as psd
    for scenario in SCENARIOS:
        scenario(psd, as_cuda)
    scenario_torch_device(psd, as_cuda)
    scenario_torch_device(psd, as_numpy)


@GPU
@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__[len("scenario_"):])
def test_gpu_coverage_features_numpy(psd, scenario):
    scenario(psd, as_numpy)


@GPU
def test_gpu_coverage_features_cuda_tensors(psd):
    """every scenario again with the coverage in cuda tensors, and the torch_device form of
    coverage_order_statistics()"""
    import sys
    from conftest import ROOT
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(p.stdout[-4000:])
    assert p.returncode == 0 and "features-child ok" in p.stdout, p.stdout[-3000:] + p.stderr[-6000:]
