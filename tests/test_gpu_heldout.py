"""ProblemSet.heldout_loss: the Poisson loss of a solved model on another contig of the same set.

The scenario functions are shared with the emulator rehearsal (tests/test_heldout_emu.py).  The
yardstick is tests/heldout_ref.py: plain loops over Python integers, math.log and math.fsum, with a
tolerance derived from the order of the device's additions; bases, sum, rows and zero_mean_rows are
integers and are compared for equality.  Every device call is made twice and must give the same
bytes.  Contigs stay below about 4000 bases.

A PeakSeg model has an odd number of rows (2 peaks + 1), so the row counts around the reduce's
one-trip size of 256 are 255 and 257 (one and two trips of a thread), and 511 and 513."""
import ctypes
import os

import numpy as np
import pytest

from heldout_ref import heldout_pair_ref
from test_gpu_dense import REL_TOL, as_cuda, as_numpy

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


def wrap_pairs(wrap, problem, contig, scale):
    """the pairs where the contigs are: numpy arrays, or cuda tensors that are read in place"""
    problem = np.ascontiguousarray(problem, dtype=np.int32)
    contig = np.ascontiguousarray(contig, dtype=np.int32)
    scale = np.ascontiguousarray(scale, dtype=np.float64)
    if wrap is as_numpy:
        return problem, contig, scale
    import torch
    return tuple(torch.from_numpy(a).to("cuda:0") for a in (problem, contig, scale))


def poisson_vector(n, spans, seed, background=0.5):
    """n per-base Poisson counts: rate `background`, and `rate` on every (start, end, rate) of
    spans; from the library's own counter-based stream, so a seed names the same data everywhere"""
    from peaksegdisk_amd import synthetic
    lam = np.full(n, background, dtype=np.float64)
    for s, e, rate in spans:
        lam[s:e] = rate
    return synthetic.poisson_from_uniform(lam, synthetic.uniform01(seed, 3, n)).astype(np.int32)


def steps(n, spans, background=1):
    v = np.full(n, background, dtype=np.int32)
    for s, e, value in spans:
        v[s:e] = value
    return v


def score(pset, vectors, wrap, problem, contig, scale):
    """heldout_loss twice (the same bytes), the timer, every pair against the yardstick, and the
    segments tables untouched by the call -> the columns"""
    before = pset.segment_columns()
    out = pset.heldout_loss(wrap_pairs(wrap, problem, contig, scale))
    again = pset.heldout_loss(wrap_pairs(wrap, problem, contig, scale))
    ms = ctypes.c_float(-1.0)
    assert _lib().peakseg_hip_heldout_loss_last_ms(ctypes.byref(ms)) == 0 and ms.value >= 0.0
    assert sorted(out) == ["bases", "loss", "rows", "sum", "zero_mean_rows"]
    assert [out[k].dtype for k in ("loss", "rows", "bases", "sum", "zero_mean_rows")] == \
        [np.float64, np.int32, np.int64, np.int64, np.int32]
    for name in out:
        assert out[name].shape == (len(problem),)
        assert out[name].tobytes() == again[name].tobytes(), name
    after = pset.segment_columns()
    for a, b in zip(before, after):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    known = {}
    for i, (p, c, a) in enumerate(zip(problem, contig, scale)):
        key = (int(p), int(c), float(a))
        if key not in known:
            known[key] = heldout_pair_ref(before[int(p)], vectors[int(c)], float(a))
        ref = known[key]
        for name in ("rows", "bases", "sum", "zero_mean_rows"):
            assert int(out[name][i]) == ref[name], (i, name, int(out[name][i]), ref[name])
        if ref["zero_mean_rows"]:
            assert out["loss"][i] == INF, i
        else:
            assert abs(float(out["loss"][i]) - ref["loss"]) <= ref["tol"], \
                (i, float(out["loss"][i]), ref["loss"], ref["tol"])
    return out


def make_set(psd, wrap, vectors, problems):
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors], problems)
    pset.solve()
    return pset


# ---- the loss scenarios -------------------------------------------------------------------------

def scenario_own_contig(psd, wrap):
    """the own contig at scale 1 meets the yardstick and the total.loss of the set's loss row; scales
    0.5 and 1/3; the other contigs of the set"""
    spans = [(100, 160, 20.0), (300, 380, 12.0), (450, 470, 30.0)]
    vectors = [poisson_vector(600, spans, seed) for seed in (11, 12, 13)]
    penalties = [0.0, 3.0, 40.0, 1e5]
    pset = make_set(psd, wrap, vectors, [(0, pen) for pen in penalties])
    try:
        k = len(penalties)
        out = score(pset, vectors, wrap, list(range(k)), [0] * k, [1.0] * k)
        for p in range(k):
            loss = pset.loss(p)
            assert int(out["rows"][p]) == int(loss[1]) and int(out["bases"][p]) == 600
            assert int(out["sum"][p]) == int(vectors[0].sum())
            assert out["loss"][p] == pytest.approx(loss[6], rel=REL_TOL)
        assert int(out["rows"][0]) > int(out["rows"][2]) >= 3 and int(out["rows"][3]) == 1
        problem = [p for p in range(k) for _ in range(6)]
        contig = [c for _ in range(k) for c in (0, 1, 2, 0, 1, 2)]
        scale = [a for _ in range(k) for a in (0.5, 0.5, 0.5, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0)]
        score(pset, vectors, wrap, problem, contig, scale)
    finally:
        pset.close()


def scenario_one_row(psd, wrap):
    """a one-row model (penalty +Inf, served in closed form) on its own and on another contig"""
    vectors = [poisson_vector(300, [(100, 150, 9.0)], 21), poisson_vector(300, [(40, 90, 5.0)], 22)]
    pset = make_set(psd, wrap, vectors, [(0, INF), (1, INF)])
    try:
        out = score(pset, vectors, wrap, [0, 0, 1, 1], [0, 1, 0, 1], [1.0, 0.5, 1.0 / 3.0, 1.0])
        assert out["rows"].tolist() == [1] * 4 and out["bases"].tolist() == [300] * 4
    finally:
        pset.close()


def alternating(rows):
    """`rows` bases 1, 9, 1, 9, .. 1: at penalty 0 every base is a segment"""
    v = np.ones(rows, dtype=np.int32)
    v[1::2] = 9
    return v


def scenario_row_counts(psd, wrap):
    """models of 255, 257, 511 and 513 rows: one trip of the reduce's threads, two, and three"""
    for rows in (255, 257, 511, 513):
        other = (np.arange(rows) % 7).astype(np.int32) + 1
        vectors = [alternating(rows), other]
        pset = make_set(psd, wrap, vectors, [(0, 0.0)])
        try:
            out = score(pset, vectors, wrap, [0, 0, 0], [0, 1, 1], [1.0, 1.0, 1.0 / 3.0])
            assert out["rows"].tolist() == [rows] * 3
        finally:
            pset.close()


def scenario_run_counts(psd, wrap):
    """the peak segment of the model meets 16, 17, tile_runs and tile_runs + 1 runs of the held-out
    contig (the fold's line between a thread's region and a work item, one tile and two); the
    contigs' first runs are no multiples of 4 in the set's arrays (contig 0 has three runs)"""
    tile = _lib().peakseg_hip_region_stats_tile_runs()
    assert tile == 1024
    n, s, e = 1500, 150, 150 + tile + 100
    counts = (16, 17, tile, tile + 1)
    vectors = [steps(n, [(s, e, 40)])]
    for runs in counts:
        v = np.full(n, 7, dtype=np.int32)
        v[s:s + runs - 1:2] = 3
        v[s + 1:s + runs - 1:2] = 5
        v[s + runs - 1:e] = 9
        assert int(np.count_nonzero(np.diff(v[s:e]))) + 1 == runs and v[s - 1] != v[s] and v[e - 1] != v[e]
        vectors.append(v)
    pset = make_set(psd, wrap, vectors, [(0, 100.0)])
    try:
        cols = pset.segment_columns()[0]
        assert cols[0].tolist() == [e, s, 0] and cols[1].tolist() == [n, e, s]
        score(pset, vectors, wrap, [0] * 5, [0, 1, 2, 3, 4], [1.0, 0.5, 1.0, 1.0 / 3.0, 1.0])
        score(pset, vectors, wrap, [0] * 4, [4, 3, 2, 1], [1.0] * 4)
    finally:
        pset.close()


def scenario_pair_counts(psd, wrap):
    """1, 256 and 257 pairs (one workgroup of the pairs' scan, and two); pairs repeated and in any
    order"""
    spans = [(60, 90, 15.0), (200, 230, 8.0)]
    vectors = [poisson_vector(300, spans, seed) for seed in (31, 32, 33)]
    problems = [(0, 0.0), (0, 6.0), (1, 2.0), (2, INF), (1, 60.0)]
    pset = make_set(psd, wrap, vectors, problems)
    try:
        for n in (1, 256, 257):
            i = np.arange(n)
            problem = ((i * 7 + 3) % len(problems)).tolist()
            contig = ((i * 5 + 1) % 3).tolist()
            scale = [(1.0, 0.5, 1.0 / 3.0)[j % 3] for j in range(n)]
            out = score(pset, vectors, wrap, problem, contig, scale)
            if n > 1:
                same = [j for j in range(n) if (problem[j], contig[j], scale[j]) ==
                        (problem[0], contig[0], scale[0])]
                assert len(same) > 1
                assert len({out["loss"][j].tobytes() for j in same}) == 1
        out = pset.heldout_loss(wrap_pairs(wrap, [], [], []))
        assert all(len(out[name]) == 0 for name in out)
    finally:
        pset.close()


def scenario_zero_segment(psd, wrap):
    """an all-zero segment: scored where the held-out contig has no reads either its term is 0 and
    no logarithm is taken; where it has reads the loss is +Inf and zero_mean_rows is 1"""
    train = steps(300, [(100, 200, 20)], background=0)
    quiet = steps(300, [(120, 180, 6)], background=0)
    loud = quiet.copy()
    loud[50] = 1
    vectors = [train, quiet, loud]
    pset = make_set(psd, wrap, vectors, [(0, 10.0)])
    try:
        cols = pset.segment_columns()[0]
        assert cols[2][0] == 0.0 and cols[2][2] == 0.0 and cols[2][1] > 19.0
        out = score(pset, vectors, wrap, [0, 0, 0], [0, 1, 2], [1.0, 0.5, 0.5])
        assert out["zero_mean_rows"].tolist() == [0, 0, 1]
        assert np.isfinite(out["loss"][:2]).all() and out["loss"][2] == INF
        assert out["sum"].tolist() == [2000, 360, 361]
    finally:
        pset.close()


def refused(pset, wrap, problem, contig, scale, text, status=23):
    with pytest.raises(RuntimeError, match=text) as ei:
        pset.heldout_loss(wrap_pairs(wrap, problem, contig, scale))
    assert ei.value.status == status


def scenario_refusals(psd, wrap):
    """every refusal with its status and the pair it names; a set that is not solved, and one that
    was not made from dense counts; buffers that do not fit: status 14 and nothing allocated"""
    from peaksegdisk_amd import _native
    assert _native.ERROR_HELDOUT_ARGUMENTS == 23
    vectors = [steps(200, [(50, 90, 12)]), steps(200, [(60, 80, 5)]), steps(150, [(60, 80, 5)])]
    problems = [(0, INF), (2, INF)]
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors], problems)
    try:
        with pytest.raises(RuntimeError, match="not solved") as ei:
            pset.heldout_loss(wrap_pairs(wrap, [0], [0], [1.0]))
        assert ei.value.status == _native.ERROR_DEVICE_SOLVER
        pset.solve()
        good = ([0, 0, 1], [0, 1, 2], [1.0, 0.5, 1.0])
        score(pset, vectors, wrap, *good)
        room = pset.hbm_bytes
        refused(pset, wrap, [0, 0, 2], [0, 1, 0], [1.0] * 3, "pair 2")
        refused(pset, wrap, [0, -1, 0], [0, 1, 0], [1.0] * 3, "pair 1")
        refused(pset, wrap, [0, 0, 0], [0, 1, 3], [1.0] * 3, "pair 2")
        refused(pset, wrap, [0, 0, 0], [-1, 1, 0], [1.0] * 3, "pair 0")
        for bad in (0.0, -1.0, INF, float("nan")):
            refused(pset, wrap, [0, 0, 0], [0, 1, 0], [1.0, bad, 1.0], "pair 1")
        refused(pset, wrap, [0, 0, 0], [0, 1, 2], [1.0] * 3, "pair 2")      # 150 bases against 200
        refused(pset, wrap, [1, 0, 0], [1, 1, 0], [1.0] * 3, "pair 0")
        # the first bad pair is the one named
        refused(pset, wrap, [0, 5, 0, 0], [0, 0, 9, 0], [1.0, 1.0, 1.0, -2.0], "pair 1")
        none = [ctypes.byref(ctypes.c_void_p()) for _ in range(5)]
        a = np.zeros(1, np.int32)
        x = np.ones(1, np.float64)
        assert pset._lib.peakseg_hip_problem_set_pack_heldout_loss(
            pset._h, -1, a.ctypes.data, a.ctypes.data, x.ctypes.data, 0, *none) == -23
        assert "-1 pairs" in pset._lib.peakseg_hip_last_error().decode()
        assert pset._lib.peakseg_hip_problem_set_pack_heldout_loss(
            pset._h, 1, None, a.ctypes.data, x.ctypes.data, 0, *none) == -23
        assert pset._lib.peakseg_hip_problem_set_packed_heldout_loss_download(
            pset._h, None, None, None, None, None) == -1      # nothing is packed after a refusal
        # host arrays are refused before anything is allocated; device arrays are checked by the
        # first launch, which needs the pairs' columns (the call of four pairs grew them)
        assert pset.hbm_bytes == room if wrap is as_numpy else pset.hbm_bytes >= room
        score(pset, vectors, wrap, *good)
    finally:
        pset.close()
    count = np.array([1, 5, 1], dtype=np.int32)
    plain = psd.ProblemSet([(count, np.array([10, 10, 10], dtype=np.int32))], [(0, 1.0)])
    try:
        plain.solve()
        with pytest.raises(RuntimeError, match="dense") as ei:
            plain.heldout_loss(wrap_pairs(wrap, [0], [0], [1.0]))
        assert ei.value.status == _native.ERROR_DEVICE_SOLVER
    finally:
        plain.close()
    # buffers that do not fit: the same set again, allowed 8 bytes less than everything it held
    # after its buffers were there: status 14, and nothing was allocated
    os.environ["PEAKSEG_HIP_MAX_BYTES"] = str(room - 8)
    try:
        capped = psd.ProblemSet.from_dense([as_numpy(v) for v in vectors], problems)
    finally:
        del os.environ["PEAKSEG_HIP_MAX_BYTES"]
    try:
        capped.solve()
        capped.segment_columns()         # (score() packed the segments tables of the first set too)
        before = capped.hbm_bytes
        with pytest.raises(RuntimeError, match="do not fit") as ei:
            capped.heldout_loss(wrap_pairs(as_numpy, *good))
        assert ei.value.status == _native.ERROR_DEVICE_MEMORY == 14
        assert capped.hbm_bytes == before
    finally:
        capped.close()


# ---- the fold scenarios --------------------------------------------------------------------------

def set_coverage(pset):
    """the per-base coverage of every contig of the set, read back through region_stats with one
    region per base"""
    regions = [(np.arange(n, dtype=np.int32), np.arange(1, n + 1, dtype=np.int32))
               for n in pset.contig_bases]
    return [r["sum"] for r in pset.region_stats(regions)]


def dense_fold_set(psd, wrap, vectors, folds, seed, penalties=(INF,)):
    """from_dense_folds twice (the same coverage, base for base), every fold's train and test
    contig against the yardstick, train + test = the input, the tests sum to the input -> the
    yardstick's counts per input"""
    from heldout_ref import dense_folds_ref
    covs = []
    for _ in range(2):
        pset = psd.ProblemSet.from_dense_folds([wrap(v) for v in vectors], list(penalties),
                                               folds=folds, seed=seed)
        try:
            assert pset.folds == folds and len(pset.contig_bases) == len(vectors) * folds * 2
            assert len(pset.problems) == len(vectors) * folds * len(penalties)
            covs.append(set_coverage(pset))
        finally:
            pset.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*covs))
    ms = ctypes.c_float(-1.0)
    assert _lib().peakseg_hip_fold_units_last_ms(ctypes.byref(ms)) == 0 and ms.value >= 0.0
    refs = []
    for i, v in enumerate(vectors):
        t = dense_folds_ref(v, i, folds, seed)
        assert np.array_equal(t.sum(axis=0), v)
        tests = np.zeros(len(v), dtype=np.int64)
        for f in range(folds):
            train, test = covs[0][(i * folds + f) * 2], covs[0][(i * folds + f) * 2 + 1]
            assert np.array_equal(test, t[f]), (i, f)
            assert np.array_equal(train + test, v), (i, f)
            tests += test
        assert np.array_equal(tests, v)
        refs.append(t)
    return refs


EDGE_COUNTS = [0, 1, 63, 64, 65, 32, 33, 21, 22, 43, 100000, 2, 3, 128, 129, 0]


def scenario_fold_counts(psd, wrap):
    """counts at the words' edges -- 0, 1, 63, 64, 65 for two folds, 32, 33 for four, 21, 22, 43 for
    eight -- and one base of 100 000; two identical input contigs get different splits; two seeds
    differ"""
    v = np.array(EDGE_COUNTS, dtype=np.int32)
    for folds in (2, 4, 8):
        a = dense_fold_set(psd, wrap, [v, v.copy()], folds, 1)
        assert not np.array_equal(a[0], a[1])
        b = dense_fold_set(psd, wrap, [v], folds, 2)
        assert not np.array_equal(a[0], b[0])
        # thinning: the big base's units spread over the folds about evenly
        big = a[0][:, EDGE_COUNTS.index(100000)]
        assert big.min() > 100000 / folds * 0.95 and big.max() < 100000 / folds * 1.05


def scenario_fold_sizes(psd, wrap):
    """contigs of 1, 255, 256, 257 and dense_tile_bases + 1 bases in one call"""
    tile = _lib().peakseg_hip_dense_tile_bases()
    assert tile + 1 <= 4100
    vectors = [poisson_vector(n, [(n // 3, n // 2, 12.0)], 40 + k, background=2.0)
               for k, n in enumerate((1, 255, 256, 257, tile + 1))]
    dense_fold_set(psd, wrap, vectors, 4, 7, penalties=(INF, 5.0))


def scenario_fold_refusals(psd, wrap):
    """the refused count 2^20 + 1, named by contig and base; a number of folds that is not 2, 4 or 8;
    no penalty"""
    most = _lib().peakseg_hip_fold_max_count()
    assert most == 2 ** 20
    ok = np.array([1, most, 3], dtype=np.int32)
    dense_fold_set(psd, wrap, [ok], 2, 3)
    bad = np.array([1, 2, 3, most + 1, 5], dtype=np.int32)
    with pytest.raises(RuntimeError, match="contig 1: base 3") as ei:
        psd.ProblemSet.from_dense_folds([wrap(ok), wrap(bad)], [INF], folds=4, seed=1)
    assert ei.value.status == 23
    for folds in (0, 1, 3, 16, -2):
        with pytest.raises(RuntimeError, match="not 2, 4 or 8") as ei:
            psd.ProblemSet.from_dense_folds([wrap(ok)], [INF], folds=folds, seed=1)
        assert ei.value.status == 23
        with pytest.raises(RuntimeError, match="not 2, 4 or 8") as ei:
            psd.ProblemSet.from_reads_folds([(wrap([1]), wrap([5]))], [INF], folds=folds, seed=1)
        assert ei.value.status == 23
    with pytest.raises(ValueError, match="no penalty"):
        psd.ProblemSet.from_dense_folds([wrap(ok)], [], folds=4)
    negative = np.array([1, -2, 3], dtype=np.int32)
    with pytest.raises(RuntimeError, match="negative") as ei:
        psd.ProblemSet.from_dense_folds([wrap(negative)], [INF], folds=2)
    assert ei.value.status == 17


def reads_fold_set(psd, wrap, reads, extents, folds, seed, bases_counted="each"):
    """from_reads_folds twice (the same coverage), every fold's train and test contig against the
    pile-up of the yardstick's folds, train + test = the pile-up of all reads"""
    from heldout_ref import pileup_ref, read_folds_ref
    covs = []
    for _ in range(2):
        pset = psd.ProblemSet.from_reads_folds(
            [tuple(wrap(a) for a in entry) for entry in reads], [INF], folds=folds, seed=seed,
            extents=extents, bases_counted=bases_counted)
        try:
            assert pset.contig_starts == [lo for lo, _ in extents for _ in range(2 * folds)]
            assert pset.contig_bases == [hi - lo for lo, hi in extents for _ in range(2 * folds)]
            covs.append(set_coverage(pset))
        finally:
            pset.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*covs))
    for i, entry in enumerate(reads):
        start, end = np.asarray(entry[0]), np.asarray(entry[1])
        count = np.asarray(entry[2]) if len(entry) == 3 else np.ones(len(start), dtype=np.int32)
        lo, hi = extents[i]
        fold = read_folds_ref(len(start), i, folds, seed)
        whole = pileup_ref(start, end, count, lo, hi, bases_counted)
        for f in range(folds):
            inside = fold == f
            test = pileup_ref(start[inside], end[inside], count[inside], lo, hi, bases_counted)
            assert np.array_equal(covs[0][(i * folds + f) * 2 + 1], test), (i, f)
            assert np.array_equal(covs[0][(i * folds + f) * 2], whole - test), (i, f)
    return covs[0]


def some_reads(n, seed, lo, hi):
    """n reads of 20 .. 115 bases that start in [lo - 60, hi + 20): some hang over either edge"""
    from peaksegdisk_amd import synthetic
    start = lo - 60 + np.floor(synthetic.uniform01(seed, 5, n) * (hi - lo + 80)).astype(np.int64)
    length = 20 + np.floor(synthetic.uniform01(seed, 6, n) * 96.0).astype(np.int64)
    return start.astype(np.int32), (start + length).astype(np.int32)


def scenario_fold_reads(psd, wrap):
    """reads in shuffled order, with and without the count column, clipped at the extent; 1, 256
    and 257 reads; two, four and eight folds; the last base of a read alone"""
    from peaksegdisk_amd import synthetic
    extents = [(100, 700), (0, 300), (50, 400), (1000, 1400)]
    reads = []
    for k, (n, (lo, hi)) in enumerate(zip((300, 1, 256, 257), extents)):
        start, end = synthetic.shuffled(90 + k, *some_reads(n, 80 + k, lo, hi))
        assert n < 2 or (np.diff(start) < 0).any()
        reads.append((start, end))
    counted = [entry + ((np.arange(len(entry[0])) % 4).astype(np.int32),) for entry in reads]
    for folds in (2, 4, 8):
        reads_fold_set(psd, wrap, reads, extents, folds, 5)
    cov = reads_fold_set(psd, wrap, counted, extents, 4, 5)
    assert sum(int(c.sum()) for c in cov) > 0
    reads_fold_set(psd, wrap, counted, extents, 2, 6, bases_counted="end")
    a = reads_fold_set(psd, wrap, reads[:1] * 2, extents[:1] * 2, 4, 9)
    assert not np.array_equal(a[1], a[9])      # two identical inputs get different splits


# ---- the selection, end to end -------------------------------------------------------------------

SELECT_SEED = 1
SELECT_FOLDS = 4
# (15 significant digits: what the entry points' paste() keeps of a penalty)
SELECT_PENALTIES = [0.0] + [float("%.15g" % x) for x in np.logspace(0.0, 5.25, 8)]


def three_peaks(seed=SELECT_SEED):
    """3000 bases: three peaks of rate 20 on a background of rate 0.5"""
    return poisson_vector(3000, [(400, 520, 20.0), (1300, 1450, 20.0), (2300, 2400, 20.0)], seed)


def yardstick_sums(pset, tests, folds, n_penalties, i=0):
    """(the sums over the folds of heldout_ref's losses of input i, one per penalty; the sums of
    their tolerances), from the set's own segments tables and the yardstick's test coverage"""
    import math
    cols = pset.segment_columns()
    sums, tols = [], []
    for j in range(n_penalties):
        refs = [heldout_pair_ref(cols[(i * folds + f) * n_penalties + j], tests[f], 1.0 / (folds - 1))
                for f in range(folds)]
        sums.append(math.fsum(r["loss"] for r in refs) if all(r["zero_mean_rows"] == 0 for r in refs)
                    else INF)
        tols.append(sum(r["tol"] for r in refs))
    return sums, tols


def check_choice(sel, sums, tols, penalties, folds):
    """the margin of the yardstick's choice, asserted first; then the selection against it.
    Neighbouring penalties of a log-spaced ladder often give the same models in every fold: their
    sums are the same bytes (yardstick and device alike), and the rule takes the largest of them.
    The margin is asserted between the best sum and the best sum that differs from it."""
    smallest = min(sums)
    tied = [j for j in range(len(sums)) if sums[j] == smallest]
    others = [sums[j] for j in range(len(sums)) if sums[j] != smallest]
    assert others and min(others) - smallest > 1000.0 * max(tols), (sums, tols)
    best = max(tied, key=lambda j: penalties[j])
    device = sel.summary["heldout_loss"].to_numpy()
    assert len({device[j].tobytes() for j in tied}) == 1
    assert sel.train_index == best and sel.train_penalty == penalties[best]
    assert sel.penalty == penalties[best] * folds / (folds - 1)
    total = sel.summary["heldout_loss"].to_numpy()
    for j in range(len(sums)):
        # (every fold's loss is within its tolerance; the two sums over the folds round once each)
        assert total[j] == sums[j] or abs(total[j] - sums[j]) <= tols[j] + 2.0 ** -51 * abs(sums[j]), j
    return best


def same_selection(a, b):
    assert a.table.equals(b.table) and a.summary.equals(b.summary)
    assert (a.train_index, a.train_penalty, a.penalty, a.rule) == \
        (b.train_index, b.train_penalty, b.penalty, b.rule)


def scenario_select_dense(psd, wrap):
    """select_penalty_dense end to end: the chosen penalty is the yardstick's argmin, by a margin;
    penalty 0 and the no-peak penalty lose; the chosen model has three peaks; refit"""
    from heldout_ref import dense_folds_ref
    from peaksegdisk_amd.heldout import select_from_set
    v, folds, pens = three_peaks(), SELECT_FOLDS, SELECT_PENALTIES
    pset = psd.ProblemSet.from_dense_folds([wrap(v)], pens, folds=folds, seed=SELECT_SEED)
    try:
        pset.solve()
        sel = select_from_set(pset)[0]
        same_selection(sel, select_from_set(pset)[0])
        sums, tols = yardstick_sums(pset, dense_folds_ref(v, 0, folds, SELECT_SEED), folds, len(pens))
    finally:
        pset.close()
    best = check_choice(sel, sums, tols, pens, folds)
    assert 0 < best < len(pens) - 1
    assert sums[0] > sums[best] and sums[-1] > sums[best]
    assert sel.table["peaks"][sel.table["penalty"] == pens[-1]].tolist() == [0] * folds
    assert sel.table["peaks"][sel.table["penalty"] == pens[best]].tolist() == [3] * folds
    assert list(sel.table.columns) == ["penalty", "fold", "peaks", "segments", "heldout_loss",
                                       "zero_mean_rows"]
    assert sel.table["fold"].tolist() == [f for f in range(folds) for _ in pens]
    whole = psd.select_penalty_dense(wrap(v), pens, folds=folds, seed=SELECT_SEED, refit=True)
    same_selection(whole, sel)
    want = psd.PeakSegFPOP_dense(wrap(v), [whole.penalty])[0]
    assert whole.fit.segments.equals(want.segments)
    assert whole.fit.loss.drop(columns=["seconds"]).equals(want.loss.drop(columns=["seconds"]))
    assert int(whole.fit.loss["peaks"].iloc[0]) == 3
    # several samples in one call, two folds, the other rule: each sample as if alone but for its
    # own random words
    small = poisson_vector(400, [(150, 220, 15.0)], 8)
    few = [2.0, 20.0, 2000.0]
    alone = psd.select_penalty_dense(wrap(small), few, folds=2, seed=4)
    two = psd.select_penalty_dense([wrap(small), wrap(small)], few, folds=2, seed=4, rule="1se")
    assert len(two) == 2 and two[0].rule == "1se" and two[0].fit is None and two[0].folds == 2
    assert two[0].table.equals(alone.table) and not two[1].table.equals(alone.table)
    assert two[0].train_penalty >= alone.train_penalty and two[0].penalty == two[0].train_penalty * 2


def scenario_select_reads(psd, wrap):
    """select_penalty_reads on synthetic.poisson_reads of a short contig against its yardstick"""
    from heldout_ref import pileup_ref, read_folds_ref
    from peaksegdisk_amd import synthetic
    from peaksegdisk_amd.heldout import select_from_set
    start, end, extent = synthetic.poisson_reads(120, seed=3)
    folds, pens = SELECT_FOLDS, SELECT_PENALTIES
    pset = psd.ProblemSet.from_reads_folds([(wrap(start), wrap(end))], pens, folds=folds, seed=2,
                                           extents=[extent])
    try:
        pset.solve()
        sel = select_from_set(pset)[0]
        fold = read_folds_ref(len(start), 0, folds, 2)
        ones = np.ones(len(start), dtype=np.int64)
        tests = [pileup_ref(start[fold == f], end[fold == f], ones[fold == f], *extent)
                 for f in range(folds)]
        sums, tols = yardstick_sums(pset, tests, folds, len(pens))
    finally:
        pset.close()
    check_choice(sel, sums, tols, pens, folds)
    whole = psd.select_penalty_reads((wrap(start), wrap(end)), pens, folds=folds, seed=2,
                                     extents=extent, refit=True)
    same_selection(whole, sel)
    want = psd.PeakSegFPOP_reads((wrap(start), wrap(end)), [whole.penalty], extents=extent)[0]
    assert whole.fit.segments.equals(want.segments)


LOSS_SCENARIOS = [scenario_own_contig, scenario_one_row, scenario_row_counts, scenario_run_counts,
                  scenario_pair_counts, scenario_zero_segment, scenario_refusals]
FOLD_SCENARIOS = [scenario_fold_counts, scenario_fold_sizes, scenario_fold_refusals,
                  scenario_fold_reads]
SCENARIOS = LOSS_SCENARIOS + FOLD_SCENARIOS + [scenario_select_dense, scenario_select_reads]


# ---- MI355X ----------------------------------------------------------------------------------

@GPU
@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__[len("scenario_"):])
def test_gpu_heldout(psd, scenario):
    scenario(psd, as_numpy)


_CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process
sys.path[:0] = [%(root)r, %(tests)r]
import test_gpu_heldout as gh
gh.child_main()
print("heldout-child ok")
"""


def child_main():
    import torch
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd as psd
    # contigs and pairs in cuda tensors, read in place; the device-side check of the pairs
    scenario_own_contig(psd, as_cuda)
    scenario_pair_counts(psd, as_cuda)
    scenario_refusals(psd, as_cuda)
    # numpy and cuda inputs give the same set: the same yardstick, base for base
    scenario_fold_counts(psd, as_cuda)
    scenario_fold_refusals(psd, as_cuda)
    scenario_fold_reads(psd, as_cuda)
    # the torch_device form: tensors that alias the library's buffers
    vectors = [steps(200, [(50, 90, 12)]), steps(200, [(60, 80, 5)])]
    pset = make_set(psd, as_cuda, vectors, [(0, 5.0), (1, 5.0)])
    try:
        pairs = ([0, 1, 0], [1, 0, 0], [0.5, 0.5, 1.0])
        host = pset.heldout_loss(wrap_pairs(as_numpy, *pairs))
        dev = pset.heldout_loss(wrap_pairs(as_cuda, *pairs), torch_device="cuda:0")
        assert [dev[k].dtype for k in ("loss", "rows", "bases", "sum", "zero_mean_rows")] == \
            [torch.float64, torch.int32, torch.int64, torch.int64, torch.int32]
        for name in host:
            assert dev[name].device.type == "cuda" and tuple(dev[name].shape) == (3,)
            assert dev[name].cpu().numpy().tobytes() == host[name].tobytes(), name
        mixed = wrap_pairs(as_cuda, *pairs)[:2] + (np.array(pairs[2]),)
        try:
            pset.heldout_loss(mixed)
            raise AssertionError("pairs in two kinds of memory were accepted")
        except ValueError as e:
            assert "one call takes one kind" in str(e)
    finally:
        pset.close()


@GPU
def test_gpu_heldout_cuda_tensors(psd):
    """contigs and pairs in cuda tensors, the device-side check of the pairs, and the torch_device
    form"""
    import subprocess
    import sys
    from conftest import ROOT
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(p.stdout[-4000:])
    assert p.returncode == 0 and "heldout-child ok" in p.stdout, p.stdout[-3000:] + p.stderr[-6000:]
