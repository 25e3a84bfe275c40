"""Dense in-memory coverage: run-length encoding on the device, ProblemSet.from_dense,
segment_columns / loss and PeakSegFPOP_dense.

The scenario functions are shared with the emulator rehearsal (tests/test_dense_emu.py), which runs
them without a GPU on host arrays; the tests marked gpu run them on the MI355X with the input once
as numpy arrays and once as cuda tensors, plus the sizes the emulator cannot do (2048 contigs, one
contig of 2.5e8 bases).

Expected values never come from the library under test: the encoder is compared with numpy's
run-length encoding, the solver with the deterministic oracle run on a bedGraph file of the
RE-ENCODED runs (adjacent equal bins of the synthetic data merge into one run in the dense form).
Mono27ac has no two equal neighbours, expands and re-encodes to itself, and its recorded answers
(tests/golden/known_answers.json) apply as they stand; its 20-digit loss fields were recorded from
the libm build of the oracle, which the deterministic build matches to REL_TOL only
(tests/test_oracle_golden.py), so they are compared with that tolerance and the deterministic
oracle's own file exactly."""
import ctypes
import os
import subprocess
import time

import numpy as np
import pytest

from conftest import GOLDEN, ORACLE_DIR, format_g, read_loss, read_segments

GPU = pytest.mark.gpu
REL_TOL = 1e-6  # libm build against deterministic build of the oracle, as tests/test_oracle_golden.py


@pytest.fixture(scope="module")
def psd():
    import __graft_entry__ as entry
    entry.build_hip()
    entry.build_oracle()
    import peaksegdisk_amd
    from peaksegdisk_amd import _native
    assert _native.lib.peakseg_hip_device_count() >= 1, "no HIP device: GPU tests need an MI355X"
    return peaksegdisk_amd


def _lib():
    from peaksegdisk_amd import _native
    return _native.lib


# ---- helpers ---------------------------------------------------------------------------------

def rle(x):
    """numpy's run-length encoding as api.PeakSegFPOP_vec does it: (count, weight, run_end)"""
    x = np.asarray(x)
    change = np.flatnonzero(np.diff(x) != 0)
    ends = np.concatenate([change + 1, [len(x)]]).astype(np.int64)
    starts = np.concatenate([[0], ends[:-1]]).astype(np.int64)
    return x[starts].astype(np.int32), (ends - starts).astype(np.int32), ends.astype(np.int32)


def merge_runs(count, width):
    """the run-length encoding of np.repeat(count, width) without expanding it"""
    count = np.asarray(count)
    first = np.concatenate([[True], count[1:] != count[:-1]])
    ends_all = np.cumsum(np.asarray(width, dtype=np.int64))
    last = np.concatenate([first[1:], [True]])
    ends = ends_all[last]
    starts = np.concatenate([[0], ends[:-1]])
    return count[first].astype(np.int32), (ends - starts).astype(np.int32), ends.astype(np.int32)


def as_numpy(v):
    return np.ascontiguousarray(v, dtype=np.int32)


def as_cuda(v):
    import torch
    return torch.from_numpy(as_numpy(v)).to("cuda:0")


def _address(v):
    if isinstance(v, np.ndarray):
        return v.ctypes.data, 0
    return v.data_ptr(), 1 if v.device.type == "cuda" else 0


def encode_probe(vectors):
    """-> (status, runs int64[C], count, weight, run_end (concatenated), min, max, sum)"""
    nc = len(vectors)
    lens = [int(v.shape[0]) for v in vectors]
    nb = (ctypes.c_longlong * nc)(*lens)
    where = [_address(v) for v in vectors]
    assert len({w for _, w in where}) == 1
    ptr = (ctypes.c_void_p * nc)(*[a for a, _ in where])
    total = sum(lens)
    runs = np.zeros(nc, np.int64)
    sums = np.zeros(nc, np.int64)
    mn = np.zeros(nc, np.int32)
    mx = np.zeros(nc, np.int32)
    out = [np.full(total, -7, np.int32) for _ in range(3)]
    st = _lib().peakseg_hip_dense_encode_probe(
        0, nc, nb, ptr, where[0][1], runs.ctypes.data, out[0].ctypes.data, out[1].ctypes.data,
        out[2].ctypes.data, mn.ctypes.data, mx.ctypes.data, sums.ctypes.data)
    k = int(runs.sum()) if st == 0 else 0
    return st, runs, out[0][:k], out[1][:k], out[2][:k], mn, mx, sums


def check_encoding(vectors_np, wrap, what):
    st, runs, count, weight, run_end, mn, mx, sums = encode_probe([wrap(v) for v in vectors_np])
    assert st == 0, (what, _lib().peakseg_hip_last_error())
    want = [rle(v) for v in vectors_np]
    assert runs.tolist() == [len(w[0]) for w in want], what
    assert np.array_equal(count, np.concatenate([w[0] for w in want])), what
    assert np.array_equal(weight, np.concatenate([w[1] for w in want])), what
    assert np.array_equal(run_end, np.concatenate([w[2] for w in want])), what
    assert mn.tolist() == [int(v.min()) for v in vectors_np], what
    assert mx.tolist() == [int(v.max()) for v in vectors_np], what
    assert sums.tolist() == [int(v.astype(np.int64).sum()) for v in vectors_np], what
    return count, weight, run_end


def geometric_vector(rng, n, p=0.2, top=6):
    """n bases of runs with geometric lengths"""
    k = max(4, int(n * p * 2) + 4)
    while True:
        lengths = rng.geometric(p, k)
        if lengths.sum() >= n:
            break
        k *= 2
    return np.repeat(rng.integers(0, top, k), lengths)[:n].astype(np.int32)


# ---- scenario 3: the encoder against numpy ---------------------------------------------------

def scenario_encoder(wrap):
    T = _lib().peakseg_hip_dense_tile_bases()
    assert T >= 64
    rng = np.random.default_rng(20240607)
    for n in (1, 2, T - 1, T, T + 1, 3 * T + 5):
        check_encoding([geometric_vector(rng, n)], wrap, "length %d" % n)
    check_encoding([np.full(2 * T + 3, 9, np.int32)], wrap, "constant")
    check_encoding([(np.arange(2 * T + 7) % 5).astype(np.int32)], wrap, "no equal neighbours")
    v = np.zeros(5 * T, np.int32)
    v[T - 3:T + 4] = 2                 # a run over one tile boundary
    v[2 * T - 1:4 * T + 1] = 7         # a run over three
    v[4 * T + 1:] = 1
    check_encoding([v], wrap, "runs that straddle tile boundaries")
    for k in range(20):
        n = int(rng.integers(1, 3 * T))
        check_encoding([geometric_vector(rng, n, p=float(rng.choice([0.02, 0.2, 0.7])))], wrap,
                       "random %d" % k)
    # one call of 50 contigs: neighbours that meet in equal values stay two runs
    lens = rng.integers(1, 3 * T + 1, 50)
    lens[[4, 17, 33]] = 1
    many = [geometric_vector(rng, int(n)) for n in lens]
    for c in (5, 18, 20, 41):
        many[c][0] = many[c - 1][-1]
    assert many[17][0] == many[18][0]
    check_encoding(many, wrap, "50 contigs")
    if wrap is not as_numpy:
        # device input at every 4-byte offset of a 16-byte line: slices of one buffer
        base = wrap(geometric_vector(rng, 2 * T + 16))
        for lead in range(4):
            part = base[lead:lead + T + 9]
            st, runs, count, weight, run_end, _, _, _ = encode_probe([part])
            want = rle(part.cpu().numpy())
            assert st == 0 and np.array_equal(count, want[0]) and np.array_equal(weight, want[1]) \
                and np.array_equal(run_end, want[2]), lead


def scenario_encoder_refusals(wrap):
    from peaksegdisk_amd import _native
    v = np.array([3, 3, 1, -2, 5], np.int32)
    st = encode_probe([wrap(np.ones(7, np.int32)), wrap(v)])[0]
    assert st == _native.ERROR_DENSE_ARGUMENTS
    err = _native.lib.peakseg_hip_last_error().decode()
    assert "contig 1" in err and "negative" in err, err
    big = np.full(2 ** 22 + 1, 2 ** 31 - 1, np.int32)   # sums to 2^53 + 2^31 - 2^22 - 1
    st = encode_probe([wrap(big)])[0]
    assert st == _native.ERROR_DENSE_ARGUMENTS
    err = _native.lib.peakseg_hip_last_error().decode()
    assert "contig 0" in err and "2^53" in err, err
    ok = np.full(2 ** 22, 2 ** 31 - 1, np.int32)        # just below: accepted, exact
    st, runs, count, weight, run_end, mn, mx, sums = encode_probe([wrap(ok)])
    assert st == 0 and runs[0] == 1 and sums[0] == (2 ** 31 - 1) * 2 ** 22 < 2 ** 53
    assert weight.tolist() == [2 ** 22] and run_end.tolist() == [2 ** 22]


# ---- scenario 4: the whole path against the oracle --------------------------------------------

def oracle_files(oracle, directory, chrom, first, vector, pen_str):
    """the oracle's two files for the re-encoded runs of `vector`"""
    os.makedirs(directory, exist_ok=True)
    bg = os.path.join(directory, "coverage.bedGraph")
    if not os.path.exists(bg):
        count, weight, ends = rle(vector)
        with open(bg, "w") as f:
            f.write("".join("%s\t%d\t%d\t%d\n" % (chrom, first + e - w, first + e, c) for c, w, e in
                            zip(count.tolist(), weight.tolist(), ends.tolist())))
    assert oracle.solve(bg, pen_str) == 0
    pre = "%s_penalty=%s" % (bg, pen_str)
    return read_segments(pre + "_segments.bed"), read_loss(pre + "_loss.tsv").split("\t")


def check_problem(columns, loss, segs, loss_text, what):
    """one problem's segment_columns() and loss() against the oracle's files"""
    start, end, mean = columns
    assert start.tolist() == [r[1] for r in segs], what
    assert end.tolist() == [r[2] for r in segs], what
    assert ["background" if k % 2 == 0 else "peak" for k in range(len(start))] == \
        [r[3] for r in segs], what
    assert format_g(mean) == [r[4] for r in segs], what
    assert len(loss) == 10
    for k in range(10):
        assert float(loss[k]) == float(loss_text[k]), (what, k, loss[k], loss_text[k])


def mono27ac_dense():
    cols = np.loadtxt(os.path.join(GOLDEN, "Mono27ac.bedGraph"), usecols=(1, 2, 3), dtype=np.int64)
    assert cols[0, 0] == 60000 and cols[-1, 1] == 580000
    return np.repeat(cols[:, 2], cols[:, 1] - cols[:, 0]).astype(np.int32)


def scenario_mono27ac(psd, oracle_det, known_answers, tmp_path, wrap):
    dense = mono27ac_dense()
    assert len(dense) == 520000 and len(rle(dense)[0]) == 6921
    pens = ["0", "1952.6", "10000", "Inf"]
    pset = psd.ProblemSet.from_dense([wrap(dense)], [(0, float(p)) for p in pens])
    try:
        pset.solve()
        launches, steps = pset.solve_stats
        assert launches >= 1 and steps == 3 * 6921       # the Inf model is not launched
        columns = pset.segment_columns(first_chromStart=[60000])
        for k, pen in enumerate(pens):
            want = known_answers["mono27ac"]["penalties"][pen]
            loss = pset.loss(k)
            assert int(loss[1]) == want["segments"] and int(loss[2]) == want["peaks"]
            assert int(loss[3]) == 520000 and int(loss[4]) == 6921
            assert loss[6] == pytest.approx(float(want["total_loss"]), rel=REL_TOL)
            if "equality_constraints" in want:
                assert int(loss[7]) == want["equality_constraints"]
            if "max_intervals" in want:
                assert loss[9] == want["max_intervals"]
            if "mean_pen_cost" in want:
                assert loss[5] == pytest.approx(float(want["mean_pen_cost"]), rel=REL_TOL)
            if "first_segment_row" in want:
                row = want["first_segment_row"].split("\t")
                assert [int(columns[k][0][0]), int(columns[k][1][0]), "%g" % columns[k][2][0]] == \
                    [int(row[1]), int(row[2]), row[4]]
            segs, loss_text = oracle_files(oracle_det, str(tmp_path / "mono"), "chr11", 60000,
                                           dense, pen)
            check_problem(columns[k], loss, segs, loss_text, "Mono27ac penalty %s" % pen)
            r = pset.result(k)
            assert r.n_segments == want["segments"] and r.n_peaks == want["peaks"]
            s_idx, s_mean = pset.segments(k)
            assert len(s_idx) == want["segments"] and np.array_equal(s_mean, columns[k][2])
    finally:
        pset.close()
    return columns


def three_contigs():
    from peaksegdisk_amd import synthetic
    cs, ce, cnt = synthetic.poisson_coverage(3000, seed=5)
    a = np.repeat(cnt, ce - cs).astype(np.int32)
    b = synthetic.increasing_coverage(400)[2].astype(np.int32)
    c = np.full(777, 4, np.int32)
    return [a, b, c]


def scenario_three_contigs(psd, oracle_det, tmp_path, wrap):
    vectors = three_contigs()
    assert len(rle(vectors[0])[0]) < 3000  # equal neighbours merged: the problem is the merged one
    pens = ["0.5", "40", "3000", "Inf"]
    firsts = [1000, 0, 123456]
    problems = [(c, float(p)) for c in range(3) for p in pens]
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors], problems)
    try:
        pset.solve()
        launches, steps = pset.solve_stats
        # 6 dynamic programs; Inf and the constant contig have the closed form
        assert steps == 3 * (len(rle(vectors[0])[0]) + 400), steps
        with_starts = pset.segment_columns(first_chromStart=firsts)
        without = pset.segment_columns()
        rows, ptr_s, ptr_m, total = pset.pack_tables()
        assert total == sum(len(c[0]) for c in without)
        for k, (c, _) in enumerate(problems):
            pen = pens[k % 4]
            segs, loss_text = oracle_files(oracle_det, str(tmp_path / ("c%d" % c)), "chrT",
                                           firsts[c], vectors[c], pen)
            check_problem(with_starts[k], pset.loss(k), segs, loss_text, (c, pen))
            assert np.array_equal(without[k][0] + firsts[c], with_starts[k][0])
            assert np.array_equal(without[k][1] + firsts[c], with_starts[k][1])
            assert np.array_equal(without[k][2], with_starts[k][2])
            if c == 2 or pen == "Inf":
                assert len(with_starts[k][0]) == 1 and pset.result(k).n_segments == 1
    finally:
        pset.close()
    # a set of nothing but closed forms launches no forward kernel
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors], [(0, float("inf")), (2, 40.0)])
    try:
        f_ms, _ = pset.solve()
        assert pset.solve_stats == (0, 0) and f_ms == 0.0
        cols = pset.segment_columns(first_chromStart=firsts)
        assert [int(cols[1][0][0]), int(cols[1][1][0]), float(cols[1][2][0])] == \
            [123456, 123456 + 777, 4.0]
        # ... and goes on to a dynamic program when a penalty changes
        pset.set_penalty(0, 40.0)
        pset.solve()
        assert pset.solve_stats[0] >= 1
        segs, loss_text = oracle_files(oracle_det, str(tmp_path / "c0"), "chrT", firsts[0],
                                       vectors[0], "40")
        check_problem(pset.segment_columns(first_chromStart=firsts)[0], pset.loss(0), segs,
                      loss_text, "after set_penalty")
    finally:
        pset.close()
    # a set that was not made from dense counts has no run_end[]
    count, weight, _ = rle(vectors[1])
    plain = psd.ProblemSet([(count, weight)], [(0, 40.0)])
    try:
        plain.solve()
        with pytest.raises(RuntimeError, match="dense"):
            plain.segment_columns()
    finally:
        plain.close()


def scenario_api(psd, tmp_path, wrap):
    """PeakSegFPOP_dense against PeakSegFPOP_dir on a directory that holds the same runs"""
    vectors = three_contigs()[:2]
    pens = [[0.5, 3000, float("inf")], [40]]
    got = psd.PeakSegFPOP_dense([wrap(v) for v in vectors], pens, chrom="chrT",
                                chrom_starts=[1000, 0])
    assert [len(g) for g in got] == [3, 1]
    for c, v in enumerate(vectors):
        d = tmp_path / ("dir%d" % c)
        d.mkdir(parents=True)
        count, weight, ends = rle(v)
        first = [1000, 0][c]
        with open(str(d / "coverage.bedGraph"), "w") as f:
            f.write("".join("chrT\t%d\t%d\t%d\n" % (first + e - w, first + e, k) for k, w, e in
                            zip(count.tolist(), weight.tolist(), ends.tolist())))
        for k, pen in enumerate(pens[c]):
            want = psd.PeakSegFPOP_dir(str(d), psd.paste(pen))
            fit = got[c][k]
            assert fit.segments.equals(want.segments), (c, pen)
            assert list(fit.segments.dtypes) == list(want.segments.dtypes)
            keep = [n for n in want.loss.columns if n != "seconds"]
            assert list(fit.loss.columns) == list(want.loss.columns)
            assert fit.summary()[keep].equals(want.summary()[keep]), (c, pen)
            assert list(fit.loss.dtypes) == list(want.loss.dtypes), (c, pen)
            a, b = fit.coef(), want.coef()
            assert a.segments.equals(b.segments) and a.changes.equals(b.changes) and \
                a.peaks.equals(b.peaks)
    one = psd.PeakSegFPOP_dense(wrap(vectors[1]), [40])
    assert len(one) == 1 and one[0].segments["chrom"].iloc[0] == "chrUnknown"
    assert one[0].segments["mean"].tolist() == got[1][0].segments["mean"].tolist()


# ---- MI355X ----------------------------------------------------------------------------------
# The tests that hand cuda tensors to the library run in a child process that imports torch
# first: torch ships its own HIP runtime, which must be the first one loaded (bench.py and
# tests/test_gpu_round3.py do the same); child_main() below is what the child runs.

_CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process
sys.path[:0] = [%(root)r, %(tests)r]
import test_gpu_dense as gd
gd.child_main(sys.argv[1], sys.argv[2])
print("dense-child ok")
"""


def run_child(which, tmp_path, timeout):
    import sys
    from conftest import ROOT
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code, which, str(tmp_path)], capture_output=True,
                       text=True, timeout=timeout)
    print(p.stdout[-4000:])
    assert p.returncode == 0 and "dense-child ok" in p.stdout, p.stdout[-3000:] + p.stderr[-6000:]


def child_main(which, tmp):
    import json
    import pathlib
    import __graft_entry__ as entry
    from conftest import Oracle
    entry.build_hip()
    entry.build_oracle()
    import peaksegdisk_amd as psd
    tmp_path = pathlib.Path(tmp)
    if which == "encoder":
        scenario_encoder(as_cuda)
        scenario_encoder_refusals(as_cuda)
    elif which == "whole_path":
        with open(os.path.join(GOLDEN, "known_answers.json")) as f:
            known = json.load(f)
        whole_path_both_ways(psd, Oracle("det"), known, tmp_path)
    elif which == "throughput":
        throughput_regime(psd, tmp_path)
    elif which == "long":
        one_long_contig(psd, tmp_path)
    else:
        raise ValueError(which)


@GPU
def test_gpu_dense_encoder_numpy(psd):
    scenario_encoder(as_numpy)
    scenario_encoder_refusals(as_numpy)


@GPU
def test_gpu_dense_encoder_cuda_tensors(psd, tmp_path):
    run_child("encoder", tmp_path, 300)


@GPU
def test_gpu_dense_whole_path(psd, tmp_path):
    """Scenarios 3 and 4 once from numpy arrays and once from cuda tensors: the same bits both
    ways; one cuda run is made with Tensor.cpu / Tensor.numpy patched to raise (no copy through
    the host); segment_columns(torch_device=...) aliases the library's packed buffers."""
    run_child("whole_path", tmp_path, 600)


def whole_path_both_ways(psd, oracle_det, known_answers, tmp_path):
    import torch
    from unittest import mock
    a = scenario_mono27ac(psd, oracle_det, known_answers, tmp_path / "n", as_numpy)
    scenario_three_contigs(psd, oracle_det, tmp_path / "n", as_numpy)
    scenario_api(psd, tmp_path / "n", as_numpy)

    def refuse(*args, **kwargs):
        raise AssertionError("a cuda tensor was copied to the host")
    dense_t = as_cuda(mono27ac_dense())
    with mock.patch.object(torch.Tensor, "cpu", refuse), \
            mock.patch.object(torch.Tensor, "numpy", refuse):
        pset = psd.ProblemSet.from_dense([dense_t], [(0, 1952.6), (0, 0.0)])
        try:
            pset.solve()
            cols = pset.segment_columns(first_chromStart=[60000])
            offs, t_start, t_end, t_mean = pset.segment_columns(first_chromStart=[60000],
                                                                torch_device="cuda:0")
            kept = [t_start.clone(), t_end.clone(), t_mean.clone()]
            p1, p2, p3 = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
            first = (ctypes.c_int * 1)(60000)
            total = _lib().peakseg_hip_problem_set_pack_segments(
                pset._h, first, None, ctypes.byref(p1), ctypes.byref(p2), ctypes.byref(p3))
            assert (t_start.data_ptr(), t_end.data_ptr(), t_mean.data_ptr()) == \
                (p1.value, p2.value, p3.value)
            assert total == len(t_start) == offs[-1] and t_start.device.type == "cuda"
            assert t_start.dtype == torch.int32 and t_mean.dtype == torch.float64
        finally:
            pset.close()
    for k in (0, 1):
        sl = slice(int(offs[k]), int(offs[k + 1]))
        assert np.array_equal(kept[0].cpu().numpy()[sl], cols[k][0])
        assert np.array_equal(kept[1].cpu().numpy()[sl], cols[k][1])
        assert np.array_equal(kept[2].cpu().numpy()[sl], cols[k][2])
    assert np.array_equal(cols[0][0], a[1][0]) and np.array_equal(cols[0][2], a[1][2])
    assert np.array_equal(cols[1][0], a[0][0]) and np.array_equal(cols[1][2], a[0][2])
    b = scenario_mono27ac(psd, oracle_det, known_answers, tmp_path / "t", as_cuda)
    for x, y in zip(a, b):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
    scenario_three_contigs(psd, oracle_det, tmp_path / "t", as_cuda)
    scenario_api(psd, tmp_path / "t", as_cuda)


def _oracle_cli(bg, pen, db):
    return subprocess.Popen([os.path.join(ORACLE_DIR, "_build", "oracle_cli_det"), bg, pen, db],
                            stdout=subprocess.DEVNULL)


@GPU
def test_gpu_dense_throughput_regime(psd, tmp_path):
    run_child("throughput", tmp_path, 600)


def throughput_regime(psd, tmp_path):
    """2048 contigs of 10 k bins expanded on the device (about 2.5e5 bases each, 2 GB of int32 in
    all), one penalty each: every packed table and psd_result equal to the set made from
    host-encoded arrays, 64 seeded picks equal to the oracle's files.  The build of the forward
    kernel is the planner's choice and is printed."""
    import torch
    from peaksegdisk_amd import synthetic
    n_contigs = 2048
    grid = synthetic.penalty_grid()
    rng = np.random.default_rng(7)
    picks = sorted(rng.choice(n_contigs, 64, replace=False).tolist())
    host, dense, runs_of, procs = [], [], {}, {}
    for k in range(n_contigs):
        cs, ce, cnt = synthetic.poisson_coverage(10000, seed=k)
        width = (ce - cs).astype(np.int64)
        count, weight, ends = merge_runs(cnt, width)
        host.append((count, weight))
        dense.append(torch.repeat_interleave(torch.from_numpy(cnt).to("cuda:0"),
                                             torch.from_numpy(width).to("cuda:0")))
        assert dense[-1].dtype == torch.int32 and len(dense[-1]) == int(ends[-1])
        if k in picks:
            d = tmp_path / ("o%d" % k)
            d.mkdir()
            bg = str(d / "coverage.bedGraph")
            synthetic.write_bedgraph(bg, ends - weight, ends, count, chrom="chrT")
            procs[k] = _oracle_cli(bg, grid[k % 64], bg + ".db")
            runs_of[k] = bg
    problems = [(k, float(grid[k % 64])) for k in range(n_contigs)]
    t0 = time.time()
    a = psd.ProblemSet.from_dense(dense, problems)
    t_create = time.time() - t0
    del dense
    b = psd.ProblemSet(host, problems)
    try:
        ms_a = a.solve()[0]
        ms_b = b.solve()[0]
        print("dense set: created in %.3f s, kernel %.1f ms on %s; host-encoded set: %.1f ms on %s"
              % (t_create, ms_a, a.kernel_build, ms_b, b.kernel_build))
        rows_a, _, _, total_a = a.pack_tables()
        rows_b, _, _, total_b = b.pack_tables()
        assert total_a == total_b and np.array_equal(rows_a, rows_b)
        start_a, mean_a = a.packed_download(total_a)
        start_b, mean_b = b.packed_download(total_b)
        assert np.array_equal(start_a, start_b) and np.array_equal(mean_a, mean_b)
        fields = ["status", "kernel_status", "n_segments", "n_peaks", "n_equality_constraints",
                  "max_intervals", "total_intervals", "best_cost"]
        for k in range(n_contigs):
            ra, rb = a.result(k), b.result(k)
            assert [getattr(ra, f) for f in fields] == [getattr(rb, f) for f in fields], k
        columns = a.segment_columns()
        for k in picks:
            assert procs[k].wait() == 0
            pre = "%s_penalty=%s" % (runs_of[k], grid[k % 64])
            check_problem(columns[k], a.loss(k), read_segments(pre + "_segments.bed"),
                          read_loss(pre + "_loss.tsv").split("\t"), k)
    finally:
        a.close()
        b.close()
        for p in procs.values():
            if p.poll() is None:
                p.kill()


@GPU
def test_gpu_dense_one_long_contig(psd, tmp_path):
    run_child("long", tmp_path, 600)


def one_long_contig(psd, tmp_path):
    """One contig of 2.5e8 bases (poisson_coverage(10**7) expanded on the device, 1 GB): the
    encoder's arrays against the run-length encoding of the same vector (computed from the bins:
    merging equal neighbours of (count, width) is the encoding of their expansion).  Then its
    first 2.5e7 bases at 4 penalties from the device tensor against the host-encoded set, the two
    largest penalties against the oracle's files as well."""
    import torch
    from peaksegdisk_amd import synthetic
    cs, ce, cnt = synthetic.poisson_coverage(10 ** 7, seed=1)
    width = (ce - cs).astype(np.int64)
    dense = torch.repeat_interleave(torch.from_numpy(cnt).to("cuda:0"),
                                    torch.from_numpy(width).to("cuda:0"))
    assert dense.dtype == torch.int32 and len(dense) == int(ce[-1]) > 2.4e8
    want = merge_runs(cnt, width)
    st, runs, count, weight, run_end, mn, mx, sums = encode_probe([dense])
    assert st == 0 and runs[0] == len(want[0])
    assert np.array_equal(count, want[0]) and np.array_equal(weight, want[1]) and \
        np.array_equal(run_end, want[2])
    assert (mn[0], mx[0], sums[0]) == (cnt.min(), cnt.max(),
                                       int((cnt.astype(np.int64) * width).sum()))
    ms = [ctypes.c_float() for _ in range(3)]
    _lib().peakseg_hip_dense_last_encode_ms(*[ctypes.byref(m) for m in ms])
    total_ms = sum(m.value for m in ms)
    print("encoder, %d bases, %d runs: count %.3f ms, scan %.3f ms, scatter %.3f ms: %.2f TB/s"
          % (len(dense), runs[0], ms[0].value, ms[1].value, ms[2].value,
             (8.0 * len(dense) + 12.0 * runs[0]) / (total_ms * 1e-3) / 1e12))
    # the first 2.5e7 bases
    n_head = 25 * 10 ** 6
    bins = int(np.searchsorted(ce, n_head, side="left")) + 1
    w_head = width[:bins].copy()
    w_head[-1] -= int(ce[bins - 1]) - n_head
    h_count, h_weight, h_ends = merge_runs(cnt[:bins], w_head)
    assert int(h_ends[-1]) == n_head
    pens = ["0.72", "37.3", "1550.5", "51795"]
    d = tmp_path / "head"
    d.mkdir()
    bg = str(d / "coverage.bedGraph")
    synthetic.write_bedgraph(bg, h_ends - h_weight, h_ends, h_count, chrom="chrT")
    procs = {pen: _oracle_cli(bg, pen, "%s_%s.db" % (bg, pen)) for pen in pens[2:]}
    problems = [(0, float(p)) for p in pens]
    a = psd.ProblemSet.from_dense([dense[:n_head]], problems)
    b = psd.ProblemSet([(h_count, h_weight)], problems)
    try:
        ms_a = a.solve()[0]
        ms_b = b.solve()[0]
        print("%d runs x 4 penalties: kernel %.0f ms from dense counts, %.0f ms host-encoded"
              % (len(h_count), ms_a, ms_b))
        rows_a, _, _, total_a = a.pack_tables()
        rows_b, _, _, total_b = b.pack_tables()
        assert total_a == total_b and np.array_equal(rows_a, rows_b)
        for x, y in zip(a.packed_download(total_a), b.packed_download(total_b)):
            assert np.array_equal(x, y)
        columns = a.segment_columns()
        for k in (2, 3):
            assert procs[pens[k]].wait() == 0
            pre = "%s_penalty=%s" % (bg, pens[k])
            check_problem(columns[k], a.loss(k), read_segments(pre + "_segments.bed"),
                          read_loss(pre + "_loss.tsv").split("\t"), pens[k])
    finally:
        a.close()
        b.close()
        for p in procs.values():
            if p.poll() is None:
                p.kill()
