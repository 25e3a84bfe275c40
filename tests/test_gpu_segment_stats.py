"""ProblemSet.segment_stats: the reads, the largest count and the summit of every row of the
segments table, computed on the device from the resident runs.

The scenario functions are shared with the emulator rehearsal (tests/test_segment_stats_emu.py),
which runs them without a GPU on host arrays; the tests marked gpu run them on the MI355X with the
input once as numpy arrays (in this process) and once as cuda tensors (in a child process that
imports torch first, as tests/test_gpu_dense.py does).

The expected columns never come from the library: for a row [a, b) of segment_columns() they are
numpy on the dense vector -- v[a:b].sum() in int64, v[a:b].max(), and the first index that attains
the maximum, extended to the end of its run.  Everything is integer arithmetic, so the comparisons
are exact.  Where a solved model is at hand the sums also give a check of the solver that involves
neither the oracle nor a file: sum over rows of (length * mean - sum * log(mean)) is total.loss."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_gpu_dense import as_cuda, as_numpy, mono27ac_dense, rle, three_contigs

GPU = pytest.mark.gpu
LOSS_TOL = 1e-12   # of the sum of the rows' |terms|: numpy's log against the library's own


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


# ---- the oracle: numpy on the dense vector -----------------------------------------------------

def expected_stats(v, start, end, first):
    """the four columns of the rows [start, end) (coordinates that begin at `first`) of vector v"""
    v = np.asarray(v)
    _, weight, ends = rle(v)
    run_end_of_base = np.repeat(ends.astype(np.int64), weight)
    n = len(start)
    out = (np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32),
           np.zeros(n, np.int32))
    for r, (a, b) in enumerate(zip((start.astype(np.int64) - first).tolist(),
                                   (end.astype(np.int64) - first).tolist())):
        part = v[a:b]
        assert len(part) > 0
        i = a + int(np.argmax(part))              # the first index that attains the maximum
        out[0][r] = part.sum(dtype=np.int64)
        out[1][r] = part.max()
        out[2][r] = first + i
        out[3][r] = first + run_end_of_base[i]
    return out


def check_set(pset, vectors, firsts=None, what=""):
    """every problem's four columns against numpy; -> (segment_columns, segment_stats)"""
    columns = pset.segment_columns(first_chromStart=firsts)
    stats = pset.segment_stats(first_chromStart=firsts)
    assert len(stats) == len(columns) == len(pset.problems)
    for k, (c, pen) in enumerate(pset.problems):
        first = 0 if firsts is None else firsts[c]
        want = expected_stats(vectors[c], columns[k][0], columns[k][1], first)
        got = stats[k]
        assert [a.dtype for a in got] == [np.int64, np.int32, np.int32, np.int32]
        for name, g, w in zip(("sum", "max", "summitStart", "summitEnd"), got, want):
            assert len(g) == len(columns[k][0]), (what, k, name)
            bad = np.flatnonzero(g != w)
            assert len(bad) == 0, (what, k, pen, name, bad[:5].tolist(), g[bad[:5]].tolist(),
                                   w[bad[:5]].tolist())
        assert int(got[0].sum()) == int(np.asarray(vectors[c]).sum(dtype=np.int64)), (what, k)
    return columns, stats


def check_loss_identity(pset, columns, stats, what=""):
    """total.loss of every problem recomputed from the sums: the rows' length * mean - sum *
    log(mean), where a row without reads contributes length * mean"""
    for k in range(len(pset.problems)):
        start, end, mean = columns[k]
        length = (end.astype(np.int64) - start.astype(np.int64)).astype(np.float64)
        s = stats[k][0].astype(np.float64)
        log_mean = np.log(np.where(s > 0, mean, 1.0))
        terms = length * mean - np.where(s > 0, s * log_mean, 0.0)
        total, scale = float(terms.sum()), float(np.abs(terms).sum())
        want = float(pset.loss(k)[6])
        print("%s problem %d: total.loss %.17g, from the sums %.17g, difference %.3g of %.6g = %.3g"
              % (what, k, want, total, abs(total - want), scale,
                 abs(total - want) / scale if scale else 0.0))
        assert abs(total - want) <= LOSS_TOL * scale, (what, k, total, want, scale)


# ---- scenario 1: tile boundaries ---------------------------------------------------------------

def tile_blocks(T):
    lengths = [T - 1, 2, 3 * T + 5, 1, T, T, 2 * T - 1, 64, 1, 63, T + 1]
    v = np.concatenate([(50 if k % 2 else 0) + (np.arange(n) % 2) for k, n in enumerate(lengths)])
    return lengths, v.astype(np.int32)


def scenario_tile_boundaries(psd, wrap):
    T = _lib().peakseg_hip_segment_stats_tile_runs()
    assert T >= 64
    lengths, v = tile_blocks(T)
    assert len(rle(v)[0]) == len(v) == 9 * T + 135          # every base is its own run
    vectors = [v, np.repeat(v, 3)]
    ends = np.cumsum(lengths)[::-1]
    pset = psd.ProblemSet.from_dense([wrap(x) for x in vectors], [(0, 20.0), (1, 20.0)])
    try:
        pset.solve()
        for firsts in (None, [1000, 7]):
            columns, stats = check_set(pset, vectors, firsts, "tile boundaries %r" % (firsts,))
            for k, scale in ((0, 1), (1, 3)):
                first = 0 if firsts is None else firsts[k]
                # the premise: the model's segments are the blocks
                assert columns[k][1].tolist() == (first + scale * ends).tolist(), (T, k)
                # ... so a block's summit is its second base (its only one in a block of one)
                begin = first + scale * (ends - np.array(lengths[::-1]))
                one = np.array(lengths[::-1]) == 1
                assert stats[k][1].tolist() == [50 * ((10 - r) % 2) + (0 if one[r] else 1)
                                                for r in range(11)]
                assert stats[k][2].tolist() == (begin + np.where(one, 0, scale)).tolist()
                assert stats[k][3].tolist() == (begin + np.where(one, 1, 2) * scale).tolist()
    finally:
        pset.close()


# ---- scenario 2: Mono27ac ----------------------------------------------------------------------

def scenario_mono27ac(psd, wrap):
    dense = mono27ac_dense()
    pens = [0.0, 1952.6, 10000.0, float("inf")]
    pset = psd.ProblemSet.from_dense([wrap(dense)], [(0, p) for p in pens])
    try:
        pset.solve()
        columns, stats = check_set(pset, [dense], [60000], "Mono27ac")
        assert len(stats[0][0]) == 6399 and len(stats[3][0]) == 1
        check_loss_identity(pset, columns, stats, "Mono27ac")
    finally:
        pset.close()


# ---- scenario 3: three contigs -----------------------------------------------------------------

def scenario_three_contigs(psd, wrap):
    vectors = three_contigs()
    pens = [0.5, 40.0, 3000.0, float("inf")]
    firsts = [1000, 0, 123456]
    problems = [(c, p) for c in range(3) for p in pens]
    pset = psd.ProblemSet.from_dense([wrap(x) for x in vectors], problems)
    try:
        pset.solve()
        columns, stats = check_set(pset, vectors, firsts, "three contigs")
        check_loss_identity(pset, columns, stats, "three contigs")
        for k in range(8, 12):      # the constant contig: one row, its summit the whole contig
            assert [a.tolist() for a in stats[k]] == [[4 * 777], [4], [123456], [123456 + 777]]
        for k in range(4, 8):       # the increasing contig: every row's summit is its last run
            assert np.array_equal(stats[k][3], columns[k][1])
    finally:
        pset.close()


# ---- scenario 4: 64-bit sums -------------------------------------------------------------------

def scenario_wide_sums(psd, wrap):
    """a product count * weight beyond 2^32, and sums beyond it across lanes, waves and tiles.  The
    long contig is solved at penalty Inf (one row over 70002 runs, no dynamic program), and it
    lies behind one run: its runs begin at no multiple of 16 bytes.  A third contig of five runs
    gives two rows of 4.9e9 reads each in a model of five rows."""
    a = np.array([0] * 10 + [70000, 69999] * 35000 + [0] * 10, np.int32)
    b = np.full(70000, 70000, np.int32)
    c = np.repeat(np.array([1, 70000, 1, 70000, 1], np.int32), 70000)
    assert 70000 * 70000 > 2 ** 32
    pset = psd.ProblemSet.from_dense([wrap(b), wrap(a), wrap(c)],
                                     [(0, 1000.0), (1, float("inf")), (2, 1000.0)])
    try:
        pset.solve()
        columns, stats = check_set(pset, [b, a, c], None, "64-bit sums")
        assert stats[0][0].tolist() == [70000 * 70000] and stats[0][1].tolist() == [70000]
        assert stats[1][0].tolist() == [35000 * 139999]
        assert [int(x[0]) for x in stats[1][1:]] == [70000, 10, 11]
        assert len(columns[2][0]) == 5
        assert stats[2][0].tolist() == [70000, 70000 * 70000, 70000, 70000 * 70000, 70000]
    finally:
        pset.close()


# ---- scenario 5: the contract ------------------------------------------------------------------

def scenario_contract(psd, wrap):
    lib = _lib()
    vectors = three_contigs()[:2]
    pset = psd.ProblemSet.from_dense([wrap(x) for x in vectors], [(0, 40.0), (1, 0.5)])
    try:
        none = [ctypes.c_void_p() for _ in range(4)]
        assert lib.peakseg_hip_problem_set_pack_segment_stats(
            pset._h, None, None, *[ctypes.byref(q) for q in none]) == -1     # not solved
        with pytest.raises(RuntimeError):
            pset.segment_stats()
        pset.solve()
        _, before = check_set(pset, vectors, [1000, 0], "contract")
        pset.set_penalty(0, 3000.0)
        with pytest.raises(RuntimeError):
            pset.segment_stats()                                             # not solved again yet
        pset.solve()
        out = [np.zeros(len(vectors[0]), dt) for dt in (np.int64, np.int32, np.int32, np.int32)]
        # solved again, not packed again: no old numbers
        assert lib.peakseg_hip_problem_set_packed_segment_stats_download(
            pset._h, *[a.ctypes.data for a in out]) == -1
        _, after = check_set(pset, vectors, [1000, 0], "contract, new penalty")
        assert len(after[0][0]) < len(before[0][0])
        assert all(np.array_equal(x, y) for x, y in zip(before[1], after[1]))
        with pytest.raises(RuntimeError, match="32-bit"):
            pset.segment_stats(first_chromStart=[2 ** 31 - 10, 0])
        ms = ctypes.c_float(-1.0)
        assert lib.peakseg_hip_segment_stats_last_ms(ctypes.byref(ms)) == 0 and ms.value >= 0.0
    finally:
        pset.close()
    count, weight, _ = rle(vectors[1])
    plain = psd.ProblemSet([(count, weight)], [(0, 40.0)])
    try:
        plain.solve()
        with pytest.raises(RuntimeError, match="dense"):
            plain.segment_stats()
    finally:
        plain.close()


def scenario_api(psd, wrap):
    vectors = three_contigs()[:2]
    pens = [[0.5, 3000, float("inf")], [40]]
    starts = [1000, 0]
    plain = psd.PeakSegFPOP_dense([wrap(v) for v in vectors], pens, chrom="chrT", chrom_starts=starts)
    fits = psd.PeakSegFPOP_dense([wrap(v) for v in vectors], pens, chrom="chrT", chrom_starts=starts,
                                 stats=True)
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors],
                                     [(c, float(p)) for c, q in enumerate(pens) for p in q])
    try:
        pset.solve()
        direct = pset.segment_stats(first_chromStart=starts)
    finally:
        pset.close()
    k = 0
    for c in range(2):
        for fit, bare in zip(fits[c], plain[c]):
            assert not hasattr(bare, "stats")
            assert fit.segments.equals(bare.segments)
            keep = [n for n in bare.loss.columns if n != "seconds"]
            assert fit.loss[keep].equals(bare.loss[keep])
            assert fit.coef().segments.equals(bare.coef().segments)
            assert list(fit.stats.columns) == ["reads", "max.count", "summitStart", "summitEnd"]
            assert len(fit.stats) == len(fit.segments)
            for name, col in zip(fit.stats.columns, direct[k]):
                assert np.array_equal(fit.stats[name].to_numpy(), col), (c, name)
            want = expected_stats(vectors[c], fit.segments["chromStart"].to_numpy(),
                                  fit.segments["chromEnd"].to_numpy(), starts[c])
            assert np.array_equal(fit.stats["reads"].to_numpy(), want[0])
            k += 1


def scenario_torch_device(psd, wrap):
    """the four tensors alias the packed buffers and hold what the download returns"""
    import torch
    dense = mono27ac_dense()
    pset = psd.ProblemSet.from_dense([wrap(dense)], [(0, 1952.6), (0, 0.0)])
    try:
        pset.solve()
        stats = pset.segment_stats(first_chromStart=[60000])
        offs, t_sum, t_max, t_s0, t_s1 = pset.segment_stats(first_chromStart=[60000],
                                                            torch_device="cuda:0")
        ptr = [ctypes.c_void_p() for _ in range(4)]
        first = (ctypes.c_int * 1)(60000)
        total = _lib().peakseg_hip_problem_set_pack_segment_stats(
            pset._h, first, None, *[ctypes.byref(q) for q in ptr])
        assert [t.data_ptr() for t in (t_sum, t_max, t_s0, t_s1)] == [q.value for q in ptr]
        assert total == len(t_sum) == offs[-1] and t_sum.device.type == "cuda"
        assert [t.dtype for t in (t_sum, t_max, t_s0, t_s1)] == \
            [torch.int64, torch.int32, torch.int32, torch.int32]
        kept = [t.cpu().numpy() for t in (t_sum, t_max, t_s0, t_s1)]
    finally:
        pset.close()
    for k in (0, 1):
        for got, want in zip(kept, stats[k]):
            assert np.array_equal(got[int(offs[k]):int(offs[k + 1])], want)


SCENARIOS = [scenario_tile_boundaries, scenario_mono27ac, scenario_three_contigs,
             scenario_wide_sums, scenario_contract, scenario_api]


# ---- MI355X ------------------------------------------------------------------------------------

_CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process
sys.path[:0] = [%(root)r, %(tests)r]
import test_gpu_segment_stats as gs
gs.child_main()
print("stats-child ok")
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
def test_gpu_segment_stats_numpy(psd, scenario):
    scenario(psd, as_numpy)


@GPU
def test_gpu_segment_stats_cuda_tensors(psd):
    """every scenario again from cuda tensors, and the torch_device form of segment_stats()"""
    import sys
    from conftest import ROOT
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(p.stdout[-4000:])
    assert p.returncode == 0 and "stats-child ok" in p.stdout, p.stdout[-3000:] + p.stderr[-6000:]
