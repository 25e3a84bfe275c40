"""The latency kernel's inner loop of the usual data point (fpop_kernels.h): the transitions in
and out of it, the edges of the 64-point data block, and parking from inside it.

Every case runs on the SIMT emulator (CPU) and, marked gpu, on the device, against the oracle.
A build with -DPSD_LOOP_STATS counts, per chain wave, the data points taken inside the inner
loop, those taken by the general code, and the entries into the inner loop; the product build
has no such counters."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT

GPU = pytest.mark.gpu
EMU_DIR = os.path.join(ROOT, "tests", "emu")
RAMP_PENALTIES = ["0.1", "100", "10000"]
RAMP_N, RAMP_PREFIX = 640, 456
EDGE_LENGTHS = [2, 3, 63, 64, 65, 129, 130]
EDGE_PENALTIES = ["0.1", "1000"]


# ---- the libraries -------------------------------------------------------------------------

def _declare(path):
    import peaksegdisk_amd  # noqa: F401  (the package needs its own library to import)
    from peaksegdisk_amd import _native
    return _native.declare(ctypes.CDLL(path))


@pytest.fixture(scope="module")
def emu_libs():
    """(product source on the emulator, the same with -DPSD_LOOP_STATS, and with every step of
    the specialised path forced to report a rare argument as well)"""
    import __graft_entry__ as entry
    entry.build_hip()
    subprocess.run(["make", "-s", "-C", EMU_DIR], check=True)
    libs = [_declare(os.path.join(EMU_DIR, "_build", "libpeaksegdisk_emu.so"))]
    for sub, flags in (("loop_stats", "-DPSD_LOOP_STATS"),
                       ("loop_stats_rare", "-DPSD_LOOP_STATS -DPSD_FORCE_RARE")):
        out = os.path.join("_build", sub)
        subprocess.run(["make", "-s", "-C", EMU_DIR, "CXX=%s %s" % (os.environ.get("CXX", "g++"), flags),
                        "OUT=" + out, os.path.join(out, "libpeaksegdisk_emu.so")], check=True)
        libs.append(_declare(os.path.join(EMU_DIR, out, "libpeaksegdisk_emu.so")))
    return tuple(libs)


@pytest.fixture(scope="module")
def gpu_libs(tmp_path_factory):
    """(the product library, a -DPSD_LOOP_STATS build of it)"""
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd  # noqa: F401
    from peaksegdisk_amd import _native
    assert _native.lib.peakseg_hip_device_count() >= 1, "no HIP device: GPU tests need an MI355X"
    out = str(tmp_path_factory.mktemp("loop_stats") / "libpeaksegdisk_hip_loop_stats.so")
    subprocess.run(["bash", os.path.join(ROOT, "tools", "build_variant.sh"), ROOT, out,
                    "-DPSD_LOOP_STATS"], check=True)
    return _native.lib, _declare(out)


@pytest.fixture(autouse=True)
def _latency_build(monkeypatch):
    monkeypatch.setenv("PEAKSEG_HIP_VARIANT", "lat")  # the inner loop is the latency build's


# ---- data and the oracle's answers, computed once -------------------------------------------

def _write_bedgraph(path, cnt):
    with open(path, "w") as f:
        f.write("".join("chrSynth\t%d\t%d\t%d\n" % (i, i + 1, c) for i, c in enumerate(cnt)))


def _loss_fields(bg, pen):
    return open("%s_penalty=%s_loss.tsv" % (bg, pen)).read().rstrip("\n").split("\t")


@pytest.fixture(scope="module")
def ramp(oracle_det, tmp_path_factory):
    """Counts 1..200, then 440 small counts: the functions grow past the fast sizes during the
    ramp (at the two larger penalties) and come back to a few pieces after it.  The oracle's own
    output says so before anything is compared with it."""
    rng = random.Random(3)
    cnt = list(range(1, 201)) + [rng.choice([0, 1, 1, 2, 2, 3, 4, 8, 9, 2, 1]) for _ in range(440)]
    assert len(cnt) == RAMP_N
    d = tmp_path_factory.mktemp("ramp")
    bg, bg_prefix = str(d / "coverage.bedGraph"), str(d / "prefix.bedGraph")
    _write_bedgraph(bg, cnt)
    _write_bedgraph(bg_prefix, cnt[:RAMP_PREFIX])
    for pen in RAMP_PENALTIES:
        assert oracle_det.solve(bg, pen) == 0
        full = _loss_fields(bg, pen)
        mean_all, max_all = float(full[8]), int(full[9])
        if pen == "0.1":
            assert max_all <= 16  # never leaves the fast sizes
            continue
        assert 32 < max_all <= 128  # leaves them, stays within the LDS lists
        # (the recurrence is causal: a prefix run gives the same functions)
        assert oracle_det.solve(bg_prefix, pen) == 0
        mean_prefix = float(_loss_fields(bg_prefix, pen)[8])
        tail = (RAMP_N * mean_all - RAMP_PREFIX * mean_prefix) / (RAMP_N - RAMP_PREFIX)
        assert tail < 10  # back at a few pieces: the inner loop is entered again
    return np.array(cnt, dtype=np.int32), bg


@pytest.fixture(scope="module")
def edges(oracle_det, tmp_path_factory):
    """Poisson counts of lengths around the 64-point data block, the oracle's files and stores"""
    from peaksegdisk_amd import synthetic
    d = tmp_path_factory.mktemp("edges")
    out = []
    for n in EDGE_LENGTHS:
        seed = 100 + n
        cs, ce, cnt = synthetic.poisson_coverage(n, seed=seed)
        while cnt.min() == cnt.max():  # (constant data has no dynamic program: the next seed)
            seed += 1000
            cs, ce, cnt = synthetic.poisson_coverage(n, seed=seed)
        bg = str(d / ("n%d.bedGraph" % n))
        synthetic.write_bedgraph(bg, cs, ce, cnt)
        for pen in EDGE_PENALTIES:
            assert oracle_det.solve(bg, pen) == 0
        out.append((cnt, (ce - cs).astype(np.int32), ce, bg))
    return out


@pytest.fixture(scope="module")
def park_case(oracle_det, tmp_path_factory):
    from peaksegdisk_amd import synthetic
    d = tmp_path_factory.mktemp("park")
    cs, ce, cnt = synthetic.poisson_coverage(2000, seed=5)
    bg = str(d / "coverage.bedGraph")
    synthetic.write_bedgraph(bg, cs, ce, cnt)
    assert oracle_det.solve(bg, "7") == 0
    assert int(_loss_fields(bg, "7")[9]) <= 16  # every data point from 2 on is a usual one
    return cnt, (ce - cs).astype(np.int32), ce, bg


# ---- the checks, for either device ----------------------------------------------------------

def _files_equal_oracle(lib, bg, pen, tmp_path, tag):
    """PeakSegFPOP_disk of `lib` on a copy of bg: segments.bed and loss.tsv byte for byte"""
    mine = str(tmp_path / ("%s_%s" % (tag, os.path.basename(bg))))
    with open(bg, "rb") as src, open(mine, "wb") as dst:
        dst.write(src.read())
    st = lib.PeakSegFPOP_disk(os.fsencode(mine), pen.encode(),
                              os.fsencode("%s_penalty=%s.db" % (mine, pen)))
    assert st == 0, (tag, pen, st)
    for suffix in ("_segments.bed", "_loss.tsv"):
        got = open("%s_penalty=%s%s" % (mine, pen, suffix), "rb").read()
        want = open("%s_penalty=%s%s" % (bg, pen, suffix), "rb").read()
        assert got == want, (tag, pen, suffix)


def _store_equals_oracle(pset, i, ce, bg, pen, tmp_path, tag):
    got = str(tmp_path / ("%s_%d.db" % (tag, i)))
    pset.export_db(i, ce, got)
    assert open(got, "rb").read() == open("%s_penalty=%s.db" % (bg, pen), "rb").read(), (tag, pen)


def _loop_stats(lib, pset, p):
    out = (ctypes.c_int * 6)()
    n = lib.peakseg_hip_problem_set_loop_stats(pset._h, p, out)
    return n, [list(out[0:3]), list(out[3:6])]  # per chain: inside, general, entries


def check_transitions(lib, stats_lib, ramp, tmp_path, rare_lib=None):
    from peaksegdisk_amd import ProblemSet
    cnt, bg = ramp
    w = np.ones(RAMP_N, dtype=np.int32)
    ce = np.arange(1, RAMP_N + 1, dtype=np.int32)
    problems = [(0, float(p)) for p in RAMP_PENALTIES]
    for pen in RAMP_PENALTIES:
        _files_equal_oracle(lib, bg, pen, tmp_path, "files")
    for tag, which in (("product", lib), ("stats", stats_lib), ("rare", rare_lib)):
        if which is None:
            continue
        pset = ProblemSet([(cnt, w)], problems, lib=which)
        pset.solve()
        assert pset.kernel_build == "lat"
        for i, pen in enumerate(RAMP_PENALTIES):
            assert pset.result(i).status == 0
            _store_equals_oracle(pset, i, ce, bg, pen, tmp_path, tag)
            n, per_chain = _loop_stats(which, pset, i)
            if tag == "product":
                assert n == 0 and per_chain == [[0, 0, 0], [0, 0, 0]]  # no counters there
                continue
            assert n == 6
            for inside, general, entries in per_chain:
                assert inside + general == RAMP_N
                if tag == "rare":  # every data point leaves the inner loop
                    assert inside == 0 and general == RAMP_N
                elif pen == "0.1":  # every data point from 2 on is inside, in one entry
                    assert (inside, general, entries) == (RAMP_N - 2, 2, 1)
                else:  # out during the ramp, in again after it
                    assert inside > 0 and general > 2 and entries >= 2
        pset.close()


def check_edges(lib, edges, tmp_path):
    from peaksegdisk_amd import ProblemSet
    problems = [(k, float(p)) for k in range(len(edges)) for p in EDGE_PENALTIES]
    pset = ProblemSet([(cnt, w) for cnt, w, _, _ in edges], problems, lib=lib)
    pset.solve()
    assert pset.kernel_build == "lat"
    for i, (k, _) in enumerate(problems):
        pen = EDGE_PENALTIES[i % len(EDGE_PENALTIES)]
        cnt, w, ce, bg = edges[k]
        assert pset.result(i).status == 0
        _store_equals_oracle(pset, i, ce, bg, pen, tmp_path, "edge")
        _files_equal_oracle(lib, bg, pen, tmp_path, "edge%d" % i)
    pset.close()


def check_parking(stats_lib, park_case, tmp_path, monkeypatch):
    """An arena far too small, as in test_arena_regrowth_resumes_instead_of_repeating: the
    problem parks inside the inner loop and resumes at that data point, inside a data block."""
    from peaksegdisk_amd import ProblemSet
    cnt, w, ce, bg = park_case
    n = len(cnt)
    monkeypatch.setenv("PEAKSEG_HIP_NO_CHECKPOINT", "1")
    monkeypatch.setenv("PEAKSEG_HIP_PIECES_PER_FUNCTION", "1")
    monkeypatch.setenv("PEAKSEG_HIP_NO_LIVE_GROWTH", "1")
    monkeypatch.setenv("PEAKSEG_HIP_ARENA_BLOCK_LOG2", "12")
    pset = ProblemSet([(cnt, w)], [(0, 7.0)], lib=stats_lib)
    pset.solve()
    launches, steps = pset.solve_stats
    assert launches >= 2, "the arena was never exhausted"
    assert steps == n, (launches, steps)  # nothing computed twice
    assert pset.result(0).status == 0
    got, per_chain = _loop_stats(stats_lib, pset, 0)
    assert got == 6
    for inside, general, entries in per_chain:  # the last launch
        resumed_at = n - (inside + general)
        assert resumed_at >= 2 and resumed_at % 64 != 0, resumed_at
        assert general == 0 and entries == 1  # it went on inside the inner loop
    _store_equals_oracle(pset, 0, ce, bg, "7", tmp_path, "park")
    pset.close()


# ---- on the emulator ------------------------------------------------------------------------

def test_emu_transitions_in_and_out_of_the_inner_loop(emu_libs, ramp, tmp_path):
    check_transitions(emu_libs[0], emu_libs[1], ramp, tmp_path, rare_lib=emu_libs[2])


def test_emu_edges_of_the_data_block(emu_libs, edges, tmp_path):
    check_edges(emu_libs[0], edges, tmp_path)


def test_emu_parking_from_inside_the_inner_loop(emu_libs, park_case, tmp_path, monkeypatch):
    check_parking(emu_libs[1], park_case, tmp_path, monkeypatch)


# ---- on the device --------------------------------------------------------------------------

@GPU
def test_transitions_in_and_out_of_the_inner_loop(gpu_libs, ramp, tmp_path):
    check_transitions(gpu_libs[0], gpu_libs[1], ramp, tmp_path)


@GPU
def test_edges_of_the_data_block(gpu_libs, edges, tmp_path):
    check_edges(gpu_libs[0], edges, tmp_path)


@GPU
def test_parking_from_inside_the_inner_loop(gpu_libs, park_case, tmp_path, monkeypatch):
    check_parking(gpu_libs[1], park_case, tmp_path, monkeypatch)
