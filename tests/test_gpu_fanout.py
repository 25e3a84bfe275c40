"""PEAKSEG_HIP_DEVICES on the MI355X: the batch entry points spread over several problem sets in
one process -- one per listed device, each on a host thread of its own -- and leave exactly the
files, statuses and search rows of the call without the knob (_timing.tsv's seconds excepted).

A listed device may repeat ("0,0": two sets, one after the other), which is how the fan-out runs
on a box with one GPU; "all" is every visible device.  The scenario functions are shared with the
emulator rehearsal (tests/test_fanout_cpu.py) at smaller sizes."""
import ctypes
import os
import shutil
import threading

import pytest

from conftest import GOLDEN, read_loss, read_segments

MONO = os.path.join(GOLDEN, "Mono27ac.bedGraph")
SIX_POINTS = [(0, 1, 3), (1, 2, 9), (2, 3, 18), (3, 4, 15), (4, 5, 20), (5, 6, 2)]


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


def _set_knob(devices):
    if devices is None:
        os.environ.pop("PEAKSEG_HIP_DEVICES", None)
    else:
        os.environ["PEAKSEG_HIP_DEVICES"] = devices


def outputs(root):
    """every file under root: bytes, a cost-function database by its size only, a _timing.tsv
    (whose seconds differ from run to run) by its existence only"""
    out = {}
    for dirpath, _, files in os.walk(root):
        for f in files:
            path = os.path.join(dirpath, f)
            rel = os.path.relpath(path, root)
            if f.endswith(".db"):
                out[rel] = os.path.getsize(path)
            elif f.endswith("_timing.tsv"):
                out[rel] = "timing"
            else:
                with open(path, "rb") as fh:
                    out[rel] = fh.read()
    return out


def _bins(path):
    with open(path) as f:
        return sum(1 for line in f if line.strip())


def expected_shard_of(entries, n_shards):
    """The dealing PEAKSEG_HIP_DEVICES promises, computed with parallel.shard_problems over
    parallel.predicted_cost's default ramp: the device programs are the entries' distinct
    (file, penalty) pairs that need the dynamic program, in order of first appearance."""
    from peaksegdisk_amd import parallel
    prog_of, programs, entry_prog = {}, [], []
    for bg, pen in entries:
        if pen == "Inf" or not os.path.exists(bg):
            entry_prog.append(-1)
            continue
        key = (bg, pen)
        if key not in prog_of:
            prog_of[key] = len(programs)
            programs.append((_bins(bg), float(pen)))
        entry_prog.append(prog_of[key])
    distinct = sorted(set(p for _, p in programs))
    costs = [parallel.predicted_cost(b, distinct.index(p), len(distinct)) for b, p in programs]
    shard_of_prog = {}
    for s, progs in enumerate(parallel.shard_problems(costs, n_shards)):
        for k in progs:
            shard_of_prog[k] = s
    return [shard_of_prog[k] if k >= 0 else -1 for k in entry_prog], len(programs)


def file_batch_entries(root, mono_pens, n_synth, synth_bins, synth_pens):
    """Mono27ac x mono_pens, n_synth synthetic contigs x synth_pens, an Inf entry, the first
    entry once more and a missing file"""
    from peaksegdisk_amd import synthetic
    os.makedirs(root)
    mono = os.path.join(root, "mono.bedGraph")
    shutil.copy(MONO, mono)
    entries = [(mono, p) for p in mono_pens]
    for c in range(n_synth):
        cs, ce, cnt = synthetic.poisson_coverage(synth_bins, seed=60 + c)
        bg = os.path.join(root, "synth%d.bedGraph" % c)
        synthetic.write_bedgraph(bg, cs, ce, cnt)
        entries += [(bg, p) for p in synth_pens]
    entries.insert(1, (mono, "Inf"))
    entries.append(entries[0])
    entries.append((os.path.join(root, "missing.bedGraph"), "10"))
    return entries


def disk_batch(entries):
    n = len(entries)
    bgs = (ctypes.c_char_p * n)(*[os.fsencode(b) for b, _ in entries])
    pens = (ctypes.c_char_p * n)(*[p.encode() for _, p in entries])
    dbs = (ctypes.c_char_p * n)(*[os.fsencode("%s_penalty=%s.db" % e) for e in entries])
    status = (ctypes.c_int * n)()
    _lib().PeakSegFPOP_disk_batch(n, bgs, pens, dbs, status)
    return list(status)


def scenario_file_batch(oracle_det, tmp_path, devices, n_shards, mono_pens, n_synth, synth_bins,
                        synth_pens):
    from peaksegdisk_amd import _native
    base = os.path.join(str(tmp_path), "unset")
    fan = os.path.join(str(tmp_path), "fanout")
    e_base = file_batch_entries(base, mono_pens, n_synth, synth_bins, synth_pens)
    e_fan = file_batch_entries(fan, mono_pens, n_synth, synth_bins, synth_pens)
    _set_knob(None)
    st_base = disk_batch(e_base)
    assert _native.last_fanout()["device"] == []
    _set_knob(devices)
    try:
        st_fan = disk_batch(e_fan)
    finally:
        _set_knob(None)
    report = _native.last_fanout()
    assert st_fan == st_base
    assert st_base[-1] == 3 and st_base[1] == 0 and set(st_base[:-1]) == {0}, st_base
    assert outputs(fan) == outputs(base)
    shard_of, n_programs = expected_shard_of(e_fan, n_shards)
    assert report["device"] == (list(range(n_shards)) if devices == "all" else
                                [int(d) for d in devices.split(",")])
    assert sum(report["programs"]) == n_programs
    assert report["shard_of"] == shard_of
    assert all(s >= 0 for s in report["seconds"])
    # two of the problems against the CPU oracle
    odir = os.path.join(str(tmp_path), "oracle")
    os.makedirs(odir)
    for (bg, pen) in (e_fan[0], e_fan[-3]):
        obg = os.path.join(odir, os.path.basename(bg))
        shutil.copy(bg, obg)
        assert oracle_det.solve(obg, pen) == 0
        for suffix in ("_segments.bed", "_loss.tsv"):
            a = "%s_penalty=%s%s" % (bg, pen, suffix)
            b = "%s_penalty=%s%s" % (obg, pen, suffix)
            assert open(a, "rb").read() == open(b, "rb").read(), (a, b)
    return report


def _problem_dirs(root, specs):
    """specs: (name, n_bins or None for Mono27ac or "six" for the six points, seed)"""
    from peaksegdisk_amd import synthetic
    dirs = []
    for name, n_bins, seed in specs:
        d = os.path.join(root, name)
        os.makedirs(d)
        bg = os.path.join(d, "coverage.bedGraph")
        if n_bins is None:
            shutil.copy(MONO, bg)
        elif n_bins == "six":
            with open(bg, "w") as f:
                f.write("".join("chr1\t%d\t%d\t%d\n" % r for r in SIX_POINTS))
        else:
            cs, ce, cnt = synthetic.poisson_coverage(n_bins, seed=seed)
            synthetic.write_bedgraph(bg, cs, ce, cnt)
        dirs.append(d)
    return dirs


def scenario_dir_batch(psd, tmp_path, devices, n_shards, specs, pens):
    """Python's PeakSegFPOP_dir_batch with devices=..., run twice: the first run leaves the
    files of the call without the knob, its _timing.tsv seconds add up to the same wall time on
    every shard; the second is served from the cache and deals nothing."""
    from peaksegdisk_amd import _native
    base = _problem_dirs(os.path.join(str(tmp_path), "unset"), specs)
    fan = _problem_dirs(os.path.join(str(tmp_path), "fanout"), specs)
    pairs = [(k, p) for k in range(len(specs)) for p in pens] + [(0, "Inf")]
    assert "PEAKSEG_HIP_DEVICES" not in os.environ
    fits_base = psd.PeakSegFPOP_dir_batch([base[k] for k, _ in pairs], [p for _, p in pairs])
    fits = psd.PeakSegFPOP_dir_batch([fan[k] for k, _ in pairs], [p for _, p in pairs],
                                     devices=devices)
    assert "PEAKSEG_HIP_DEVICES" not in os.environ  # restored
    report = _native.last_fanout()
    assert not any(f.cached for f in fits + fits_base)
    assert outputs(os.path.join(str(tmp_path), "fanout")) == \
        outputs(os.path.join(str(tmp_path), "unset"))
    assert len(report["device"]) == n_shards and sum(report["programs"]) == len(pairs) - 1
    shard_of = report["shard_of"]
    assert len(shard_of) == len(pairs) and shard_of[-1] == -1
    assert all(0 <= s < n_shards for s in shard_of[:-1])
    # each shard's seconds (and those of the one entry no shard solved) add up to the wall time
    sums = {}
    for (k, p), s in zip(pairs, shard_of):
        with open("%s/coverage.bedGraph_penalty=%s_timing.tsv" % (fan[k], p)) as f:
            sums[s] = sums.get(s, 0.0) + float(f.read().split("\t")[2])
    assert len(sums) >= 2
    assert max(sums.values()) - min(sums.values()) <= 1e-9 * max(sums.values()), sums
    # again: every pair is a cache hit, no shard solves anything
    again = psd.PeakSegFPOP_dir_batch([fan[k] for k, _ in pairs], [p for _, p in pairs],
                                      devices=devices)
    assert all(f.cached for f in again)
    report = _native.last_fanout()
    assert report["shard_of"] == [-1] * len(pairs) and report["device"] == []
    for a, b in zip(fits, again):
        assert a.segments.equals(b.segments)


ROW_FIELDS = ["penalty_str", "penalty", "total_loss", "peaks", "segments", "bases", "iteration",
              "under_peaks", "over_peaks", "cached"]


def _search_batch(dirs, targets, verbose):
    from peaksegdisk_amd import _native
    n, cap = len(dirs), 64
    rows = (_native.PsdSearchRow * (cap * n))()
    n_rows = (ctypes.c_int * n)()
    chosen = (ctypes.c_int * n)()
    status = (ctypes.c_int * n)()
    _lib().PeakSegFPOP_sequential_search_batch(
        n, (ctypes.c_char_p * n)(*[os.fsencode(d) for d in dirs]), (ctypes.c_int * n)(*targets),
        verbose, cap, rows, n_rows, chosen, status)
    table = [[tuple(getattr(rows[d * cap + k], f) for f in ROW_FIELDS) for k in range(n_rows[d])]
             for d in range(n)]
    return table, list(n_rows), list(chosen), list(status)


PRINT_FN = ctypes.CFUNCTYPE(None, ctypes.c_char_p)


def _with_print(fn):
    """fn() with the library's text going to a ctypes callback: (result, [(native thread id,
    text)])"""
    got = []
    cb = PRINT_FN(lambda text: got.append((threading.get_native_id(), text.decode())))
    _lib().peakseg_hip_set_print(ctypes.cast(cb, ctypes.c_void_p))
    try:
        return fn(), got
    finally:
        _lib().peakseg_hip_set_print(None)


def _lines_by_dir(got):
    """the verbose lines ("<dir>: Next = ...") per directory name, in their order"""
    per = {}
    for line in "".join(t for _, t in got).splitlines():
        d, rest = line.split(": ", 1)
        per.setdefault(os.path.basename(d), []).append(rest)
    return per


def scenario_search(psd, tmp_path, devices, n_shards, specs, targets):
    from peaksegdisk_amd import _native
    base = _problem_dirs(os.path.join(str(tmp_path), "unset"), specs)
    fan = _problem_dirs(os.path.join(str(tmp_path), "fanout"), specs)
    _set_knob(None)
    r_base, got_base = _with_print(lambda: _search_batch(base, targets, 1))
    _set_knob(devices)
    try:
        r_fan, got_fan = _with_print(lambda: _search_batch(fan, targets, 1))
    finally:
        _set_knob(None)
    report = _native.last_fanout()
    assert r_fan == r_base
    assert r_base[3] == [0] * len(specs) and all(c >= 0 for c in r_base[2])
    assert outputs(os.path.join(str(tmp_path), "fanout")) == \
        outputs(os.path.join(str(tmp_path), "unset"))
    me = threading.get_native_id()
    assert got_fan and {t for t, _ in got_fan} == {me}
    assert _lines_by_dir(got_fan) == _lines_by_dir(got_base)
    assert len(report["device"]) == n_shards
    assert len(report["shard_of"]) == len(specs)
    assert all(0 <= s < n_shards for s in report["shard_of"])
    # the Python entry with devices=: everything is cached now, same choices
    fits = psd.sequentialSearch_dir_batch(fan, targets, devices=devices)
    for d, fit in enumerate(fits):
        row = r_base[0][d][r_base[2][d]]
        assert int(fit.loss["peaks"].iloc[0]) == row[3]
    assert "PEAKSEG_HIP_DEVICES" not in os.environ
    # the six points with target 2 (the reference's example): 2 peaks
    six = [k for k, s in enumerate(specs) if s[1] == "six"]
    for k in six:
        assert r_base[0][k][r_base[2][k]][3] == 2
    return report


def scenario_bad_device(tmp_path, bad):
    """an id that is not visible: the dynamic programs get status 12 and the message names it;
    the trivial model is still written; nothing is dealt"""
    from peaksegdisk_amd import _native
    root = os.path.join(str(tmp_path), "bad")
    os.makedirs(root)
    bg = os.path.join(root, "coverage.bedGraph")
    with open(bg, "w") as f:
        f.write("chr1\t0\t10\t2\nchr1\t10\t20\t10\nchr1\t20\t30\t14\n")
    _set_knob(str(bad))
    try:
        st = disk_batch([(bg, "10.5"), (bg, "Inf")])
        msg = _native.last_error()
        report = _native.last_fanout()
        single = _lib().PeakSegFPOP_disk(os.fsencode(bg), b"3", os.fsencode(bg + ".db"))
    finally:
        _set_knob(None)
    assert st == [_native.ERROR_NO_HIP_DEVICE, 0]
    assert "device %d" % bad in msg and "%d HIP devices visible" % _lib().peakseg_hip_device_count() in msg
    assert report == {"device": [], "programs": [], "seconds": [], "shard_of": [-1, -1]}
    assert single == _native.ERROR_NO_HIP_DEVICE
    assert read_segments(bg + "_penalty=Inf_segments.bed")[0][3] == "background"
    assert read_loss(bg + "_penalty=Inf_loss.tsv").split("\t")[:3] == ["Inf", "1", "0"]


# ---- on the MI355X ------------------------------------------------------------------------

def _gpu_pens():
    from peaksegdisk_amd import synthetic
    return ["1952.6"] + synthetic.penalty_grid(12, 0.0, 5.0), synthetic.penalty_grid(8, 0.0, 5.0)


@pytest.mark.gpu
@pytest.mark.parametrize("devices", ["0,0", "all"])
def test_file_batch_fanout(psd, oracle_det, tmp_path, devices):
    n_shards = 2 if devices == "0,0" else _lib().peakseg_hip_device_count()
    mono_pens, synth_pens = _gpu_pens()
    scenario_file_batch(oracle_det, tmp_path, devices, n_shards, mono_pens, 4, 50000, synth_pens)


@pytest.mark.gpu
@pytest.mark.parametrize("devices", ["0,0", "all"])
def test_dir_batch_fanout_then_cache(psd, tmp_path, devices):
    n_shards = 2 if devices == "0,0" else _lib().peakseg_hip_device_count()
    specs = [("mono", None, 0), ("s1", 50000, 71), ("s2", 30000, 72), ("s3", 40000, 73)]
    from peaksegdisk_amd import synthetic
    scenario_dir_batch(psd, tmp_path, devices, n_shards, specs, synthetic.penalty_grid(6, 0.0, 5.0))


@pytest.mark.gpu
@pytest.mark.parametrize("devices", ["0,0", "all"])
def test_search_batch_fanout(psd, tmp_path, devices):
    n_shards = 2 if devices == "0,0" else _lib().peakseg_hip_device_count()
    specs = [("mono", None, 0), ("six", "six", 0), ("s1", 20000, 81), ("s2", 15000, 82)]
    scenario_search(psd, tmp_path, devices, n_shards, specs, [19, 2, 7, 3])


@pytest.mark.gpu
def test_device_id_equal_to_the_count(psd, tmp_path):
    scenario_bad_device(tmp_path, _lib().peakseg_hip_device_count())
