"""The parallel penalty search (PeakSegFPOP_parallel_search / parallelSearch_dir): `width` models
per round, every round in one launch.

The scenario functions are shared with the emulator rehearsal (tests/test_parallel_search_emu.py),
which runs them without a GPU; the tests marked gpu run them on the MI355X, together with the
cases that are too long for the emulator (Mono27ac's 3198 peaks, the 5e5-bin contig of the
sequential suite, the fan-out over the box's device list).

What a search must satisfy is checked by replaying its rows (check_rules): the first row of every
round after the first is the reference's secant penalty of the bracket at the round's start, every
other row lies strictly inside that bracket, no penalty string is asked for twice, no round is
wider than `width`, and the chosen model never has more peaks than asked."""
import ctypes
import os
import shutil
import threading
import time

import pytest

from conftest import GOLDEN, read_segments

import test_gpu_round2 as gp2

GPU = pytest.mark.gpu
ROW_FIELDS = ["penalty_str", "penalty", "total_loss", "peaks", "segments", "bases", "iteration",
              "under_peaks", "over_peaks"]


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


def mono_dir(root, name):
    d = root / name / "chr11-60000-580000"
    d.mkdir(parents=True)
    shutil.copy(os.path.join(GOLDEN, "Mono27ac.bedGraph"), str(d / "coverage.bedGraph"))
    return str(d)


def _row_dict(r):
    d = {f: getattr(r, f) for f in ROW_FIELDS}
    d["penalty_str"] = r.penalty_str.decode()
    d["cached"] = r.cached
    return d


def native_search(problem_dir, target, width, capacity=1024, sequential=False):
    """-> (status, rows as dicts, chosen row index) of one native search"""
    from peaksegdisk_amd import _native
    rows = (_native.PsdSearchRow * capacity)()
    n = ctypes.c_int(-1)
    chosen = ctypes.c_int(0)
    if sequential:
        st = _lib().PeakSegFPOP_sequential_search(os.fsencode(problem_dir), target, 0, capacity,
                                                  rows, ctypes.byref(n), ctypes.byref(chosen))
    else:
        st = _lib().PeakSegFPOP_parallel_search(os.fsencode(problem_dir), target, width, 0,
                                                capacity, rows, ctypes.byref(n),
                                                ctypes.byref(chosen))
    return st, [_row_dict(rows[k]) for k in range(max(n.value, 0))], chosen.value


def native_search_batch(problem_dirs, targets, width, capacity=1024):
    from peaksegdisk_amd import _native
    n = len(problem_dirs)
    rows = (_native.PsdSearchRow * (capacity * n))()
    dirs = (ctypes.c_char_p * n)(*[os.fsencode(d) for d in problem_dirs])
    peaks = (ctypes.c_int * n)(*targets)
    n_rows = (ctypes.c_int * n)()
    chosen = (ctypes.c_int * n)()
    status = (ctypes.c_int * n)()
    st = _lib().PeakSegFPOP_parallel_search_batch(n, dirs, peaks, width, 0, capacity, rows, n_rows,
                                                  chosen, status)
    return st, [([_row_dict(rows[d * capacity + k]) for k in range(n_rows[d])], chosen[d],
                 status[d]) for d in range(n)]


def same_rows(a, b):
    return [[r[f] for f in ROW_FIELDS] for r in a] == [[r[f] for f in ROW_FIELDS] for r in b]


def check_rules(psd, rows, chosen, target, width):
    """Replay the rows of a parallel search against the rules of a round.  Returns the number of
    rounds."""
    NA = -2 ** 31
    strings = [r["penalty_str"] for r in rows]
    assert len(set(strings)) == len(strings), "a penalty string was asked for twice"
    rounds = max(r["iteration"] for r in rows)
    by_round = [[r for r in rows if r["iteration"] == it] for it in range(1, rounds + 1)]
    assert [r["iteration"] for r in rows] == sorted(r["iteration"] for r in rows)
    assert [r["penalty_str"] for r in by_round[0]] == ["0", "Inf"]
    assert all(r["under_peaks"] == NA and r["over_peaks"] == NA for r in by_round[0])
    over, under = by_round[0]
    for models in by_round[1:]:
        assert 1 <= len(models) <= width
        secant = (over["total_loss"] - under["total_loss"]) / (under["peaks"] - over["peaks"])
        assert secant >= 0
        assert models[0]["penalty_str"] == psd.paste(secant)
        for m in models:
            assert (m["under_peaks"], m["over_peaks"]) == (under["peaks"], over["peaks"])
        for m in models[1:]:
            assert over["penalty"] < m["penalty"] < under["penalty"]
            assert m["penalty"] == float(m["penalty_str"])
        if models is by_round[-1]:
            break
        # the bracket the next round starts from: the secant model as the reference places its
        # one model, every other model where it narrows the bracket and keeps it ordered
        assert all(m["peaks"] != target for m in models)
        first = models[0]
        assert first["peaks"] not in (under["peaks"], over["peaks"])
        if first["peaks"] < target:
            under = first
        else:
            over = first
        for m in models[1:]:
            if m["peaks"] < target:
                closer = m["peaks"] > under["peaks"] or (
                    m["peaks"] == under["peaks"] and m["penalty"] < under["penalty"])
                if closer and m["penalty"] > over["penalty"]:
                    under = m
            else:
                closer = m["peaks"] < over["peaks"] or (
                    m["peaks"] == over["peaks"] and m["penalty"] > over["penalty"])
                if closer and m["penalty"] < under["penalty"]:
                    over = m
    # the end: a model with the target (the one with the largest penalty), else `under`
    assert 0 <= chosen < len(rows)
    assert rows[chosen]["peaks"] <= target
    hits = [r for r in rows if r["peaks"] == target]
    if hits:
        last_hits = [r for r in by_round[-1] if r["peaks"] == target]
        assert last_hits and rows[chosen]["penalty"] == max(r["penalty"] for r in last_hits)
    elif rounds > 1:
        assert rows[chosen]["peaks"] == max(r["peaks"] for r in rows if r["peaks"] < target)
    return rounds


def check_files_against_oracle(oracle, problem_dir, oracle_dir, rows):
    """every model's _segments.bed and _loss.tsv: the oracle's bytes at that penalty string; its
    _timing.tsv: one row of three fields"""
    bg, obg = (os.path.join(d, "coverage.bedGraph") for d in (problem_dir, oracle_dir))
    for r in rows:
        pen = r["penalty_str"]
        if not os.path.exists("%s_penalty=%s_loss.tsv" % (obg, pen)):
            assert oracle.solve(obg, pen) == 0
            if os.path.exists("%s_penalty=%s.db" % (obg, pen)):
                os.unlink("%s_penalty=%s.db" % (obg, pen))
        for suffix in ("_segments.bed", "_loss.tsv"):
            assert open("%s_penalty=%s%s" % (bg, pen, suffix), "rb").read() == \
                open("%s_penalty=%s%s" % (obg, pen, suffix), "rb").read(), (pen, suffix)
        t = open("%s_penalty=%s_timing.tsv" % (bg, pen)).read().split("\t")
        assert len(t) == 3 and float(t[0]) == float(pen)
        assert not os.path.exists("%s_penalty=%s.db" % (bg, pen))


def reference_choice(trace, target):
    """the model sequentialSearch_dir returns, from the models its loop visited"""
    hits = [m for m in trace if m["peaks"] == target]
    if hits:
        return hits[-1]
    return max((m for m in trace if m["peaks"] < target), key=lambda m: m["peaks"])


def scenario_width_one(psd, known_answers, tmp_path):
    """width 1 is the sequential search: the rows of PeakSegFPOP_sequential_search, field by
    field, and the reference's eleven penalties for Mono27ac's 19 peaks"""
    st, par, par_chosen = native_search(mono_dir(tmp_path, "par"), 19, 1)
    assert st == 0
    st, seq, seq_chosen = native_search(mono_dir(tmp_path, "seq"), 19, 0, sequential=True)
    assert st == 0
    assert same_rows(par, seq) and par_chosen == seq_chosen
    want = known_answers["mono27ac"]["sequential_search_19"]
    assert [r["peaks"] for r in par] == want["peaks"] and len(par) == 11
    assert [r["penalty"] for r in par] == pytest.approx([float(p) for p in want["penalties"]],
                                                        rel=1e-9)
    assert par[par_chosen]["peaks"] == 19


def scenario_same_model_in_fewer_rounds(psd, oracle, tmp_path, targets, width=8):
    """For each target on Mono27ac: the model of the reference's loop (driven by the oracle), the
    oracle's bytes for every model visited, the rules of a round, and at most half the loop's
    iterations, rounded up."""
    odir = mono_dir(tmp_path, "oracle")
    obg = os.path.join(odir, "coverage.bedGraph")
    report = {}
    for target in targets:
        gdir = mono_dir(tmp_path, "par%d" % target)
        t0 = time.time()
        st, rows, chosen = native_search(gdir, target, width)
        seconds = time.time() - t0
        assert st == 0
        trace = gp2._oracle_search(oracle, odir, target)
        want = reference_choice(trace, target)
        got = rows[chosen]
        assert got["peaks"] == want["peaks"]
        seg_g = read_segments("%s_penalty=%s_segments.bed" % (
            os.path.join(gdir, "coverage.bedGraph"), got["penalty_str"]))
        seg_o = read_segments("%s_penalty=%s_segments.bed" % (obg, want["penalty"]))
        assert seg_g == seg_o  # chromStart, chromEnd, status, and the means as printed
        check_files_against_oracle(oracle, gdir, odir, rows)
        rounds = check_rules(psd, rows, chosen, target, width)
        iterations = len(trace) - 1  # iteration 1 asks for two models
        print("Mono27ac target %d: %d peaks; reference loop %d iterations, width %d: %d rounds, "
              "%d models, %.1f s" % (target, got["peaks"], iterations, width, rounds, len(rows),
                                     seconds))
        assert rounds <= (iterations + 1) // 2
        report[target] = (gdir, rows, chosen)
    return report


def scenario_cache_and_errors(psd, tmp_path, gdir, rows, chosen, target, width=8):
    """a second identical call: the same rows, all cached; bad arguments; a target above the
    maximum"""
    st, again, again_chosen = native_search(gdir, target, width)
    assert st == 0 and same_rows(again, rows) and again_chosen == chosen
    assert all(r["cached"] for r in again)
    from peaksegdisk_amd import _native
    for bad in (dict(target=-1, width=width), dict(target=target, width=-1),
                dict(target=target, width=257), dict(target=target, width=width, capacity=1)):
        st, got, got_chosen = native_search(gdir, **bad)
        assert st == _native.ERROR_SEARCH_ARGUMENTS and got == [] and got_chosen == -1
    st, got, got_chosen = native_search(gdir, target, width, capacity=3)  # round 2 does not fit
    assert st == _native.ERROR_SEARCH_ARGUMENTS
    with pytest.raises(ValueError, match="peaks.int=300000 but max=259999 peaks for N=520000"):
        psd.parallelSearch_dir(gdir, 300000)
    with pytest.raises(ValueError):
        psd.parallelSearch_dir(gdir, target, width=300)
    fit = psd.parallelSearch_dir(gdir, target, width=width)
    assert int(fit.loss["peaks"].iloc[0]) == rows[chosen]["peaks"]
    assert list(fit.others["peaks"]) == [r["peaks"] for r in rows]
    assert list(fit.others["iteration"]) == [r["iteration"] for r in rows]


def _small_dirs(root, specs):
    from peaksegdisk_amd import synthetic
    out = []
    for name, n_bins, seed in specs:
        d = root / name
        d.mkdir(parents=True)
        cs, ce, cnt = synthetic.poisson_coverage(n_bins, seed=seed)
        synthetic.write_bedgraph(str(d / "coverage.bedGraph"), cs, ce, cnt)
        out.append(str(d))
    return out


def _same_files(dir_a, dir_b, rows):
    for r in rows:
        for suffix in ("_segments.bed", "_loss.tsv"):
            a, b = ("%s_penalty=%s%s" % (os.path.join(d, "coverage.bedGraph"), r["penalty_str"],
                                         suffix) for d in (dir_a, dir_b))
            assert open(a, "rb").read() == open(b, "rb").read()
        t = "%s_penalty=%s_timing.tsv" % (os.path.join(dir_a, "coverage.bedGraph"),
                                          r["penalty_str"])
        assert len(open(t).read().split("\t")) == 3


def scenario_batch_and_fanout(psd, tmp_path, monkeypatch, specs, targets, devices, n_shards,
                              width=4):
    """the batch form: per directory the rows and files of the single form; the same under
    PEAKSEG_HIP_DEVICES, with one shard per listed device"""
    monkeypatch.delenv("PEAKSEG_HIP_DEVICES", raising=False)
    alone = _small_dirs(tmp_path / "alone", specs)
    together = _small_dirs(tmp_path / "together", specs)
    fanned = _small_dirs(tmp_path / "fanned", specs)
    singles = []
    for d, target in zip(alone, targets):
        st, rows, chosen = native_search(d, target, width)
        assert st == 0
        check_rules(psd, rows, chosen, target, width)
        singles.append((rows, chosen))
    assert len({len(rows) for rows, _ in singles}) > 1  # searches of different lengths
    st, batch = native_search_batch(together, targets, width)
    assert st == 0
    assert psd.last_fanout()["device"] == []
    monkeypatch.setenv("PEAKSEG_HIP_DEVICES", devices)
    st, fan = native_search_batch(fanned, targets, width)
    report = psd.last_fanout()
    monkeypatch.delenv("PEAKSEG_HIP_DEVICES")
    assert st == 0
    assert len(report["device"]) == n_shards
    assert sorted(set(report["shard_of"])) == list(range(min(n_shards, len(specs))))
    for (rows, chosen), d_a, d_t, d_f, got_t, got_f in zip(singles, alone, together, fanned,
                                                          batch, fan):
        for got, d in ((got_t, d_t), (got_f, d_f)):
            assert got[2] == 0 and got[1] == chosen and same_rows(got[0], rows)
            _same_files(d, d_a, rows)
    # the Python form, served from the cache; a directory listed twice is refused
    fits = psd.parallelSearch_dir_batch(together, targets, width=width)
    assert [int(f.loss["peaks"].iloc[0]) for f in fits] == [r[c]["peaks"] for r, c in singles]
    with pytest.raises(psd.PeakSegError) as e:
        psd.parallelSearch_dir_batch([together[0], together[0]], 2, width=width)
    assert e.value.status == 15
    # a directory without data fails alone; the other search still ends
    bad = tmp_path / "together" / "missing"
    bad.mkdir()
    st, got = native_search_batch([together[0], str(bad)], [targets[0], 2], width)
    assert st == 3 and got[1][2] == 3 and got[0][2] == 0 and same_rows(got[0][0], singles[0][0])


# ---- on the MI355X ------------------------------------------------------------------------

@GPU
def test_parallel_search_width_one_is_the_sequential_search(psd, known_answers, tmp_path):
    scenario_width_one(psd, known_answers, tmp_path)


@GPU
def test_parallel_search_same_model_in_fewer_rounds(psd, oracle_det, tmp_path):
    report = scenario_same_model_in_fewer_rounds(psd, oracle_det, tmp_path,
                                                 [19, 100, 1000, 2500, 15])
    gdir, rows, chosen = report[19]
    scenario_cache_and_errors(psd, tmp_path, gdir, rows, chosen, 19)


@GPU
def test_parallel_search_for_most_peaks_minus_one(psd, oracle_det, tmp_path):
    """Mono27ac, 3198 peaks (most.peaks - 1): near penalty 0 the cost is numerically unstable and
    peaks are not monotone in the penalty; the reference's own loop gives up at 2894 peaks.  The
    search must end, return at most 3198 peaks, and every model it visited must be the oracle's
    (no claim that it is the sequential search's model)."""
    gdir = mono_dir(tmp_path, "par")
    st, rows, chosen = native_search(gdir, 3198, 8)
    assert st == 0
    assert rows[chosen]["peaks"] <= 3198
    strings = [r["penalty_str"] for r in rows]
    assert len(set(strings)) == len(strings)
    assert all(sum(1 for r in rows if r["iteration"] == it) <= 8
               for it in range(2, rows[-1]["iteration"] + 1))
    check_files_against_oracle(oracle_det, gdir, mono_dir(tmp_path, "oracle"), rows)
    print("Mono27ac target 3198: %d peaks chosen, %d rounds, %d models"
          % (rows[chosen]["peaks"], rows[-1]["iteration"], len(rows)))


@GPU
def test_parallel_search_on_a_long_contig(psd, tmp_path, n_bins=500000, peaks_int=354):
    """The 5e5-bin contig of test_sequential_search_on_a_long_contig at the default width: the
    target's model, byte-identical to the oracle's at the chosen penalty, the segmentation of the
    model the reference's loop ends on (that loop runs on the oracle, on host cores, while the GPU
    searches), in at most half the loop's iterations, rounded up."""
    import test_gpu_round3 as gp3
    from peaksegdisk_amd import synthetic
    cs, ce, cnt = synthetic.poisson_coverage(n_bins, seed=1)
    gdir = tmp_path / "gpu" / "chrSynth-0-1"
    odir = tmp_path / "oracle" / "chrSynth-0-1"
    for d in (gdir, odir):
        d.mkdir(parents=True)
    bg = str(odir / "coverage.bedGraph")
    gp2.write_bedgraph_chunked(bg, cs, ce, cnt)
    os.link(bg, str(gdir / "coverage.bedGraph"))
    loop = {}

    def reference_loop():
        try:
            loop["trace"] = gp3._oracle_search(str(odir), peaks_int)
        except BaseException as e:  # reported below
            loop["error"] = e
    worker = threading.Thread(target=reference_loop)
    worker.start()
    t0 = time.time()
    try:
        st, rows, chosen = native_search(str(gdir), peaks_int, 0)
    finally:
        seconds = time.time() - t0
        worker.join()
    assert "error" not in loop, loop.get("error")
    assert st == 0
    rounds = check_rules(psd, rows, chosen, peaks_int, 8)
    trace = loop["trace"]
    iterations = len(trace) - 1
    print("search of %d bins for %d peaks: reference loop %d iterations; default width: %d rounds, "
          "%d models, %.1f s" % (n_bins, peaks_int, iterations, rounds, len(rows), seconds))
    got = rows[chosen]
    assert got["peaks"] == peaks_int
    want = reference_choice(trace, peaks_int)
    assert want["peaks"] == peaks_int
    gbg = str(gdir / "coverage.bedGraph")
    if not os.path.exists("%s_penalty=%s_loss.tsv" % (bg, got["penalty_str"])):
        gp3._oracle_model(bg, got["penalty_str"])
    for suffix in ("_segments.bed", "_loss.tsv"):
        assert open("%s_penalty=%s%s" % (gbg, got["penalty_str"], suffix), "rb").read() == \
            open("%s_penalty=%s%s" % (bg, got["penalty_str"], suffix), "rb").read()
    seg_g = read_segments("%s_penalty=%s_segments.bed" % (gbg, got["penalty_str"]))
    seg_o = read_segments("%s_penalty=%s_segments.bed" % (bg, want["penalty"]))
    assert [s[:4] for s in seg_g] == [s[:4] for s in seg_o]
    assert rounds <= (iterations + 1) // 2


@GPU
def test_parallel_search_batch_and_fanout(psd, tmp_path, monkeypatch):
    specs = [("s1", 20000, 81), ("s2", 15000, 82), ("s3", 12000, 83)]
    scenario_batch_and_fanout(psd, tmp_path, monkeypatch, specs, [7, 25, 2], "0,0", 2)


@GPU
def test_parallel_search_single_form_fans_out_its_rounds(psd, tmp_path, monkeypatch):
    """PEAKSEG_HIP_DEVICES with the single form: each round's models dealt over the listed
    devices; rows equal to the call without the knob"""
    monkeypatch.delenv("PEAKSEG_HIP_DEVICES", raising=False)
    pdir = mono_dir(tmp_path, "plain")
    st, rows, chosen = native_search(pdir, 19, 8)
    assert st == 0
    fdir = mono_dir(tmp_path, "fanned")
    fit = psd.parallelSearch_dir(fdir, 19, width=8, devices="0,0")
    report = psd.last_fanout()
    assert len(report["device"]) == 2 and sum(report["programs"]) >= 1
    assert "PEAKSEG_HIP_DEVICES" not in os.environ
    st, again, again_chosen = native_search(fdir, 19, 8)
    assert st == 0 and same_rows(again, rows) and again_chosen == chosen
    assert all(r["cached"] for r in again)
    assert int(fit.loss["peaks"].iloc[0]) == 19
    _same_files(fdir, pdir, rows)
