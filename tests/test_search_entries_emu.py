"""The four penalty-search entries side by side, on the SIMT emulator build of the library
(tests/emu; swapped into peaksegdisk_amd._native for this module's tests only, as in
tests/test_parallel_search_emu.py).

PeakSegFPOP_sequential_search, _sequential_search_batch, _parallel_search and
_parallel_search_batch drive one state machine; what tells them apart is words, and this module
pins those words and the places where the entries must agree and no other test looks:

  * the text of last_error() per entry (a full row table, a directory listed twice, bad arguments);
  * the verbose lines, which at width 1 are the same for a sequential and a parallel entry;
  * the batch forms at width 1: same rows, same choice, same files;
  * a search that fails at a model: n_rows counts the models recorded before it, so that
    rows[n_rows] names the one that failed (the Python wrappers build their message from it).

Data: the three small Poisson directories of the emulator's batch test (400, 900 and 1400 bins)."""
import ctypes
import os
import subprocess

import pytest

import test_gpu_parallel_search as ps
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu")
SPECS = [("s1", 400, 81), ("s2", 900, 82), ("s3", 1400, 83)]
TARGETS = [7, 2, 11]
KIND = {"sequential": "sequential", "sequential_batch": "sequential",
        "parallel": "parallel", "parallel_batch": "parallel"}
PRINT_FN = ctypes.CFUNCTYPE(None, ctypes.c_char_p)


@pytest.fixture(scope="module")
def psd():
    import __graft_entry__ as entry
    entry.build_hip()  # the package refuses to import without its HIP library
    subprocess.run(["make", "-s", "-C", EMU_DIR], check=True)
    import peaksegdisk_amd
    from peaksegdisk_amd import _native
    emu = _native.declare(ctypes.CDLL(os.environ.get(
        "PSD_EMU_LIB_OVERRIDE", os.path.join(EMU_DIR, "_build", "libpeaksegdisk_emu.so"))))
    real = _native.lib
    _native.lib = emu
    try:
        yield peaksegdisk_amd
    finally:
        _native.lib = real


@pytest.fixture(scope="module")
def singles(psd, tmp_path_factory):
    """[(rows, chosen)] of PeakSegFPOP_sequential_search on each directory alone, and where"""
    dirs = ps._small_dirs(tmp_path_factory.mktemp("alone"), SPECS)
    out = []
    for d, target in zip(dirs, TARGETS):
        st, rows, chosen = ps.native_search(d, target, 1, sequential=True)
        assert st == 0 and chosen >= 0
        out.append((rows, chosen))
    return dirs, out


def sequential_search_batch(problem_dirs, targets, capacity=1024):
    """ps.native_search_batch for PeakSegFPOP_sequential_search_batch"""
    return search("sequential_batch", problem_dirs, targets, capacity=capacity)[:2]


def search(entry, problem_dirs, targets, width=1, capacity=1024, verbose=0, raw=None):
    """One native search through any of the four entries ->
    (status, [(rows as dicts, chosen, status) per directory], the row table itself, [n_rows]).
    raw: dict(dirs=, peaks=, rows=) replaces those arguments as given (None: a null pointer)."""
    from peaksegdisk_amd import _native
    lib = ps._lib()
    n = len(problem_dirs)
    rows = (_native.PsdSearchRow * (capacity * n))()
    n_rows = (ctypes.c_int * n)(*([-1] * n))
    chosen = (ctypes.c_int * n)()
    status = (ctypes.c_int * n)()
    a = dict(dirs=(ctypes.c_char_p * n)(*[os.fsencode(d) for d in problem_dirs]),
             peaks=(ctypes.c_int * n)(*targets), rows=rows)
    a.update(raw or {})
    if entry == "sequential":
        st = lib.PeakSegFPOP_sequential_search(a["dirs"][0], targets[0], verbose, capacity,
                                               a["rows"], n_rows, chosen)
    elif entry == "parallel":
        st = lib.PeakSegFPOP_parallel_search(a["dirs"][0], targets[0], width, verbose, capacity,
                                             a["rows"], n_rows, chosen)
    elif entry == "sequential_batch":
        st = lib.PeakSegFPOP_sequential_search_batch(n, a["dirs"], a["peaks"], verbose, capacity,
                                                     a["rows"], n_rows, chosen, status)
    else:
        st = lib.PeakSegFPOP_parallel_search_batch(n, a["dirs"], a["peaks"], width, verbose,
                                                   capacity, a["rows"], n_rows, chosen, status)
    if not entry.endswith("_batch"):
        status[0] = st
    per_dir = [([ps._row_dict(rows[d * capacity + k]) for k in range(max(n_rows[d], 0))],
                chosen[d], status[d]) for d in range(n)]
    return st, per_dir, rows, list(n_rows)


def with_print(fn):
    """(fn(), the text the library printed meanwhile, as lines)"""
    got = []
    cb = PRINT_FN(lambda text: got.append(text.decode()))
    ps._lib().peakseg_hip_set_print(ctypes.cast(cb, ctypes.c_void_p))
    try:
        result = fn()
    finally:
        ps._lib().peakseg_hip_set_print(None)
    return result, "".join(got).splitlines(keepends=True)


@pytest.mark.parametrize("entry", sorted(KIND))
def test_error_text_names_the_entry(psd, tmp_path, entry):
    from peaksegdisk_amd import _native
    kind = KIND[entry]
    dirs = ps._small_dirs(tmp_path, SPECS[:1])
    # a row table that round 3 does not fit in
    st, per_dir, _, _ = search(entry, dirs, TARGETS[:1], width=1, capacity=3)
    assert st == _native.ERROR_SEARCH_ARGUMENTS and per_dir[0][2] == st
    assert _native.last_error() == "%s search: more than 3 models" % kind
    # bad arguments: a negative target or no room for round 1 (single), a null table (batch)
    for bad in (dict(targets=[-1]), dict(capacity=1)):
        if entry.endswith("_batch") and "targets" in bad:
            bad = dict(raw=dict(rows=None))
        st = search(entry, dirs, **{"targets": TARGETS[:1], **bad})[0]
        assert st == _native.ERROR_SEARCH_ARGUMENTS
        assert _native.last_error() == "%s search: bad arguments" % kind
    if entry.endswith("_batch"):
        st, per_dir, _, n_rows = search(entry, [dirs[0], dirs[0]], [2, 2])
        assert st == _native.ERROR_SEARCH_ARGUMENTS
        assert [p[2] for p in per_dir] == [0, st] and n_rows[1] == 0
        assert _native.last_error() == \
            "%s search: problem directory %s is listed twice" % (kind, dirs[0])


def test_verbose_lines_at_width_one(psd, tmp_path):
    seq = ps._small_dirs(tmp_path / "seq", SPECS[:2])
    par = ps._small_dirs(tmp_path / "par", SPECS[:2])
    (st_s, got_s, _, _), lines_s = with_print(
        lambda: search("sequential", seq[:1], TARGETS[:1], verbose=1))
    (st_p, got_p, _, _), lines_p = with_print(
        lambda: search("parallel", par[:1], TARGETS[:1], width=1, verbose=1))
    assert st_s == st_p == 0 and ps.same_rows(got_s[0][0], got_p[0][0])
    assert lines_s == lines_p and lines_s[0] == "Next = 0, Inf \n"
    assert len(lines_s) == got_s[0][0][-1]["iteration"]
    assert all(line.startswith("Next = ") and line.endswith(" \n") for line in lines_s)
    # the batch forms name the directory in front of every line (the first directory's files are
    # there already: cached models print the same)
    (st_s, _, _, _), lines_s = with_print(
        lambda: search("sequential_batch", seq, TARGETS[:2], verbose=1))
    (st_p, _, _, _), lines_p = with_print(
        lambda: search("parallel_batch", par, TARGETS[:2], width=1, verbose=1))
    assert st_s == st_p == 0
    assert lines_s[:2] == ["%s: Next = 0, Inf \n" % d for d in seq]
    assert [line.replace(str(tmp_path / "par"), str(tmp_path / "seq")) for line in lines_p] == \
        lines_s


def test_batch_forms_agree_at_width_one(psd, singles, tmp_path):
    alone, want = singles
    seq = ps._small_dirs(tmp_path / "seq", SPECS)
    par = ps._small_dirs(tmp_path / "par", SPECS)
    st_s, got_s = sequential_search_batch(seq, TARGETS)
    st_p, got_p = ps.native_search_batch(par, TARGETS, 1)
    assert st_s == st_p == 0
    for (rows, chosen), d_a, d_s, d_p, g_s, g_p in zip(want, alone, seq, par, got_s, got_p):
        for got, d in ((g_s, d_s), (g_p, d_p)):
            assert got[2] == 0 and got[1] == chosen and ps.same_rows(got[0], rows)
            ps._same_files(d, d_a, rows)


@pytest.mark.parametrize("entry,width", [("sequential", 1), ("sequential_batch", 1),
                                         ("parallel", 4), ("parallel_batch", 4)])
def test_the_failing_model_is_rows_n_rows(psd, singles, tmp_path, entry, width):
    """Penalty 0 solves, penalty Inf cannot write its loss file: the search fails with that
    model's status, has recorded one row, and the row after it names the failure."""
    _, want = singles
    dirs = ps._small_dirs(tmp_path, SPECS[:2])
    os.mkdir(os.path.join(dirs[0], "coverage.bedGraph_penalty=Inf_loss.tsv"))
    if not entry.endswith("_batch"):
        dirs = dirs[:1]
    st, per_dir, rows, n_rows = search(entry, dirs, TARGETS[:len(dirs)], width=width)
    print(entry, "status", st, "n_rows", n_rows)
    assert st == per_dir[0][2] == 8  # ERROR_WRITING_LOSS_OUTPUT
    assert per_dir[0][1] == -1
    assert n_rows[0] == 1
    assert ps.same_rows(per_dir[0][0], want[0][0][:1]) and rows[0].peaks > 0
    assert rows[1].penalty_str == b"Inf"
    if entry.endswith("_batch"):  # the healthy directory's search goes on to its end
        if width == 1:
            assert per_dir[1][2] == 0 and per_dir[1][1] == want[1][1]
            assert ps.same_rows(per_dir[1][0], want[1][0])
        else:
            alone = ps._small_dirs(tmp_path / "alone", SPECS[1:2])[0]
            st1, rows1, chosen1 = ps.native_search(alone, TARGETS[1], width)
            assert st1 == 0 and per_dir[1][2] == 0 and per_dir[1][1] == chosen1
            assert ps.same_rows(per_dir[1][0], rows1)
