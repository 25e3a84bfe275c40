"""CPU rehearsal of the parallel penalty search: the scenario functions of
tests/test_gpu_parallel_search.py on the SIMT emulator build of the library (tests/emu), checked
against the oracle, plus the paths that need no solver at all.  As in tests/test_emu_parity.py the
emulator library is swapped into peaksegdisk_amd._native for this module's tests only.

One emulator search per target serves the model, rule and round-count checks; the reference's loop
is driven by the oracle.

Narrowing on ERROR_DEVICE_MEMORY: test_emu_parallel_search_narrows_on_a_memory_status caps
PEAKSEG_HIP_MAX_BYTES (checkpointed store forbidden) so that a round of eight Mono27ac models does
not fit; the search must come back with the width-1 search's model all the same.  Status 14 is
reachable this way where the library refuses to create the set; see that test for why its search
runs in a process of its own."""
import ctypes
import os
import shutil
import subprocess

import pytest

import test_gpu_parallel_search as ps
from conftest import GOLDEN, ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu")


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


def test_emu_parallel_search_width_one_is_the_sequential_search(psd, known_answers, tmp_path):
    ps.scenario_width_one(psd, known_answers, tmp_path)


def test_emu_parallel_search_same_model_in_fewer_rounds(psd, oracle_det, tmp_path):
    """Mono27ac, width 8, targets 19, 100, 1000, 2500 and 15 (no 15-peak model: 14 peaks); then
    the cache and the argument checks on the first of these directories"""
    report = ps.scenario_same_model_in_fewer_rounds(psd, oracle_det, tmp_path,
                                                    [19, 100, 1000, 2500, 15])
    gdir, rows, chosen = report[19]
    ps.scenario_cache_and_errors(psd, tmp_path, gdir, rows, chosen, 19)


def test_emu_parallel_search_batch_and_fanout(psd, tmp_path, monkeypatch):
    specs = [("s1", 400, 81), ("s2", 900, 82), ("s3", 1400, 83)]
    ps.scenario_batch_and_fanout(psd, tmp_path, monkeypatch, specs, [7, 2, 11], "0,0", 2)


_NARROWING_WORKER = r"""
import ctypes, json, os, sys
import numpy as np
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
from peaksegdisk_amd import _native
_native.lib = _native.declare(ctypes.CDLL(sys.argv[2]))
from peaksegdisk_amd import ProblemSet
import test_gpu_parallel_search as ps
cols = np.loadtxt(os.path.join(sys.argv[3], "coverage.bedGraph"), usecols=(1, 2, 3), dtype=np.int64)
count, weight = cols[:, 2].astype(np.int32), (cols[:, 1] - cols[:, 0]).astype(np.int32)
two = ProblemSet([(count, weight)], [(0, 1000.0), (0, 2000.0)])
os.environ["PEAKSEG_HIP_MAX_BYTES"] = "%d" % two.hbm_bytes
two.close()
st, rows, chosen = ps.native_search(sys.argv[3], 19, 8)
print(json.dumps({"status": st, "rows": rows, "chosen": chosen}))
"""


def test_emu_parallel_search_narrows_on_a_memory_status(psd, oracle_det, tmp_path):
    """A budget that holds two Mono27ac models but not eight (what a set of two holds when it is
    created; checkpointed store forbidden): the width-8 search halves its width when a round's
    launch reports ERROR_DEVICE_MEMORY, repeats the models still missing, and ends with the model
    of the width-1 search (the reference's loop, driven here by the oracle).  The search runs in a
    process of its own: what a set may hold before the library refuses it depends on what the
    process has solved before, and a set that is admitted under such a cap and then cannot grow is
    the arena's business, not this test's."""
    import json
    import sys
    gdir = ps.mono_dir(tmp_path, "w8")
    odir = ps.mono_dir(tmp_path, "w1")
    env = dict(os.environ, PEAKSEG_HIP_NO_CHECKPOINT="1")
    env.pop("PEAKSEG_HIP_MAX_BYTES", None)
    emu = os.environ.get("PSD_EMU_LIB_OVERRIDE",
                         os.path.join(EMU_DIR, "_build", "libpeaksegdisk_emu.so"))
    p = subprocess.run([sys.executable, "-c", _NARROWING_WORKER, ROOT, emu, gdir], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    rows, chosen = got["rows"], got["chosen"]
    assert got["status"] == 0
    want = ps.reference_choice(ps.gp2._oracle_search(oracle_det, odir, 19), 19)
    assert rows[chosen]["peaks"] == want["peaks"] == 19
    assert ps.read_segments("%s_penalty=%s_segments.bed" % (
        os.path.join(gdir, "coverage.bedGraph"), rows[chosen]["penalty_str"])) == \
        ps.read_segments("%s_penalty=%s_segments.bed" % (
            os.path.join(odir, "coverage.bedGraph"), want["penalty"]))
    # the budget did bite: after round 1 no round kept eight models
    widths = [sum(1 for r in rows if r["iteration"] == it)
              for it in range(2, rows[-1]["iteration"] + 1)]
    assert widths and max(widths) < 8, widths
    ps.check_rules(psd, rows, chosen, 19, 8)


def test_parallel_search_without_gpu(tmp_path):
    """The real library on a machine without a device: the first round's penalty 0 is a dynamic
    program, so the call fails with status 12 before anything is returned (no CPU fallback)."""
    import __graft_entry__ as entry
    entry.build_hip()
    from peaksegdisk_amd import _native, api
    real = _native.declare(ctypes.CDLL(_native.LIB_PATH))
    if real.peakseg_hip_device_count() > 0:
        pytest.skip("a GPU is visible")
    d = tmp_path / "prob"
    d.mkdir()
    shutil.copy(os.path.join(GOLDEN, "Mono27ac.bedGraph"), str(d / "coverage.bedGraph"))
    rows = (_native.PsdSearchRow * 32)()
    n = ctypes.c_int(-1)
    chosen = ctypes.c_int(0)
    st = real.PeakSegFPOP_parallel_search(os.fsencode(str(d)), 19, 8, 0, 32, rows,
                                          ctypes.byref(n), ctypes.byref(chosen))
    assert st == _native.ERROR_NO_HIP_DEVICE and n.value == 0 and chosen.value == -1
    for peaks, width, cap in ((-1, 8, 32), (19, -1, 32), (19, 257, 32), (19, 8, 1)):
        st = real.PeakSegFPOP_parallel_search(os.fsencode(str(d)), peaks, width, 0, cap, rows,
                                              ctypes.byref(n), ctypes.byref(chosen))
        assert st == _native.ERROR_SEARCH_ARGUMENTS and n.value == 0 and chosen.value == -1
    assert _native.lib is not None
    if _native.lib.peakseg_hip_device_count() == 0:  # (not while the emulator is swapped in)
        with pytest.raises(api.PeakSegError) as e:
            api.parallelSearch_dir(str(d), 19)
        assert e.value.status == 12
        with pytest.raises(api.PeakSegError) as e:
            api.parallelSearch_dir_batch([str(d)], 19, width=4)
        assert e.value.status == 12
    with pytest.raises(ValueError):
        api.parallelSearch_dir(str(d), -1)
    with pytest.raises(ValueError):
        api.parallelSearch_dir_batch([str(d)], [1, 2])
