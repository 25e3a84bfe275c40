"""PEAKSEG_HIP_DEVICES without a GPU: a device id that is not visible on the real HIP library,
and the fan-out itself on the SIMT emulator (tests/emu, one device: "0,0,0" is three problem
sets, one after the other, on three host threads).  The scenarios are those of
tests/test_gpu_fanout.py at emulator sizes."""
import ctypes
import os
import subprocess

import pytest

import test_gpu_fanout as fo
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu")


@pytest.fixture(scope="module")
def real():
    import __graft_entry__ as entry
    entry.build_hip()
    from peaksegdisk_amd import _native
    return _native


@pytest.fixture(scope="module")
def emu():
    import __graft_entry__ as entry
    entry.build_hip()  # the package refuses to import without its HIP library
    subprocess.run(["make", "-s", "-C", EMU_DIR], check=True)
    import peaksegdisk_amd
    from peaksegdisk_amd import _native
    lib = _native.declare(ctypes.CDLL(os.path.join(EMU_DIR, "_build", "libpeaksegdisk_emu.so")))
    real_lib = _native.lib
    _native.lib = lib
    try:
        yield peaksegdisk_amd
    finally:
        _native.lib = real_lib


def test_bad_device_id_on_the_real_library(real, tmp_path):
    """PEAKSEG_HIP_DEVICES=3 (or the first id past the visible ones): status 12 for the dynamic
    program, the Inf model still written, the message names device 3 and the visible count."""
    bad = max(3, real.lib.peakseg_hip_device_count())
    fo.scenario_bad_device(tmp_path, bad)


def test_malformed_device_list(real, tmp_path):
    bg = str(tmp_path / "coverage.bedGraph")
    with open(bg, "w") as f:
        f.write("chr1\t0\t10\t2\nchr1\t10\t20\t10\nchr1\t20\t30\t14\n")
    for bad in ("0,", "x", "0;1", ",0", "-1"):
        os.environ["PEAKSEG_HIP_DEVICES"] = bad
        try:
            st = fo.disk_batch([(bg, "10.5"), (bg, "Inf")])
            msg = real.last_error()
        finally:
            del os.environ["PEAKSEG_HIP_DEVICES"]
        assert st == [real.ERROR_NO_HIP_DEVICE, 0], bad
        assert "PEAKSEG_HIP_DEVICES=%s is not" % bad in msg, msg


def test_file_batch_on_the_emulator(emu, oracle_det, tmp_path):
    report = fo.scenario_file_batch(oracle_det, tmp_path, "0,0,0", 3,
                                    ["1952.6", "157.994737329317", "40000"], 2, 1500,
                                    ["3", "30", "300", "3000"])
    assert report["device"] == [0, 0, 0] and min(report["programs"]) >= 1


def test_dir_batch_twice_on_the_emulator(emu, tmp_path):
    specs = [("s1", 1500, 71), ("s2", 1200, 72), ("s3", 900, 73)]
    fo.scenario_dir_batch(emu, tmp_path, [0, 0], 2, specs, ["5", "500"])


def test_search_batch_on_the_emulator(emu, tmp_path):
    specs = [("six", "six", 0), ("s1", 1500, 81), ("s2", 1000, 82)]
    fo.scenario_search(emu, tmp_path, "0,0", 2, specs, [2, 3, 1])


def test_all_is_one_shard_on_the_emulator(emu, tmp_path):
    from peaksegdisk_amd import _native, synthetic
    cs, ce, cnt = synthetic.poisson_coverage(600, seed=5)
    bg = str(tmp_path / "a.bedGraph")
    synthetic.write_bedgraph(bg, cs, ce, cnt)
    os.environ["PEAKSEG_HIP_DEVICES"] = "all"
    try:
        st = fo.disk_batch([(bg, "10"), (bg, "Inf"), (bg, "100")])
    finally:
        del os.environ["PEAKSEG_HIP_DEVICES"]
    assert st == [0, 0, 0]
    report = _native.last_fanout()
    assert report["device"] == [0] and report["programs"] == [2]
    assert report["shard_of"] == [0, -1, 0]
