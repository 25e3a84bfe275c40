"""CPU rehearsal of ProblemSet.heldout_loss: the scenario functions of tests/test_gpu_heldout.py on
the SIMT emulator build of the library (tests/emu), which compiles the kernels of
peaksegdisk_amd/csrc/heldout_loss.h and region_stats.h from the same source.  The cuda-tensor and
torch_device forms run on the MI355X only.  As in tests/test_joint_path_emu.py the emulator library
is swapped into peaksegdisk_amd._native for this module's tests only."""
import ctypes
import os
import subprocess

import pytest

import test_gpu_heldout as gh
from conftest import ROOT
from test_gpu_dense import as_numpy

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


@pytest.mark.parametrize("scenario", gh.SCENARIOS, ids=lambda f: f.__name__[len("scenario_"):])
def test_emu_heldout(psd, scenario):
    scenario(psd, as_numpy)
