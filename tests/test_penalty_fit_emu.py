"""CPU rehearsal of the penalty-model fits: the scenario functions of tests/test_gpu_penalty_fit.py
on the SIMT emulator build of the library (tests/emu), which compiles the kernel of
peaksegdisk_amd/csrc/penalty_fit.h from the same source.  The end-to-end scenario runs on the MI355X
only: the emulator cannot afford its penalty searches.  As in tests/test_coverage_features_emu.py
the emulator library is swapped into peaksegdisk_amd._native for this module's tests only."""
import ctypes
import os
import subprocess

import pytest

import test_gpu_penalty_fit as pf
from conftest import ROOT

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


@pytest.mark.parametrize("scenario", pf.SCENARIOS, ids=lambda f: f.__name__[len("scenario_"):])
def test_emu_penalty_fit(psd, scenario):
    scenario(psd)
