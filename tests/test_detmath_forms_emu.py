"""CPU rehearsal of tests/test_gpu_detmath.py: its scenario functions on the SIMT emulator build of
the library (tests/emu), which compiles peaksegdisk_amd/csrc/math_forms_probe.h and the C entry from
the same source.

The emulator compiles the HOST branch of include/peakseg_detmath.h: one set of constants (set 1 is
the plain set there), a plain test instead of the wave-uniform branch, the division operator for
psd_div.  So these tests prove the harness -- the entry's copies, its bounds and refusals, the
layouts, the comparison -- and nothing about the device's arithmetic: that is what the tests marked
gpu are for."""
import ctypes
import os
import subprocess

import pytest

import test_gpu_detmath as gd
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


@pytest.mark.parametrize("form", range(8), ids=gd.FORMS)
def test_emu_forms(psd, oracle_det, form):
    gd.scenario_forms(psd, oracle_det, forms=[form])


def test_emu_division(psd, oracle_det):
    assert gd.scenario_div(psd, oracle_det, n_subnormal=20000, repaired=False) == 0


def test_emu_forms_probe_refusals(psd, oracle_det):
    gd.scenario_refusals(psd, oracle_det)
