"""CPU rehearsal of the histories of service calls: the scenario functions of
tests/test_gpu_resident_tables.py on the SIMT emulator build of the library (tests/emu), which
compiles the host code of every pack_* service and its kernels from the same source.  Scenarios 1 to
5 for every service with host arrays; the cuda-tensor forms run on the MI355X only.  As in
tests/test_heldout_emu.py the emulator library is swapped into peaksegdisk_amd._native for this
module's tests only."""
import ctypes
import os
import subprocess

import pytest

import test_gpu_resident_tables as rt
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


@pytest.mark.parametrize("name", rt.HISTORY_SERVICES)
def test_emu_history(psd, name):
    rt.scenario_history(psd, name)


@pytest.mark.parametrize("name", rt.CAPPED_SERVICES)
def test_emu_capped_twins(psd, name):
    rt.scenario_capped_twins(psd, name)


def test_emu_services_taking_turns(psd):
    rt.scenario_turns(psd)


def test_emu_clusters_as_windows(psd):
    rt.scenario_clusters_as_windows(psd)


def test_emu_solve_in_between(psd):
    rt.scenario_resolve(psd)


@pytest.mark.parametrize("name", rt.REFUSING)
def test_emu_refusal_in_between(psd, name):
    rt.scenario_refusal(psd, name)
