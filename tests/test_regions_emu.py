"""CPU rehearsal of ProblemSet.region_stats: the scenario functions of tests/test_gpu_regions.py on
the SIMT emulator build of the library (tests/emu), which compiles the kernels of
peaksegdisk_amd/csrc/region_stats.h from the same source.  "Device" memory is host memory there: the
regions are numpy arrays, and the refusals of device arrays are rehearsed by handing the C entry
the same arrays as device addresses; the cuda-tensor and torch_device forms run on the MI355X only.
As in tests/test_label_errors_emu.py the emulator library is swapped into peaksegdisk_amd._native
for this module's tests only."""
import ctypes
import os
import subprocess

import pytest

import test_gpu_regions as gr
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


@pytest.mark.parametrize("scenario", gr.SCENARIOS, ids=lambda f: f.__name__[len("scenario_"):])
def test_emu_regions(psd, scenario):
    scenario(psd, as_numpy)


def test_emu_regions_refusals(psd):
    gr.scenario_refusals(psd, as_numpy, lambda a: (a.ctypes.data, a))
