"""CPU rehearsal of the target-interval search: the scenario functions of
tests/test_gpu_target_interval.py on the SIMT emulator build of the library (tests/emu).  Every
scenario runs in a process of its own, with the emulator library swapped into
peaksegdisk_amd._native there: a search creates and solves set after set, and DESIGN.md section 8
("Memory") tells what a process that had solved other sets before once did on the emulator.

The search of Mono27ac at width 1 (17 rounds of one model each, ten seconds a model here) runs on
the MI355X only; the emulator rehearses width 1 on the small contig."""
import os
import subprocess
import sys

import pytest

import test_gpu_target_interval as gt
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu")

_CHILD = r"""
import ctypes, os, sys
sys.path[:0] = [%(root)r, %(tests)r]
import peaksegdisk_amd
from peaksegdisk_amd import _native
_native.lib = _native.declare(ctypes.CDLL(os.environ.get(
    "PSD_EMU_LIB_OVERRIDE", os.path.join(%(emu)r, "_build", "libpeaksegdisk_emu.so"))))
import test_gpu_target_interval as gt
getattr(gt, %(name)r)(peaksegdisk_amd)
print("target-child ok")
"""

SCENARIOS = [f for f in gt.SCENARIOS if f is not gt.scenario_mono27ac_width1]


@pytest.fixture(scope="module")
def emu_built():
    import __graft_entry__ as entry
    entry.build_hip()  # the package refuses to import without its HIP library
    subprocess.run(["make", "-s", "-C", EMU_DIR], check=True)


@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__[len("scenario_"):])
def test_emu_target_interval(emu_built, scenario):
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "emu": EMU_DIR,
                     "name": scenario.__name__}
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    print(p.stdout[-6000:])
    assert p.returncode == 0 and "target-child ok" in p.stdout, p.stdout[-3000:] + p.stderr[-6000:]
