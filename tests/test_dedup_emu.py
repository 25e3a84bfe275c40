"""CPU rehearsal of duplicate removal: the scenario functions of tests/test_gpu_dedup.py on the SIMT
emulator build of the library (tests/emu), which compiles the kernels of reads_dedup.h from the same
source.  "Device" memory is host memory there, so the reads are numpy arrays; the cuda-tensor form
runs on the MI355X only.  The emulator being slow, the sizes scenario runs in parts -- the sizes
below a wave at two keeps, the largest one, whose table scan takes a second trip, at one -- and the
digits scenario takes the first and last bit of every digit; the other scenarios run whole.  As in
tests/test_strand_xcorr_emu.py the emulator library is swapped into peaksegdisk_amd._native for this
module's tests only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import test_gpu_dedup as gdd
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


def test_emu_dedup_sizes_within_a_wave(psd):
    gdd.scenario_sizes(gdd.as_numpy, n_values=gdd.all_sizes()[:6], keeps=(1, 3))


def test_emu_dedup_sizes_around_a_slice(psd):
    gdd.scenario_sizes(gdd.as_numpy, n_values=gdd.all_sizes()[6:9])


def test_emu_dedup_sizes_around_a_sort_workgroup(psd):
    gdd.scenario_sizes(gdd.as_numpy, n_values=gdd.all_sizes()[9:-1])


def test_emu_dedup_table_scan_second_trip(psd):
    gdd.scenario_sizes(gdd.as_numpy, n_values=gdd.all_sizes()[-1:], keeps=(2,))


def test_emu_dedup_order_and_stability(psd):
    gdd.scenario_order(gdd.as_numpy)


def test_emu_dedup_runs_and_carries(psd):
    gdd.scenario_runs(gdd.as_numpy)


def test_emu_dedup_every_digit(psd):
    gdd.scenario_digits(gdd.as_numpy, bits=gdd.DIGIT_EDGES)


def test_emu_dedup_contigs(psd):
    gdd.scenario_contigs(gdd.as_numpy)


def test_emu_dedup_refusals(psd):
    gdd.scenario_refusals(gdd.as_numpy)


def test_emu_dedup_device_addresses(psd):
    """reads_on_device = 1 (the emulator's device memory is host memory)"""
    def host_array(v):
        room = np.zeros(v.nbytes + 16, np.uint8)
        lead = -room.ctypes.data % 16
        room[lead:lead + v.nbytes] = np.ascontiguousarray(v).view(np.uint8)
        return room, room.ctypes.data + lead
    gdd.scenario_offsets(host_array)


def test_emu_dedup_compaction(psd):
    gdd.scenario_compaction(psd, gdd.as_numpy, n_values=gdd.all_sizes()[:-1])


def test_emu_dedup_composition(psd):
    gdd.scenario_composition(psd, gdd.as_numpy)


def test_emu_dedup_fixture_and_determinism(psd):
    gdd.scenario_fixture(psd, gdd.as_numpy)


def test_emu_dedup_synthetic_share(psd):
    gdd.scenario_synthetic(psd, gdd.as_numpy)
