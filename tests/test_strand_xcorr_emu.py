"""CPU rehearsal of stranded reads: the scenario functions of tests/test_gpu_strand_xcorr.py on the
SIMT emulator build of the library (tests/emu), which compiles the kernels of strand_xcorr.h from the
same source.  "Device" memory is host memory there, so the reads are numpy arrays; the cuda-tensor
form runs on the MI355X only.  As in tests/test_reads_emu.py the emulator library is swapped into
peaksegdisk_amd._native for this module's tests only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import test_gpu_strand_xcorr as gx
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


def test_emu_xcorr_table_every_size_and_shift(psd):
    gx.scenario_table(gx.as_numpy)


def test_emu_xcorr_three_contigs_in_one_call(psd):
    gx.scenario_three_contigs(gx.as_numpy)


def test_emu_xcorr_wide_products_contention_long_contig(psd):
    gx.scenario_wide(gx.as_numpy)


def test_emu_xcorr_refusals(psd):
    gx.scenario_refusals(gx.as_numpy)


def test_emu_xcorr_device_addresses(psd):
    """reads_on_device = 1 (the emulator's device memory is host memory)"""
    def host_array(v):
        room = np.zeros(v.nbytes + 16, np.uint8)
        lead = -room.ctypes.data % 16
        room[lead:lead + v.nbytes] = np.ascontiguousarray(v).view(np.uint8)
        return room, room.ctypes.data + lead
    gx.scenario_offsets(host_array)


def test_emu_strand_extension(psd):
    gx.scenario_extension(psd, gx.as_numpy)


def test_emu_xcorr_fixture(psd):
    gx.scenario_fixture(psd, gx.as_numpy)


def test_emu_xcorr_recovery(psd):
    gx.scenario_recovery(psd, gx.as_numpy)
