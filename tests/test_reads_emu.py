"""CPU rehearsal of the path from aligned reads: the scenario functions of tests/test_gpu_reads.py
on the SIMT emulator build of the library (tests/emu), which compiles the pile-up's kernels from
the same source.  "Device" memory is host memory there, so the reads are numpy arrays; the
cuda-tensor form runs on the MI355X only.  As in tests/test_dense_emu.py the emulator library is
swapped into peaksegdisk_amd._native for this module's tests only.  The solved scenarios use a
30000-base window of the fixture, which also clips reads at both edges."""
import ctypes
import os
import subprocess

import pytest

import test_gpu_reads as gr
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


def test_emu_reads_pileup_against_numpy(psd):
    gr.scenario_pileup(gr.as_numpy)


def test_emu_reads_three_contigs_in_one_call(psd):
    gr.scenario_three_contigs(gr.as_numpy)


def test_emu_reads_many_adds_to_one_address(psd):
    gr.scenario_one_address(gr.as_numpy)


def test_emu_reads_contig_of_more_than_256_tiles(psd):
    gr.scenario_long_contig(gr.as_numpy)


def test_emu_reads_refusals(psd):
    gr.scenario_refusals(gr.as_numpy)


def test_emu_reads_python_layer_refusals(psd):
    gr.scenario_python_refusals(psd, gr.as_numpy)


def test_emu_reads_fixture_window_equals_from_dense(psd):
    gr.scenario_fixture(psd, gr.as_numpy, [gr.WINDOW])


def test_emu_reads_api_coverage_frame_and_oracle(psd, tmp_path, oracle_det):
    gr.scenario_api(psd, gr.as_numpy, tmp_path, oracle_det)


def test_emu_reads_device_addresses_at_any_offset(psd):
    """reads_on_device = 1 (the emulator's device memory is host memory): read arrays that begin
    at each of the four 4-byte offsets of a 16-byte line, and the refusal of an address that is no
    multiple of 4"""
    import numpy as np
    lib = gr._lib()
    T = lib.peakseg_hip_dense_tile_bases()
    rng = np.random.default_rng(9)
    extent = (1000, 1000 + T + 9)
    s, e, k = gr.reads_around(rng, extent[0], extent[1], 316, T)
    assert s.ctypes.data % 16 == 0 and e.ctypes.data % 16 == 0
    for lead in range(4):
        part = tuple(np.ascontiguousarray(v)[lead:lead + 300] for v in (s, e, k))
        args = gr._read_arguments([part], [extent], "each")
        for shift, want_status in ((0, 0), (2, 18)):
            args[5] = 1
            args[2][0] = part[0].ctypes.data + shift
            cov = np.full(extent[1] - extent[0], gr.SENTINEL, np.int32)
            st = lib.peakseg_hip_reads_pileup_probe(0, *args, cov.ctypes.data, None, None, None, None)
            assert st == want_status, (lead, shift, lib.peakseg_hip_last_error())
            if st == 0:
                assert np.array_equal(cov, gr.numpy_pileup(part[0], part[1], part[2], *extent))
            else:
                assert "contig 0" in lib.peakseg_hip_last_error().decode()
                assert (cov == gr.SENTINEL).all()
