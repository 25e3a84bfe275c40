"""CPU rehearsal of the dense in-memory path: the scenario functions of tests/test_gpu_dense.py on
the SIMT emulator build of the library (tests/emu), which compiles the encoder's kernels from the
same source.  "Device" memory is host memory there, so the input is numpy arrays; the cuda-tensor
form runs on the MI355X only.  As in tests/test_parallel_search_emu.py the emulator library is
swapped into peaksegdisk_amd._native for this module's tests only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import test_gpu_dense as gd
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


def test_emu_dense_encoder_against_numpy(psd):
    gd.scenario_encoder(gd.as_numpy)


def test_emu_dense_encoder_device_addresses_at_any_offset(psd):
    """counts_on_device = 1 (the emulator's device memory is host memory): a contig that begins
    at each of the four 4-byte offsets of a 16-byte line, in one call and in calls of its own"""
    lib = gd._lib()
    T = lib.peakseg_hip_dense_tile_bases()
    rng = np.random.default_rng(3)
    base = gd.geometric_vector(rng, 3 * T + 16)
    assert base.ctypes.data % 16 == 0
    parts = [base[lead:lead + 2 * T + 1 + lead] for lead in range(4)]
    for group in [parts] + [[p] for p in parts]:
        nc = len(group)
        nb = (ctypes.c_longlong * nc)(*[len(p) for p in group])
        ptr = (ctypes.c_void_p * nc)(*[p.ctypes.data for p in group])
        runs = np.zeros(nc, np.int64)
        out = [np.zeros(sum(len(p) for p in group), np.int32) for _ in range(3)]
        st = lib.peakseg_hip_dense_encode_probe(0, nc, nb, ptr, 1, runs.ctypes.data,
                                                out[0].ctypes.data, out[1].ctypes.data,
                                                out[2].ctypes.data, None, None, None)
        assert st == 0
        want = [gd.rle(p) for p in group]
        k = int(runs.sum())
        assert runs.tolist() == [len(w[0]) for w in want]
        for j in range(3):
            assert np.array_equal(out[j][:k], np.concatenate([w[j] for w in want]))


def test_emu_dense_encoder_refusals(psd):
    gd.scenario_encoder_refusals(gd.as_numpy)


def test_emu_dense_mono27ac_against_the_oracle(psd, oracle_det, known_answers, tmp_path):
    gd.scenario_mono27ac(psd, oracle_det, known_answers, tmp_path, gd.as_numpy)


def test_emu_dense_three_contigs_against_the_oracle(psd, oracle_det, tmp_path):
    gd.scenario_three_contigs(psd, oracle_det, tmp_path, gd.as_numpy)


def test_emu_dense_api_equals_the_directory_path(psd, tmp_path):
    gd.scenario_api(psd, tmp_path, gd.as_numpy)


def test_emu_dense_cpu_tensors_are_host_memory(psd):
    """a CPU torch tensor is passed as host memory, a mix of kinds is refused by name"""
    import torch
    v = gd.three_contigs()[1]
    a = psd.ProblemSet.from_dense([torch.from_numpy(v)], [(0, 40.0)])
    b = psd.ProblemSet.from_dense([v], [(0, 40.0)])
    try:
        a.solve()
        b.solve()
        for x, y in zip(a.segment_columns()[0], b.segment_columns()[0]):
            assert np.array_equal(x, y)
        assert np.array_equal(a.loss(0), b.loss(0))
    finally:
        a.close()
        b.close()
