"""The segment statistics entries on a machine without a GPU: the real library exports the four
symbols, the binding declares them, and the header names them with their definitions."""
import os

import pytest

from conftest import ROOT

SYMBOLS = ("peakseg_hip_problem_set_pack_segment_stats",
           "peakseg_hip_problem_set_packed_segment_stats_download",
           "peakseg_hip_segment_stats_tile_runs", "peakseg_hip_segment_stats_last_ms")


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as entry
    entry.build_hip()
    from peaksegdisk_amd import _native
    return _native


def test_segment_stats_symbols(native):
    for name in SYMBOLS:
        assert hasattr(native.lib, name), name
        assert name in native.EXPORTED_SYMBOLS
    T = native.lib.peakseg_hip_segment_stats_tile_runs()
    assert T >= 256 and T % 256 == 0
    # nothing to report and nothing to refuse without a set
    assert native.lib.peakseg_hip_problem_set_pack_segment_stats(
        None, None, None, None, None, None, None) == -1
    assert native.lib.peakseg_hip_problem_set_packed_segment_stats_download(
        None, None, None, None, None) == -1


def test_segment_stats_header_and_python_layer(native):
    with open(os.path.join(ROOT, "include", "peaksegdisk_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert name in header, name
    for word in ("summitStart", "summitEnd", "run_end[i] - weight[i]", "count[i] * weight[i]"):
        assert word in header, word
    import inspect
    import peaksegdisk_amd as psd
    assert hasattr(psd.ProblemSet, "segment_stats")
    assert inspect.signature(psd.PeakSegFPOP_dense).parameters["stats"].default is False
