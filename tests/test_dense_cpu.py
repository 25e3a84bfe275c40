"""The dense in-memory entries on a machine without a GPU: the real library's symbols, the order
of its argument checks, the Python layer's refusals, and the claim the device path rests on --
psd_log of the integer extremes is the pair of extremes of psd_log."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as entry
    entry.build_hip()
    from peaksegdisk_amd import _native
    return _native


def _no_gpu(native):
    return native.lib.peakseg_hip_device_count() == 0


def _create(native, vectors, problems, lengths=None):
    nc = len(vectors)
    nb = (ctypes.c_longlong * nc)(*(lengths or [len(v) for v in vectors]))
    ptr = (ctypes.c_void_p * nc)(*[v.ctypes.data if v is not None else None for v in vectors])
    k = len(problems)
    pc = (ctypes.c_int * k)(*[c for c, _ in problems])
    pp = (ctypes.c_double * k)(*[p for _, p in problems])
    h = ctypes.c_void_p()
    st = native.lib.peakseg_hip_problem_set_create_dense(0, nc, nb, ptr, 0, k, pc, pp, 0,
                                                         ctypes.byref(h))
    if st == 0:
        native.lib.peakseg_hip_problem_set_destroy(h)
    return st


def test_dense_symbols_and_status_text(native):
    for name in ("peakseg_hip_problem_set_create_dense", "peakseg_hip_problem_set_pack_segments",
                 "peakseg_hip_problem_set_packed_segments_download", "peakseg_hip_problem_set_loss",
                 "peakseg_hip_dense_encode_probe", "peakseg_hip_dense_tile_bases"):
        assert hasattr(native.lib, name), name
        assert name in native.EXPORTED_SYMBOLS
    T = native.lib.peakseg_hip_dense_tile_bases()
    assert T > 0 and T % 256 == 0
    assert native.ERROR_DENSE_ARGUMENTS == 17
    text = native.status_message(17, "f", "1", "d")
    assert text.startswith("error code 17") and "dense" in text
    import peaksegdisk_amd
    assert "PeakSegFPOP_dense" in peaksegdisk_amd.__all__


def test_dense_argument_checks_in_their_order(native):
    v = np.array([1, 1, 5, 2], np.int32)
    empty = np.zeros(0, np.int32)
    # penalties first, even when the data is bad too
    assert _create(native, [empty], [(0, float("nan"))]) == 1
    assert _create(native, [empty], [(0, 1.0), (0, -0.5)]) == 2
    assert _create(native, [None], [(0, float("nan"))], lengths=[2 ** 31]) == 1
    # what the host can see
    assert _create(native, [v, empty], [(0, 1.0), (1, float("inf"))]) == 9
    assert "contig 1" in native.last_error()
    assert _create(native, [v, None], [(0, 1.0)], lengths=[4, 2 ** 31]) == 17  # (never read)
    assert "contig 1" in native.last_error() and "2^31" in native.last_error()
    if _no_gpu(native):
        # then the device: there is no host encoder
        assert _create(native, [v], [(0, 1.0), (0, float("inf"))]) == native.ERROR_NO_HIP_DEVICE
        nb = (ctypes.c_longlong * 1)(4)
        ptr = (ctypes.c_void_p * 1)(v.ctypes.data)
        runs = np.zeros(1, np.int64)
        st = native.lib.peakseg_hip_dense_encode_probe(0, 1, nb, ptr, 0, runs.ctypes.data, None,
                                                       None, None, None, None, None)
        assert st == native.ERROR_NO_HIP_DEVICE
    nb = (ctypes.c_longlong * 1)(0)
    ptr = (ctypes.c_void_p * 1)(None)
    assert native.lib.peakseg_hip_dense_encode_probe(0, 1, nb, ptr, 0, None, None, None, None,
                                                     None, None, None) == 9


def test_dense_python_layer_refusals(native):
    import peaksegdisk_amd as psd
    from peaksegdisk_amd import ProblemSet
    good = np.array([1, 1, 5, 2], np.int32)
    with pytest.raises(ValueError, match="contig 1 has dtype int64"):
        ProblemSet.from_dense([good, good.astype(np.int64)], [(0, 1.0)])
    with pytest.raises(ValueError, match="contig 0 is not a contiguous"):
        ProblemSet.from_dense([np.arange(10, dtype=np.int32)[::2]], [(0, 1.0)])
    with pytest.raises(ValueError, match="contig 0 is not a contiguous"):
        ProblemSet.from_dense([np.zeros((2, 2), np.int32)], [(0, 1.0)])
    with pytest.raises(ValueError, match="contig 1 is a list"):
        ProblemSet.from_dense([good, [1, 2]], [(0, 1.0)])
    import torch
    with pytest.raises(ValueError, match="contig 0 has dtype torch.int64"):
        ProblemSet.from_dense([torch.arange(4)], [(0, 1.0)])
    with pytest.raises(ValueError, match="contig 0 is not a contiguous"):
        ProblemSet.from_dense([torch.arange(8, dtype=torch.int32)[::2]], [(0, 1.0)])
    with pytest.raises(ValueError, match="pen.num"):
        psd.PeakSegFPOP_dense(good, [-1.0])
    with pytest.raises(ValueError, match="pen.num"):
        psd.PeakSegFPOP_dense(good, [float("nan")])
    with pytest.raises(ValueError, match="must be integer"):
        psd.PeakSegFPOP_dense(np.array([0.5, 1.0]), [1.0])
    with pytest.raises(ValueError, match="one list per vector"):
        psd.PeakSegFPOP_dense([good, good], [[1.0]])
    if _no_gpu(native) and native.lib.peakseg_hip_device_count() == 0:
        with pytest.raises(psd.PeakSegError) as e:
            psd.PeakSegFPOP_dense(good, [1.0, float("inf")])
        assert e.value.status == 12
        with pytest.raises(psd.PeakSegError) as e:
            psd.PeakSegFPOP_dense([1, 1, 5, 2], [1.0])   # a plain list of integers is one vector
        assert e.value.status == 12
        with pytest.raises(psd.PeakSegError) as e:
            psd.PeakSegFPOP_dense(np.zeros(0, np.int32), [1.0])
        assert e.value.status == 9


_LOG_PROBE = r"""
#include <stdio.h>
#include <math.h>
#include "peakseg_detmath.h"
/* psd_log is strictly increasing on the integers the encoder can report, so the logs of the integer
 * minimum and maximum of a contig are the minimum and maximum of the logs of its counts */
static int range(long long lo, long long hi) {
  double prev = psd_log((double)lo);
  if (lo == 0 && !(prev == -INFINITY)) return 1;
  for (long long k = lo + 1; k <= hi; k++) {
    const double cur = psd_log((double)k);
    if (!(cur > prev)) { printf("not increasing at %lld\n", k); return 1; }
    /* the per-bin loop's running minimum / maximum over lo..k (drv:198-204) */
    prev = cur;
  }
  return 0;
}
int main(void) {
  if (range(0, 1000000)) return 1;
  if (range(2147483647ll - 1000, 2147483647ll)) return 1;
  if (!(psd_log(1000000.0) < psd_log(2147483647.0 - 1000))) return 1;
  /* a contig in any order: the loop of the host-encoded creator against the two logs */
  const int v[] = {7, 0, 2147483647, 3, 1000000, 1, 2147482999};
  double mn = INFINITY, mx = -INFINITY;
  int imn = v[0], imx = v[0];
  for (unsigned i = 0; i < sizeof v / sizeof v[0]; i++) {
    const double l = psd_log((double)v[i]);
    if (l < mn) mn = l;
    if (mx < l) mx = l;
    if (v[i] < imn) imn = v[i];
    if (v[i] > imx) imx = v[i];
  }
  if (mn != psd_log((double)imn) || mx != psd_log((double)imx)) return 1;
  printf("ok\n");
  return 0;
}
"""


def test_log_of_the_integer_extremes_is_the_extreme_of_the_logs(tmp_path):
    """every count 0 ... 10^6 and 2^31 - 1000 ... 2^31 - 1: psd_log (the host build of
    include/peakseg_detmath.h, which the library's host code calls) is strictly increasing, so
    psd_log(min), psd_log(max) is the pair the per-bin loop of peakseg_hip_problem_set_create
    finds"""
    src = tmp_path / "log_probe.cpp"
    src.write_text(_LOG_PROBE)
    exe = str(tmp_path / "log_probe")
    subprocess.run(["g++", "-O2", "-std=gnu++17", "-ffp-contract=off",
                    "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout
