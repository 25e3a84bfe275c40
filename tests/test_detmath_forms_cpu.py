"""The host's side of include/peakseg_detmath.h and include/peakseg_detmath_core.h beyond accuracy
(tests/test_detmath.py): the committed tables and the exactness properties the comments of
psd_log_core state about them, every form of the core against the single functions on the arguments
of tests/detmath_points.py, the records of the branch-free forms against what the header says, and
psd_div_repair on subnormal quotients."""
import ctypes
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import detmath_points as dp
import test_gpu_detmath as gd
from conftest import ROOT

TABLES = os.path.join(ROOT, "include", "peakseg_detmath_tables.h")


# ---- the tables ---------------------------------------------------------------------------------

def test_tables_are_what_the_generator_prints():
    pytest.importorskip("mpmath")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_detmath_tables.py")],
                         capture_output=True, check=True).stdout
    assert out == open(TABLES, "rb").read()


def _table(name):
    text = open(TABLES).read()
    body = re.search(r"#define %s \\\n((?:.*\\\n)*.*)\n" % name, text).group(1)
    return [float.fromhex(t) for t in re.findall(r"-?0x[0-9a-f.]+p[+-]\d+", body)]


def test_log_table_exactness_properties():
    """the three properties the comments of psd_log_core rely on, in exact rational arithmetic"""
    invc, hi, lo = _table("PSD_LOG_INVC_INIT"), _table("PSD_LOG_LOGC_HI_INIT"), _table("PSD_LOG_LOGC_LO_INIT")
    assert len(invc) == len(hi) == len(lo) == 129 and len(_table("PSD_EXP_TABLE_INIT")) == 256
    ln2_hi = Fraction(float.fromhex("0x1.62e42fee00000p-1"))
    # logc_hi[J] is a multiple of 2^-42, and k LN2_HI + logc_hi[J] is a double for every |k| <= 1074:
    # both are whole multiples of 2^-42, and a whole number below 2^53 in size is a double
    step = (ln2_hi * 2 ** 42)
    assert step.denominator == 1 and step > 0
    for J in range(129):
        h = Fraction(hi[J]) * 2 ** 42
        assert h.denominator == 1 and h >= 0, J
        assert 1074 * step + h < 2 ** 53, J
        for k in (-1074, -1, 1, 1074):
            w = k * ln2_hi + Fraction(hi[J])
            assert Fraction(float(w)) == w, (J, k)
    # m invc[J] - 1 is exact for J = 0 and J = 128: over the whole of either cell
    assert invc[0] == 1.0 and invc[128] == 0.5 and hi[0] == 0.0 and lo[0] == 0.0
    for J, cell in ((0, dp.around(1.0 + 2.0 ** -9, 8).tolist() + [1.0, float.fromhex("0x1.00fffffffffffp0")]),
                    (128, dp.around(2.0 - 2.0 ** -9, 8).tolist() + [float.fromhex("0x1.ff00000000000p0"),
                                                                 float.fromhex("0x1.fffffffffffffp0")])):
        for m in cell:
            assert int(dp.log_index([m])[0][0]) == J
            r = Fraction(m) * Fraction(invc[J]) - 1
            assert Fraction(float(r)) == r, (J, m)
    # |r| <= 2^-8 at both edges of every cell (the cell of J: (2J-1)/256 <= m - 1 < (2J+1)/256)
    for J in range(129):
        lo_edge = Fraction(max(2 * J - 1, 0), 256) + 1
        hi_edge = Fraction(min(2 * J + 1, 256), 256) + 1
        for m in (lo_edge, hi_edge):
            assert abs(m * Fraction(invc[J]) - 1) <= Fraction(1, 256), J


# ---- the values themselves ------------------------------------------------------------------------

PINNED = {"log_cells": ("log", dp.log_cell_points), "log_near": ("log", dp.log_near_points),
          "exp_rounding": ("exp", dp.exp_rounding_points), "exp_near": ("exp", dp.exp_near_points)}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_values_at_the_edges_are_pinned(oracle_det, name):
    """tests/golden/detmath_pins.json: SHA-256 of the arguments' and of the results' bits for each
    class of tests/detmath_points.py.  Host and device are built from one source, so a change of a
    constant, of the table index or of a rounding moves both alike and stays accurate: only the
    recorded bits notice that every stored function of every solve has changed with it.  (The index
    of psd_log_core rounding down at a cell edge, 0x1000 -> 0x0fff, is such a change.)"""
    import hashlib
    import json
    fn, points = PINNED[name]
    x = points()
    y = oracle_det.math(fn, x)
    pins = json.load(open(os.path.join(ROOT, "tests", "golden", "detmath_pins.json")))[name]
    assert hashlib.sha256(dp.bits(x).tobytes()).hexdigest() == pins["arguments"], \
        "the class itself has changed: record it anew"
    assert hashlib.sha256(y.view(np.uint64).tobytes()).hexdigest() == pins["results"]


# ---- the forms on the host ------------------------------------------------------------------------

def _same(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("form", [2, 3, 4], ids=["exp2", "log2", "exp2_log"])
def test_fused_forms_equal_the_single_functions(oracle_det, form):
    """bit for bit in every slot, wherever the rare element sits"""
    for x0, x1, z in gd.form_cases(form):
        got = gd.host_forms(oracle_det, form, x0, x1, z)
        one = "log" if form == 3 else "exp"
        assert _same(got.y0, oracle_det.math(one, x0)) and _same(got.y1, oracle_det.math(one, x1))
        if form == 4:
            assert _same(got.lz, oracle_det.math("log", z))
        assert not got.rare.any()


@pytest.mark.parametrize("form", [5, 6, 7], ids=["exp_nb", "log_nb", "log_wild_nb"])
def test_branch_free_forms(oracle_det, form):
    """psd_exp / psd_log wherever the record stays 0; the record is what the header's comments say
    (exp_nb: !(|x| <= 708); log_nb: not positive-normal-finite and not negative; log_wild_nb: positive
    subnormal only); the selects of log_nb (negative) and log_wild_nb (negative, 0, +inf, NaN) give
    what psd_log_slow gives, a NaN for a NaN"""
    (x, x1, z), = gd.form_cases(form)
    got = gd.host_forms(oracle_det, form, x, x1, z)
    want = oracle_det.math("exp" if form == 5 else "log", x)
    expected = gd.EXPECTED_RARE[form](x)
    assert np.array_equal(got.rare, expected)
    assert 0 < expected.sum() < x.size
    # each element's record is its own: the layouts put rare elements next to common ones
    common = expected == 0
    neg = x < 0.0
    wild = np.zeros(x.size, dtype=bool) if form == 5 else neg
    if form == 7:
        wild = neg | (x == 0.0) | (x == np.inf) | np.isnan(x)
        assert np.any(x == 0.0) and np.any(x == np.inf) and np.any(np.isnan(x))
    assert _same(got.y0[common & ~wild], want[common & ~wild])
    if form == 5:
        return
    # the arguments that the selects answer: no record, and what psd_log_slow returns
    assert neg.sum() >= 3 and np.all(common[wild])
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got.y0[wild]), nan[wild])
    assert _same(got.y0[wild & ~nan], want[wild & ~nan])


def test_fused_forms_see_every_placement():
    """the layouts of the fused forms: rare elements in each operand alone and in all, a partial last
    wave and a partial last workgroup"""
    for form, n_ops in ((2, 2), (3, 2), (4, 3)):
        cases = gd.form_cases(form)
        assert len(cases) == n_ops + 1
        for x0, x1, z in cases:
            assert x0.size == x1.size == z.size and x0.size % 64 == 37 and x0.size % 256 != 0


# ---- division repair on subnormal quotients ----------------------------------------------------------

def test_division_repair_never_moves_a_correct_subnormal_quotient(oracle_det):
    """Where the quotient is subnormal the residual fma(-q, b, a) of psd_div_repair is rounded, and a
    neighbour of the IEEE quotient is not always restored (24,668 of 6 million such cases were not).
    What holds, and what the device needs of it as long as its own division is right there
    (tests/test_gpu_detmath.py counts that): a correct quotient stays."""
    a, b = dp.subnormal_quotient_pairs(1000000)
    want = a / b
    x = np.ascontiguousarray(np.concatenate([want, a, b]))
    y = np.empty(a.size)
    oracle_det.lib.oracle_div_repair_vec(ctypes.c_int(a.size), x.ctypes.data_as(ctypes.c_void_p),
                                         y.ctypes.data_as(ctypes.c_void_p))
    assert _same(y, want)
