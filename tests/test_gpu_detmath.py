"""Every form of include/peakseg_detmath_core.h (psd_exp, psd_log, the fused psd_exp2 / psd_log2 /
psd_exp2_log and the branch-free psd_exp_nb / psd_log_nb / psd_log_wild_nb), in both of the device's
instantiations (plain constants: the throughput and packed builds; _vk, constants in vector
registers: the latency build), against the host's, bit for bit -- and the device's division.

The arguments are those of tests/detmath_points.py: the cell edges of the log's table, the rounding
points of the exp's index, the ends of the range, the thresholds of the slow paths and the special
values, laid out so that a wave holds no rare lane, one (the first, the last), all, or every other:
the rare-argument branch is wave-uniform, every lane of a wave that takes it evaluates the slow
form, and the common lanes must keep their hot-path value.

The scenario functions are shared with the emulator rehearsal (tests/test_detmath_forms_emu.py).
The host's side is oracle_math_form_vec (oracle/peakseg_oracle.c)."""
import ctypes

import numpy as np
import pytest

import detmath_points as dp

GPU = pytest.mark.gpu
FORMS = ["exp", "log", "exp2", "log2", "exp2_log", "exp_nb", "log_nb", "log_wild_nb"]
EXPECTED_RARE = {5: dp.rare_exp_nb, 6: dp.rare_log_nb, 7: dp.rare_log_wild_nb}


@pytest.fixture(scope="module")
def psd():
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd
    from peaksegdisk_amd import _native
    assert _native.lib.peakseg_hip_device_count() >= 1, "no HIP device: GPU tests need an MI355X"
    return peaksegdisk_amd


def _lib():
    from peaksegdisk_amd import _native
    return _native.lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Outputs:
    def __init__(self, n):
        self.y0, self.y1, self.lz = np.full(n, 7.0), np.full(n, 7.0), np.full(n, 7.0)
        self.rare = np.full(n, 7, dtype=np.int32)

    def pointers(self):
        return [_ptr(self.y0), _ptr(self.y1), _ptr(self.lz), _ptr(self.rare)]


def device_forms(form, which, x0, x1, z):
    out = Outputs(x0.size)
    st = _lib().peakseg_hip_math_forms_probe(form, which, x0.size, _ptr(x0), _ptr(x1), _ptr(z),
                                            *out.pointers())
    assert st == 0, (FORMS[form], which, st)
    return out


def host_forms(oracle, form, x0, x1, z):
    out = Outputs(x0.size)
    st = oracle.lib.oracle_math_form_vec(ctypes.c_int(form), ctypes.c_int(x0.size), _ptr(x0),
                                         _ptr(x1), _ptr(z), *out.pointers())
    assert st == 0, FORMS[form]
    return out


# ---- the arguments of each form -------------------------------------------------------------------

def exp_operand():
    """(common values, rare values, structured points) of an exp argument"""
    pts = dp.exp_points()
    near = np.concatenate([dp.exp_near_points(), dp.exp_specials(), [1e300, -1e300, 745.0, -746.0]])
    rare = near[~dp.is_exp_common(near)]
    rare = np.concatenate([rare[:-12:7], rare[-12:]])  # some of the near points, every special
    common = dp.exp_rounding_points()
    return common[dp.is_exp_common(common)], rare, pts


def log_operand():
    pts = dp.log_points()
    near = np.concatenate([dp.log_near_points(), dp.log_specials()])
    rare = near[~dp.is_log_common(near)]
    return dp.log_cell_points(), rare, pts


def form_cases(form):
    """-> list of (x0, x1, z): one layout for the forms of one argument; for the fused forms the rare
    elements in each operand alone and in all"""
    e, lg = exp_operand(), log_operand()
    if form in (0, 5):
        x = dp.layout(*e[:2], 0, e[2])[0]
        return [(x, np.zeros_like(x), np.zeros_like(x))]
    if form in (1, 6, 7):
        x = dp.layout(*lg[:2], 0, lg[2])[0]
        return [(x, np.zeros_like(x), np.zeros_like(x))]
    operands = {2: [e, e], 3: [lg, lg], 4: [e, e, lg]}[form]
    cases = []
    for arrays, masks in dp.fused_layouts(operands):
        # the placement is what it says: in the layout's groups only the chosen operands are rare
        commons = [dp.is_log_common if o is lg else dp.is_exp_common for o in operands]
        head = 320 * min(len(o[1]) for o in operands)
        for x, m, is_common in zip(arrays, masks, commons):
            assert np.array_equal(~is_common(x[:head]), m[:head])
        if len(arrays) == 2:
            arrays = arrays + [np.zeros_like(arrays[0])]
        cases.append(tuple(np.ascontiguousarray(a) for a in arrays))
    return cases


def _describe(name, got, want, args):
    bad = np.flatnonzero(got != want)
    rows = ["%s: %d of %d differ" % (name, bad.size, got.size)]
    for i in bad[:6]:
        rows.append("  [%d] lane %d args %s device %s host %s" % (
            i, i % 64, " ".join("%016x" % int(dp.bits(a)[i]) for a in args),
            "%016x" % int(got[i]), "%016x" % int(want[i])))
    return "\n".join(rows)


# ---- the scenarios ------------------------------------------------------------------------------

def scenario_forms(psd, oracle, sets=(0, 1), forms=range(8)):
    """device == host in every output slot of every form and set, as bit patterns (NaN results
    included) and the records as integers; the records also equal what the header's comments say,
    recomputed from the arguments' bits"""
    failures = []
    for form in forms:
        for case, (x0, x1, z) in enumerate(form_cases(form)):
            assert x0.size % 256 and x0.size % 64
            want = host_forms(oracle, form, x0, x1, z)
            if form in EXPECTED_RARE:
                assert np.array_equal(want.rare, EXPECTED_RARE[form](x0)), FORMS[form]
            else:
                assert not want.rare.any()
            for which in sets:
                got = device_forms(form, which, x0, x1, z)
                for slot in ("y0", "y1", "lz"):
                    g, w = getattr(got, slot).view(np.uint64), getattr(want, slot).view(np.uint64)
                    if not np.array_equal(g, w):
                        failures.append(_describe("%s set %d case %d %s" % (
                            FORMS[form], which, case, slot), g, w, (x0, x1, z)))
                if not np.array_equal(got.rare, want.rare):
                    failures.append(_describe("%s set %d case %d rare" % (FORMS[form], which, case),
                                              got.rare, want.rare, (x0, x1, z)))
    assert not failures, "\n".join(failures)


def div_operands(n_subnormal):
    """-> (a, b, subnormal): the operands of scenario_div and the mask of the subnormal quotients"""
    oa, ob = dp.overflow_pairs()
    # quotients at the edge of overflow: the largest finite ones and the first that round to inf
    eb = np.array([float.fromhex(h) for h in ("0x1.8p-1", "0x1.fffffffffffffp-1",
                                              "0x1.0000000000001p-1", "0x1.5555555555555p-1")])
    ea = np.concatenate([dp.around(dp.DBL_MAX * v, 3) for v in eb])
    eb = np.repeat(eb, 7)
    ea, eb = np.concatenate([ea, -ea]), np.concatenate([eb, eb])
    # quotients that round to +-0
    za = np.array([5e-324, -5e-324, 5e-324, -5e-324, 1e-300, -1e-300, dp.DBL_MIN])
    zb = np.array([4.0, 4.0, -4.0, -4.0, 1e300, 1e300, -2.0 ** 60])
    sa, sb = dp.subnormal_quotient_pairs(n_subnormal)
    nan = dp.from_bits([dp.NAN_PAYLOAD])[0]
    pa = np.array([1.0, -1.0, 0.0, -0.0, np.inf, -np.inf, np.inf, -np.inf, 3.0, -3.0, 0.0, nan, 1.0,
                   nan, np.inf])
    pb = np.array([0.0, 0.0, 0.0, 0.0, np.inf, np.inf, 2.0, -2.0, np.inf, np.inf, 5.0, 1.0, nan,
                   np.inf, nan])
    a = np.ascontiguousarray(np.concatenate([oa, ea, za, sa, pa]))
    b = np.ascontiguousarray(np.concatenate([ob, eb, zb, sb, pb]))
    return a, b


def scenario_div(psd, oracle, n_subnormal=100000, repaired=True):
    """psd_div (op 2 of peakseg_hip_math_probe) is the host's a / b on every normal, zero, infinite
    and NaN quotient (bit for bit; a NaN for a NaN: IEEE 754 leaves the payload of a division's NaN
    open) -- quotients at the edge of overflow and quotients that round to +-0, x/0, 0/0, inf/inf,
    inf/x, x/inf, NaN operands -- but for the one kind its contract excludes
    (include/peakseg_detmath.h): a quotient of finite operands that overflows, in the four sign
    combinations, is +-DBL_MAX where psd_div_repair is applied (repaired: the device) and +-inf
    where psd_div is the division operator (the host branch, which the emulator compiles).  On
    subnormal quotients, where the residual of psd_div_repair is not exact, it is the IEEE quotient
    wherever the compiler's own sequence (op 3) is; how often that sequence is off there is
    returned."""
    a, b = div_operands(n_subnormal)
    with np.errstate(all="ignore"):
        want = a / b
    x = np.ascontiguousarray(np.concatenate([a, b]))
    got = {}
    for op in (2, 3):
        y = np.full(a.size, 7.0)
        assert _lib().peakseg_hip_math_probe(op, a.size, x.ctypes.data, y.ctypes.data) == 0
        got[op] = y
    overflow = np.isinf(want) & np.isfinite(a) & (b != 0.0)
    assert overflow.sum() >= 20 + 4
    # the division itself overflows as IEEE division does; the repair then takes the neighbour
    assert np.array_equal(got[3][overflow], want[overflow])
    if repaired:
        want[overflow] = np.copysign(dp.DBL_MAX, want[overflow])
    sub = (want != 0) & (np.abs(want) < dp.DBL_MIN)
    assert sub.sum() > n_subnormal // 2 and np.isinf(want).sum() >= 4 and np.isnan(want).sum() >= 8
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got[2]), nan)
    rest = ~sub & ~nan
    bad = np.flatnonzero(got[2].view(np.uint64)[rest] != want.view(np.uint64)[rest])
    assert bad.size == 0, [(a[rest][i].hex(), b[rest][i].hex(), got[2][rest][i].hex(),
                            want[rest][i].hex()) for i in bad[:8]]
    raw_ok = got[3].view(np.uint64) == want.view(np.uint64)
    both = sub & raw_ok
    assert np.array_equal(got[2].view(np.uint64)[both], want.view(np.uint64)[both])
    off = int(np.sum(sub & ~raw_ok))
    print("subnormal quotients: %d; the compiler's sequence off on %d, psd_div on %d" % (
        sub.sum(), off, int(np.sum(sub & (got[2].view(np.uint64) != want.view(np.uint64))))))
    return off


def scenario_refusals(psd, oracle):
    """form 8, set 2 and a negative n are refused before any launch (the outputs stay as they were);
    n = 0 is nothing to do"""
    x = np.ones(4)
    for form, which, n, status in ((8, 0, 4, -1), (-1, 0, 4, -1), (0, 2, 4, -1), (0, -1, 4, -1),
                                   (0, 0, -1, -1), (0, 0, 0, 0), (7, 1, 0, 0)):
        out = Outputs(4)
        st = _lib().peakseg_hip_math_forms_probe(form, which, n, _ptr(x), _ptr(x), _ptr(x),
                                                *out.pointers())
        assert st == status, (form, which, n, st)
        assert np.all(out.y0 == 7.0) and np.all(out.rare == 7)
    # an argument array a form does not read may be left out
    out = Outputs(4)
    assert _lib().peakseg_hip_math_forms_probe(0, 0, 4, _ptr(x), None, None, _ptr(out.y0), None,
                                              None, None) == 0
    assert np.array_equal(out.y0, oracle.math("exp", x))


# ---- on the MI355X -------------------------------------------------------------------------------

@GPU
@pytest.mark.parametrize("form", range(8), ids=FORMS)
def test_forms_device_equals_host(psd, oracle_det, form):
    scenario_forms(psd, oracle_det, forms=[form])


@GPU
def test_division_device_equals_host(psd, oracle_det):
    scenario_div(psd, oracle_det)


@GPU
def test_forms_probe_refusals(psd, oracle_det):
    scenario_refusals(psd, oracle_det)
