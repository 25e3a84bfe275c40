"""Arguments for the tests of include/peakseg_detmath.h and include/peakseg_detmath_core.h that land
on the structure of the code instead of between its edges (a plain module: tests/test_detmath.py,
tests/test_detmath_forms_cpu.py, tests/test_gpu_detmath.py and its emulator rehearsal import it).

Every class asserts its own trigger from its own numbers, in integer arithmetic on the bit patterns:
a class that no longer reaches the edge it was built for fails here, loudly, instead of passing its
tests quietly.  Needs numpy only: ln 2 is summed as a rational number."""
import functools
from fractions import Fraction

import numpy as np

DBL_MIN = float.fromhex("0x1p-1022")
DBL_MAX = float.fromhex("0x1.fffffffffffffp+1023")
SUB_MAX = float.fromhex("0x0.fffffffffffffp-1022")
EXP_OVERFLOW = float.fromhex("0x1.62e42fefa39efp+9")    # psd_exp_slow: above it +inf
EXP_UNDERFLOW = float.fromhex("-0x1.74910d52d3052p+9")  # psd_exp_slow: below it 0
INV_LN2N = float.fromhex("0x1.71547652b82fep+7")        # PSD_INV_LN2N
NAN_PAYLOAD = 0x7ff8000000abcdef
NAN_NEG_PAYLOAD = 0xfff80000000fedcb


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint64).view(np.float64)


def around(x, k):
    """x and the k doubles on either side of it, in increasing order of the bit pattern (x > 0:
    increasing; x < 0: decreasing), never across zero"""
    u = int(bits([x])[0])
    assert (u & 0x7fffffffffffffff) > k
    return from_bits(np.arange(u - k, u + k + 1, dtype=np.uint64))


@functools.lru_cache(maxsize=None)
def ln2():
    """ln 2 as a rational number, wrong by less than 2^-330: the sum of 1 / (k 2^k)"""
    return sum(Fraction(1, k << k) for k in range(1, 331))


def nearest_double(q):
    """the double nearest to the rational q (int / int is correctly rounded)"""
    return q.numerator / q.denominator


# ---- log ----------------------------------------------------------------------------------------

def log_index(x):
    """(J, k) of psd_log_core for positive normal x: J = (mant_hi + 0x1000) >> 13"""
    top = (bits(x) >> np.uint64(32)).astype(np.int64)
    return ((top & 0xfffff) + 0x1000) >> 13, (top >> 20) - 1023


def is_log_common(x):
    """positive, normal and finite: the unsigned compare of the high word in psd_log"""
    top = (bits(x) >> np.uint64(32)).astype(np.int64)
    return ((top - 0x00100000) & 0xffffffff) < 0x7fe00000


@functools.lru_cache(maxsize=None)
def log_cell_points():
    """the 128 cell edges 1 + (2J+1)/256 and the 129 table points 1 + J/128 with the four doubles on
    either side, within [1, 2], times 2^k for k in -1022, -1, 0, 1, 52, 1023; the finite ones"""
    ms = [1.0 + (2 * J + 1) / 256.0 for J in range(128)] + [1.0 + J / 128.0 for J in range(129)]
    m = np.concatenate([around(v, 4) for v in ms])
    m = np.unique(m[(m >= 1.0) & (m <= 2.0)])
    # the trigger: every J and J + 1 meet within four units
    J, k = log_index(m[m < 2.0])
    u = bits(m[m < 2.0]).astype(np.int64)
    assert np.all(k == 0)
    for j in range(128):
        lo, hi = u[J == j], u[J == j + 1]
        assert len(lo) and len(hi) and 0 < hi.min() - lo.max() <= 4, j
    with np.errstate(over="ignore"):
        x = np.concatenate([np.ldexp(m, e) for e in (-1022, -1, 0, 1, 52, 1023)])
    x = x[np.isfinite(x)]
    assert np.all(is_log_common(x)) and 13000 < x.size < 15000
    return x


@functools.lru_cache(maxsize=None)
def log_near_points():
    """the eight doubles on either side of 1, 0.5, 2 and DBL_MIN (below DBL_MIN they are subnormal),
    the ends of the range, and the smallest subnormals"""
    x = np.concatenate([around(v, 8) for v in (1.0, 0.5, 2.0, DBL_MIN)] +
                       [[5e-324, 1e-323, SUB_MAX, DBL_MAX]])
    c = x[is_log_common(x)]
    J, k = log_index(c)
    assert np.any((J == 0) & (k == 0)) and np.any((J == 128) & (k == -1))
    assert np.sum(~is_log_common(x)) == 8 + 3  # the subnormals
    return x


def log_specials():
    return np.concatenate([[0.0, -0.0, -1.0, -DBL_MIN, -5e-324, np.inf, -np.inf],
                           from_bits([NAN_PAYLOAD, NAN_NEG_PAYLOAD])])


def log_points():
    return np.concatenate([log_cell_points(), log_near_points(), log_specials()])


# ---- exp ----------------------------------------------------------------------------------------

EXP_K = (list(range(-300, 300)) + list(range(90500, 90700)) + list(range(-90700, -90500)) +
         list(range(-95500, -95300)) + list(range(-131077, -131067)))


def exp_index(x):
    """ki of psd_exp_core for finite |x| < 2^40: the low bits of fma(x, PSD_INV_LN2N, 0x1.8p52).
    That sum lies in [2^52, 2^53), where doubles are the whole numbers: the one rounding of the fma
    is the rounding of the exact product to a whole number, ties to even -- round() of a Fraction."""
    c = Fraction(INV_LN2N)
    return np.array([round(Fraction(float(v)) * c) for v in np.asarray(x).ravel()], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def exp_rounding_points():
    """(k + 1/2) ln2/128 -- where rint(x 128/ln2) changes -- and k ln2/128 -- where the reduced
    argument changes sign -- with the three doubles on either side"""
    step = ln2() / 128
    half = np.array([nearest_double((Fraction(2 * k + 1, 2)) * step) for k in EXP_K])
    whole = np.array([nearest_double(k * step) for k in EXP_K if k != 0])
    offs = np.arange(-3, 4, dtype=np.int64)
    xh = from_bits((bits(half).astype(np.int64)[:, None] + offs[None, :]).astype(np.uint64))
    xw = from_bits((bits(whole).astype(np.int64)[:, None] + offs[None, :]).astype(np.uint64))
    # the trigger: around every half-way point both ki = k and ki = k + 1 occur
    ki = exp_index(xh).reshape(xh.shape)
    want = np.array(EXP_K, dtype=np.int64)
    assert np.all(ki.min(axis=1) == want) and np.all(ki.max(axis=1) == want + 1)
    allk = np.concatenate([ki.ravel(), exp_index(xw)])
    assert np.any((allk < 0) & ((allk & 127) == 0)) and np.any((allk < 0) & ((allk & 127) == 127))
    assert np.any(allk >> 7 == -1024) and np.any(allk >> 7 == -1025)  # subnormal results
    x = np.concatenate([xh.ravel(), xw.ravel(), [0.0] * 7])
    assert 16000 < x.size < 18000
    return x


@functools.lru_cache(maxsize=None)
def exp_near_points():
    """the eight doubles on either side of 708, -708, the thresholds of psd_exp_slow and
    log(DBL_MIN), the first argument with a subnormal result"""
    log_dbl_min = nearest_double(-1022 * ln2())
    x = np.concatenate([around(v, 8) for v in (708.0, -708.0, EXP_OVERFLOW, EXP_UNDERFLOW,
                                               log_dbl_min)])
    a = np.abs(x)
    assert np.sum(a <= 708.0) == 18 and np.sum(a > 708.0) == 17 * 5 - 18
    assert np.sum(x > EXP_OVERFLOW) == 8 and np.sum(x < EXP_UNDERFLOW) == 8
    return x


def exp_specials():
    return np.concatenate([[5e-324, -5e-324, 1e-300, -1e-300, 0.0, -0.0, np.inf, -np.inf],
                           from_bits([NAN_PAYLOAD, NAN_NEG_PAYLOAD])])


def exp_points():
    return np.concatenate([exp_rounding_points(), exp_near_points(), exp_specials()])


def is_exp_common(x):
    """|x| <= 708, as psd_exp tests it, on the bits: NaN and everything larger are rare"""
    return (bits(x) & np.uint64(0x7fffffffffffffff)) <= bits([708.0])[0]


# ---- the expected records of the branch-free forms, from the bits ---------------------------------

def rare_exp_nb(x):
    return (~is_exp_common(x)).astype(np.int32)


def _negative(x):
    """x < 0.0: the sign bit, but neither -0 nor a NaN"""
    u = bits(x)
    mag = u & np.uint64(0x7fffffffffffffff)
    return (u >> np.uint64(63) == 1) & (mag != 0) & (mag <= np.uint64(0x7ff0000000000000))


def rare_log_nb(x):
    return (~is_log_common(x) & ~_negative(x)).astype(np.int32)


def rare_log_wild_nb(x):
    u = bits(x)
    return ((u > 0) & (u < np.uint64(0x0010000000000000))).astype(np.int32)


# ---- wave layouts -------------------------------------------------------------------------------

def padded(n):
    """the smallest 64 q + 37 with q odd that is at least n: the last wave and the last workgroup of
    256 are partial"""
    q = max(0, -(-(n - 37) // 64))
    q += 1 - q % 2
    return 64 * q + 37


def layout(common, rare_values, n, points=(), reserve=None):
    """An array of at least n arguments whose 64-element groups -- the waves of a launch with one
    thread per element -- show for every rare value in turn: no rare element, only element 0 rare,
    only element 63 rare, all rare, alternating.  Then `points` follow, then common values up to a
    length of 64 q + 37 with q odd.  reserve: the rare values to leave groups for (default: as many
    as there are).  Returns the array and the mask of the rare placements."""
    common = np.asarray(common, dtype=np.float64)
    rare_values = np.asarray(rare_values, dtype=np.float64)
    points = np.asarray(points, dtype=np.float64)
    at = 320 * (len(rare_values) if reserve is None else reserve)
    assert at >= 320 * len(rare_values)
    total = padded(max(n, at + len(points)))
    x = np.resize(common, total)
    mask = np.zeros(total, dtype=bool)
    for r in range(len(rare_values)):
        g = 320 * r
        mask[g + 64] = True             # group 1: element 0
        mask[g + 128 + 63] = True       # group 2: element 63
        mask[g + 192:g + 256] = True    # group 3: all
        mask[g + 256:g + 320:2] = True  # group 4: alternating
        x[g:g + 320][mask[g:g + 320]] = rare_values[r]
    x[at:at + len(points)] = points
    assert total % 256 != 0 and total % 64 != 0 and (total - 37) // 64 % 2 == 1
    return x, mask


def fused_layouts(operands, n=0):
    """for the forms of two and three arguments; operands: (common, rare_values, points) of each.
    The rare elements in the first operand only, in the second only, (in the third only,) and in all:
    -> a list of (arrays, masks), one array and one mask per operand.  Each operand takes its common
    values and its points in a rotation of its own, so that the arguments of an element differ."""
    total = max(len(layout(c, r, n, p)[0]) for c, r, p in operands)
    wheres = [(a,) for a in range(len(operands))] + [tuple(range(len(operands)))]
    out = []
    for where in wheres:
        arrays, masks = [], []
        for a, (c, r, p) in enumerate(operands):
            x, m = layout(np.roll(c, 17 * a), r if a in where else [], total, np.roll(p, 5 * a),
                          reserve=len(r))
            assert len(x) == total
            arrays.append(x)
            masks.append(m)
        out.append((arrays, masks))
    return out


# ---- division -----------------------------------------------------------------------------------

def overflow_pairs():
    """operand pairs whose quotient overflows, in the four sign combinations: a / b is +-inf"""
    a = np.array([1e308, DBL_MAX, 1.0, 2.0 ** 1000, 4.0])
    b = np.array([1e-10, 0.5, 5e-324, 2.0 ** -30, SUB_MAX])
    a = np.concatenate([a, -a, a, -a])
    b = np.concatenate([b, b, -b, -b])
    with np.errstate(over="ignore"):
        assert np.all(np.isinf(a / b))
    return a, b


def subnormal_quotient_pairs(n, seed=19):
    """numerators in 2^-1030 .. 2^-1011 over divisors in 1 .. 2^40, both signs: quotients that are
    subnormal or just above, where the residual of psd_div_repair is no longer exact"""
    rng = np.random.default_rng(seed)
    a = np.ldexp(rng.uniform(0.5, 1.0, n), rng.integers(-1029, -1010, n)) * rng.choice([-1.0, 1.0], n)
    b = np.ldexp(rng.uniform(0.5, 1.0, n), rng.integers(1, 41, n)) * rng.choice([-1.0, 1.0], n)
    assert np.mean(np.abs(a / b) < DBL_MIN) > 0.5
    return a, b
