"""The definitions of the strand cross-correlation (include/peaksegdisk_hip.h)
restated in numpy and Python integers: what the device's tables, the estimate and the extension are
compared with.  Nothing here calls the library under test."""
import math
from fractions import Fraction

import numpy as np

COLUMNS = ("pairs", "sum_plus", "sq_plus", "sum_minus", "sq_minus", "cross")
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def tags(start, end, count, strand, lo, hi):
    """(p, m): int64 arrays of hi - lo entries.  The 5' base of a plus read is chromStart, of a
    minus read chromEnd - 1; one outside [lo, hi) is no tag."""
    start, end = np.asarray(start, np.int64), np.asarray(end, np.int64)
    strand = np.asarray(strand, np.int64)
    k = np.ones(len(start), np.int64) if count is None else np.asarray(count, np.int64)
    assert ((strand == 1) | (strand == -1)).all() and (start < end).all() and (k >= 0).all()
    assert int(k.sum()) < 2 ** 31
    at = np.where(strand > 0, start, end - 1)
    inside = (at >= lo) & (at < hi)
    p, m = np.zeros(hi - lo, np.int64), np.zeros(hi - lo, np.int64)
    np.add.at(p, (at - lo)[inside & (strand > 0)], k[inside & (strand > 0)])
    np.add.at(m, (at - lo)[inside & (strand < 0)], k[inside & (strand < 0)])
    return p, m


def table_of_tags(p, m, max_shift):
    """rows s = 0 .. max_shift of six Python integers"""
    B = len(p)
    cp = np.concatenate([[0], np.cumsum(p)])
    cp2 = np.concatenate([[0], np.cumsum(p * p)])
    cm = np.concatenate([[0], np.cumsum(m)])
    cm2 = np.concatenate([[0], np.cumsum(m * m)])
    where = np.flatnonzero(p)
    rows = []
    for s in range(max_shift + 1):
        pairs = max(B - s, 0)
        j = where + s
        ok = j < B
        # (every product is below 2^62 and so is their sum: sum p x sum m < 2^62)
        cross = int((p[where[ok]] * m[j[ok]]).sum()) if ok.any() else 0
        rows.append([pairs, int(cp[pairs]), int(cp2[pairs]), int(cm[B] - cm[B - pairs]),
                     int(cm2[B] - cm2[B - pairs]), cross])
    return rows


def table(start, end, count, strand, lo, hi, max_shift):
    p, m = tags(start, end, count, strand, lo, hi)
    return table_of_tags(p, m, max_shift)


def table_by_loops(p, m, max_shift):
    """the table from the definitions word for word, for small inputs: pins table_of_tags"""
    B = len(p)
    p, m = [int(v) for v in p], [int(v) for v in m]
    rows = []
    for s in range(max_shift + 1):
        left, right = range(0, max(B - s, 0)), range(min(s, B), B)
        rows.append([max(B - s, 0), sum(p[i] for i in left), sum(p[i] ** 2 for i in left),
                     sum(m[i] for i in right), sum(m[i] ** 2 for i in right),
                     sum(p[i] * m[i + s] for i in left)])
    return rows


def pooled(tables):
    return [[sum(t[s][j] for t in tables) for j in range(6)] for s in range(len(tables[0]))]


def moments(row):
    pairs, sp, sqp, sm, sqm, cross = (int(v) for v in row)
    return pairs * cross - sp * sm, pairs * sqp - sp * sp, pairs * sqm - sm * sm


def correlation(row):
    num, vx, vy = moments(row)
    if vx <= 0 or vy <= 0:
        return float("nan")
    return float(num) / (math.sqrt(float(vx)) * math.sqrt(float(vy)))


def estimate(rows, min_shift=0):
    """(shift, fragment_length, r): the largest r among the finite ones of rows[min_shift:], the
    smallest shift among equals.  Exact: r is ordered as sign(num) num^2 / (vx vy), a fraction of
    Python integers."""
    best = None
    for s in range(min_shift, len(rows)):
        num, vx, vy = moments(rows[s])
        if vx <= 0 or vy <= 0:
            continue
        key = Fraction(num * abs(num), vx * vy)
        if best is None or key > best[0]:
            best = (key, s)
    if best is None:
        raise ValueError("no finite correlation")
    return best[1], best[1] + 1, correlation(rows[best[1]])


def extend(start, end, strand, d):
    """plus: [start, start + d), minus: [end - d, end), in Python-sized integers, clamped to int32"""
    start, end = np.asarray(start, np.int64), np.asarray(end, np.int64)
    plus = np.asarray(strand) > 0
    new_start = np.where(plus, start, np.maximum(end - int(d), I32_MIN))
    new_end = np.where(plus, np.minimum(start + int(d), I32_MAX), end)
    return new_start.astype(np.int32), new_end.astype(np.int32)


def hash_strands(n, seed=1):
    """+1 iff splitmix64(seed, index) is even"""
    from peaksegdisk_amd.synthetic import splitmix64
    even = (splitmix64(seed, np.arange(n, dtype=np.uint64)) & np.uint64(1)) == 0
    return np.where(even, 1, -1).astype(np.int8)
