"""Stranded single-end reads: the strand cross-correlation of the reads' 5'
ends, the fragment length chosen from it, and the extension of reads to that length -- the step in
front of every *_reads entry point.  The integers come from the device
(peakseg_hip_reads_strand_xcorr, peakseg_hip_reads_extend; the definitions are in
include/peaksegdisk_hip.h); the correlation and the choice are formed here from them in Python
integers, so that the floats decide nothing."""
import ctypes
import math

import numpy as np

from . import _native

COLUMNS = ("pairs", "sum_plus", "sq_plus", "sum_minus", "sq_minus", "cross")


class FragmentLength:
    """What estimate_fragment_length returns: fragment_length = shift + 1, the shift of the largest
    correlation in [min_shift, max_shift], that correlation, and the pooled curve (the data frame
    of strand_cross_correlation for all contigs together)."""

    def __init__(self, shift, correlation, curve):
        self.shift = int(shift)
        self.fragment_length = self.shift + 1
        self.correlation = float(correlation)
        self.curve = curve

    def __repr__(self):
        return "FragmentLength(fragment_length=%d, shift=%d, correlation=%r)" % (
            self.fragment_length, self.shift, self.correlation)


def _status_error(who, status, lib):
    err = RuntimeError("%s: status %d: %s" % (who, status, lib.peakseg_hip_last_error().decode()))
    err.status = status
    return err


def moments(row):
    """(num, vx, vy) of one row of six Python integers"""
    pairs, sum_plus, sq_plus, sum_minus, sq_minus, cross = (int(v) for v in row)
    return (pairs * cross - sum_plus * sum_minus, pairs * sq_plus - sum_plus * sum_plus,
            pairs * sq_minus - sum_minus * sum_minus)


def correlation(row):
    """Pearson's r of one row, NaN where a variance is not positive"""
    num, vx, vy = moments(row)
    if vx <= 0 or vy <= 0:
        return float("nan")
    return float(num) / (math.sqrt(float(vx)) * math.sqrt(float(vy)))


def _larger(a, b):
    """is the correlation of moments a larger than that of b (both finite)?  Exact: the sign of num
    first, then num_a^2 vx_b vy_b against num_b^2 vx_a vy_a."""
    sa, sb = (a[0] > 0) - (a[0] < 0), (b[0] > 0) - (b[0] < 0)
    if sa != sb:
        return sa > sb
    if sa == 0:
        return False
    left, right = a[0] * a[0] * b[1] * b[2], b[0] * b[0] * a[1] * a[2]
    return left > right if sa > 0 else left < right


def choose_shift(rows, min_shift=0):
    """The shift of the largest finite correlation among rows[min_shift:], the smallest such shift
    among equals; ValueError when no shift has one."""
    best = None
    for s in range(int(min_shift), len(rows)):
        m = moments(rows[s])
        if m[1] <= 0 or m[2] <= 0:
            continue
        if best is None or _larger(m, best[1]):
            best = (s, m)
    if best is None:
        raise ValueError("no shift of %d .. %d has a finite correlation" % (min_shift, len(rows) - 1))
    return best[0]


def pooled(tables):
    """the column-wise sum of the contigs' tables in Python integers: rows of six"""
    return [[sum(int(t[s][j]) for t in tables) for j in range(len(COLUMNS))]
            for s in range(len(tables[0]))]


def curve_frame(rows):
    """shift, the six integer columns (int64; Python integers where a pooled sum passes 2^63) and
    the correlation"""
    import pandas as pd
    frame = {"shift": np.arange(len(rows), dtype=np.int64)}
    for j, name in enumerate(COLUMNS):
        col = [int(r[j]) for r in rows]
        fits = all(-2 ** 63 <= v < 2 ** 63 for v in col)
        frame[name] = np.array(col, dtype=np.int64 if fits else object)
    frame["correlation"] = np.array([correlation(r) for r in rows], dtype=np.float64)
    return pd.DataFrame(frame)


def _strand_pointers(strands, args, keep, device, who):
    """the ctypes array of the strands' addresses, checked against the reads of reads_arguments"""
    from .grid import _dense_pointer
    nc = args[0]
    if strands is None or len(strands) != nc:
        raise ValueError("%s: strands: one int8 array per contig" % who)
    side_of = {0: "host", 1: "device"}[args[5]]
    ptrs = []
    for k, v in enumerate(strands):
        ptr, n, side, ref = _dense_pointer(k, v, device, who + ": contig %d strand", dtype="int8")
        if n != args[1][k]:
            raise ValueError("%s: contig %d has %d chromStart and %d strand" % (who, k, args[1][k], n))
        if n and side != side_of:
            raise ValueError("%s: contig %d strand is in %s memory but the reads are in %s memory; "
                             "one call takes one kind" % (who, k, side, side_of))
        keep.append(ref)
        ptrs.append(ptr if n else 0)
    return (ctypes.c_void_p * nc)(*ptrs)


def xcorr_tables(reads, strands, max_shift=400, extents=None, device=0, lib=None,
                 who="strand_cross_correlation"):
    """The tables of peakseg_hip_reads_strand_xcorr: per contig an int64 array of
    (max_shift + 1, 6), and the extents as a list of (lo, hi).  reads and extents as
    ProblemSet.from_reads takes them, strands one int8 array or tensor per contig."""
    from .grid import reads_arguments
    lib = lib or _native.lib
    max_shift = int(max_shift)
    args, keep, ext = reads_arguments(reads, extents, "each", device, who)
    strand_ptrs = _strand_pointers(strands, args, keep, device, who)
    nc = args[0]
    table = np.zeros((nc, max(max_shift, 0) + 1, len(COLUMNS)), dtype=np.int64)
    st = lib.peakseg_hip_reads_strand_xcorr(device, nc, args[1], args[2], args[3], args[4], strand_ptrs,
                                            args[5], args[6], args[7], max_shift, table.ctypes.data)
    del keep
    if st != 0:
        raise _status_error("peakseg_hip_reads_strand_xcorr", st, lib)
    return [table[c] for c in range(nc)], ext


def estimate(reads, strands, max_shift=400, min_shift=0, extents=None, device=0, lib=None,
             who="estimate_fragment_length"):
    """FragmentLength of the pooled table of all contigs"""
    min_shift = int(min_shift)
    if not 0 <= min_shift <= int(max_shift):
        raise ValueError("%s: min_shift is %d, outside 0 .. max_shift = %d" % (who, min_shift, max_shift))
    tables, _ = xcorr_tables(reads, strands, max_shift, extents, device, lib, who)
    rows = pooled(tables)
    shift = choose_shift(rows, min_shift)
    return FragmentLength(shift, correlation(rows[shift]), curve_frame(rows))


def _lengths(fragment_length, nc, who):
    if isinstance(fragment_length, (int, np.integer)) and not isinstance(fragment_length, bool):
        fragment_length = [fragment_length] * nc
    lengths = list(fragment_length) if isinstance(fragment_length, (list, tuple, np.ndarray)) else []
    if len(lengths) != nc or not all(isinstance(d, (int, np.integer)) and not isinstance(d, bool)
                                     for d in lengths):
        raise ValueError("%s: fragment_length: an integer, or one per contig" % who)
    if any(not -2 ** 31 <= int(d) < 2 ** 31 for d in lengths):
        raise ValueError("%s: fragment_length must fit 32-bit integers" % who)
    return [int(d) for d in lengths]


def extend(reads, strands, fragment_length, device=0, lib=None, who="extend_reads"):
    """The reads extended from their 5' ends to fragment_length (peakseg_hip_reads_extend): a list,
    one entry per contig, of (chromStart, chromEnd) or (chromStart, chromEnd, count) in the kind of
    memory they came in -- numpy arrays for numpy arrays, tensors on cuda:`device`, allocated by
    torch and written by the kernel, for such tensors.  count passes through as it is."""
    from .grid import reads_arguments
    lib = lib or _native.lib
    placeholder = [(0, 1)] * len(reads)          # (the extension knows no extent)
    args, keep, _ = reads_arguments(reads, placeholder, "each", device, who)
    strand_ptrs = _strand_pointers(strands, args, keep, device, who)
    nc = args[0]
    lengths = _lengths(fragment_length, nc, who)
    out, out_ptrs = [], ([], [])
    for entry in reads:
        pair = []
        for j in range(2):
            v = entry[j]
            if isinstance(v, np.ndarray):
                new = np.empty(v.shape[0], dtype=np.int32)
                ptr = new.ctypes.data
            else:
                import torch
                new = torch.empty_like(v)
                ptr = new.data_ptr()
            pair.append(new)
            out_ptrs[j].append(ptr if v.shape[0] else 0)
        out.append(tuple(pair) + tuple(entry[2:3] if len(entry) > 2 and entry[2] is not None else ()))
    st = lib.peakseg_hip_reads_extend(device, nc, args[1], args[2], args[3], strand_ptrs, args[5],
                                      (ctypes.c_int * nc)(*lengths), (ctypes.c_void_p * nc)(*out_ptrs[0]),
                                      (ctypes.c_void_p * nc)(*out_ptrs[1]))
    del keep
    if st != 0:
        raise _status_error("peakseg_hip_reads_extend", st, lib)
    return out


def extended_for(reads, strands, fragment_length, extents, device, lib, who, max_shift=400,
                 min_shift=0):
    """What the *_reads entry points do with their strands= and fragment_length= keywords: (the
    reads to pile up, the extents).  Both None: the reads as they are.  Exactly one given:
    ValueError.  fragment_length "auto": the pooled estimate.  Default extents stay those of the
    reads as given -- (min chromStart, max chromEnd) per contig -- and the extension is clipped to
    them by the pile-up."""
    if strands is None and fragment_length is None:
        return reads, extents
    if strands is None or fragment_length is None:
        raise ValueError("%s: strands and fragment_length go together: %s is given without %s"
                         % ((who, "fragment_length", "strands") if strands is None
                            else (who, "strands", "fragment_length")))
    from .grid import reads_arguments
    _, keep, ext = reads_arguments(reads, extents, "each", device, who)
    del keep
    if isinstance(fragment_length, str):
        if fragment_length != "auto":
            raise ValueError('%s: fragment_length is %r, not an integer or "auto"' % (who, fragment_length))
        fragment_length = estimate(reads, strands, max_shift, min_shift, ext, device, lib,
                                   who).fragment_length
    return extend(reads, strands, fragment_length, device, lib, who), ext
