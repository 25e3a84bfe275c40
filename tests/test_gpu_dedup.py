"""Duplicate removal of aligned reads on the device: the marking by a stable
radix sort, the compaction, and the max_duplicates= keyword of the *_reads entry points.

The scenario functions are shared with the emulator rehearsal (tests/test_dedup_emu.py), which runs
them without a GPU on host arrays; the tests marked gpu run them on the MI355X with the reads once as
numpy arrays and once as cuda tensors (in a child process that imports torch first, as
tests/test_gpu_strand_xcorr.py does).

Expected values never come from the library under test: out_count, summary and the compacted reads
are those of tests/dedup_ref.py (a dict of running sums per key, walked in input order; pinned in
tests/test_dedup_cpu.py), pile-ups those of test_gpu_reads.numpy_pileup, extended reads and
cross-correlation tables those of tests/xcorr_ref.py.  Everything is integer: every comparison is for
equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dedup_ref as ref
import test_gpu_dense as gd
import test_gpu_reads as gr
import test_gpu_strand_xcorr as gx
import xcorr_ref
from test_gpu_strand_xcorr import as_cuda, as_numpy  # noqa: F401

GPU = pytest.mark.gpu
SENTINEL = -7
BY = {"fragment": 0, "five_prime": 1}
KEEPS = (1, 2, 3, 2 ** 31 - 1)
MODES = ("fragment", "five_prime")


@pytest.fixture(scope="module")
def psd():
    import __graft_entry__ as entry
    entry.build_hip()
    entry.build_oracle()
    import peaksegdisk_amd
    from peaksegdisk_amd import _native
    assert _native.lib.peakseg_hip_device_count() >= 1, "no HIP device: GPU tests need an MI355X"
    return peaksegdisk_amd


_lib = gd._lib


def host(v):
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v)


def sizes():
    """(R, P): rows of a workgroup of a sort pass, workgroups of a trip of the table scan"""
    return _lib().peakseg_hip_dedup_block_rows(), _lib().peakseg_hip_dedup_scan_span()


def all_sizes():
    R, P = sizes()
    return (0, 1, 2, 63, 64, 65, 255, 256, 257, R - 1, R, R + 1, 2 * R + 5, R * P + R + 3)


# ---- helpers ---------------------------------------------------------------------------------

def dedup_probe(contigs, strands, keep, by, wrap, lib=None):
    """-> (status, [out_count int32 numpy per contig], summary int64 (C, 4)), marshalled here, not by
    the package.  contigs: wrapped (chromStart, chromEnd[, count]); strands: wrapped int8 or None."""
    lib = lib or _lib()
    nc = len(contigs)
    args = gr._read_arguments(contigs, [(0, 1)] * nc, "each")
    out = [wrap(np.full(int(e[0].shape[0]), SENTINEL, np.int32)) for e in contigs]
    summary = np.full((nc, 4), SENTINEL, np.int64)
    st = lib.peakseg_hip_reads_dedup(0, args[0], args[1], args[2], args[3], args[4],
                                     None if strands is None else gx._pointers(strands), args[5],
                                     BY.get(by, by), keep, gx._pointers(out), summary.ctypes.data)
    got = [host(o) for o in out]
    if st != 0:   # a refused call has written nothing
        assert all((g == SENTINEL).all() for g in got) and (summary == SENTINEL).all()
        return st, None, None
    return st, got, summary


def compact_probe(contigs, strands, keep_count, wrap):
    """-> (status, [(chromStart, chromEnd, count, strand or None) numpy per contig, cut to the rows
    written], rows int64); what lies behind the rows written must be untouched"""
    nc = len(contigs)
    args = gr._read_arguments(contigs, [(0, 1)] * nc, "each")
    n = [int(e[0].shape[0]) for e in contigs]
    outs = [[wrap(np.full(m, SENTINEL, np.int32)) for m in n] for _ in range(3)]
    out_strand = None if strands is None else [wrap(np.full(m, SENTINEL, np.int8)) for m in n]
    rows = np.full(nc, SENTINEL, np.int64)
    st = _lib().peakseg_hip_reads_compact(
        0, args[0], args[1], args[2], args[3], None if strands is None else gx._pointers(strands), args[5],
        gx._pointers(keep_count), gx._pointers(outs[0]), gx._pointers(outs[1]), gx._pointers(outs[2]),
        None if strands is None else gx._pointers(out_strand), rows.ctypes.data)
    if st != 0:
        assert (rows == SENTINEL).all() and all((host(o) == SENTINEL).all() for col in outs for o in col)
        return st, None, None
    result = []
    for c in range(nc):
        cols = [host(outs[j][c]) for j in range(3)] + [None if strands is None else host(out_strand[c])]
        assert all(col is None or (col[int(rows[c]):] == SENTINEL).all() for col in cols)
        result.append(tuple(None if col is None else col[:int(rows[c])] for col in cols))
    return st, result, rows


def wrap_entry(entry, wrap):
    """(chromStart, chromEnd, count or None, strand or None) numpy -> (the wrapped reads, the strand)"""
    reads = tuple(wrap(v) for v in entry[:3] if v is not None)
    return reads, None if entry[3] is None else wrap(entry[3])


def check_marks(contigs_np, keeps, by, wrap, what, lib=None):
    """one call per keep against the reference; contigs_np: (chromStart, chromEnd, count or None,
    strand or None) per contig.  Returns the out_count of the last keep."""
    wrapped = [wrap_entry(e, wrap) for e in contigs_np]
    reads = [w[0] for w in wrapped]
    strands = None if contigs_np[0][3] is None else [w[1] for w in wrapped]
    before = [ref.before_sums(e[0], e[1], e[2], e[3], by) for e in contigs_np]
    got = None
    for keep in keeps:
        st, got, summary = dedup_probe(reads, strands, keep, by, wrap, lib)
        assert st == 0, (what, keep, (lib or _lib()).peakseg_hip_last_error())
        for c, e in enumerate(contigs_np):
            out, want = ref.marks(before[c], e[2], keep)
            assert np.array_equal(got[c], out), (what, by, keep, c)
            assert summary[c].tolist() == want, (what, by, keep, c, summary[c].tolist(), want)
    return got


def passes():
    return _lib().peakseg_hip_reads_last_dedup_passes()


def pool_reads(rng, n, span=None):
    """n reads drawn from a pool of 1.2 n candidates -- about a third of the rows repeat an earlier
    one --, both strands, some coordinates negative; counts 0-5"""
    pool = max(1, int(1.2 * n))
    start = rng.integers(-500, 500 + (span or 4 * max(n, 1)), pool)
    length = rng.integers(1, 40, pool)
    strand = np.where(rng.integers(0, 2, pool) > 0, 1, -1)
    pick = rng.integers(0, pool, n)
    return (start[pick].astype(np.int32), (start[pick] + length[pick]).astype(np.int32),
            rng.integers(0, 6, n).astype(np.int32), strand[pick].astype(np.int8))


# ---- 1: every size, keep, mode, with and without counts -------------------------------------------

def scenario_sizes(wrap, n_values=None, keeps=KEEPS):
    rng = np.random.default_rng(20250601)
    for n in n_values or all_sizes():
        s, e, k, d = pool_reads(rng, n)
        if n > 300:
            assert 0.2 < 1 - len(set(zip(s.tolist(), e.tolist(), d.tolist()))) / n < 0.45
            assert (k == 0).any()
        for by in MODES:
            for count in (None, k):
                check_marks([(s, e, count, d)], keeps, by, wrap, ("size", n, count is None))
        if n > 300:
            assert passes() >= 2


# ---- 2: order and stability -----------------------------------------------------------------------

def scenario_order(wrap):
    """the same multiset sorted, reversed and shuffled: the survivors are the earliest rows of every
    key in input order each time, which only a stable sort gives"""
    R, _ = sizes()
    rng = np.random.default_rng(2)
    n = 2 * R + 5
    few = pool_reads(rng, 300)                    # few keys: runs of about seven equal keys
    pick = rng.integers(0, 300, n)
    s, e, d = few[0][pick], few[1][pick], few[3][pick]
    k = rng.integers(0, 6, n).astype(np.int32)
    sorted_order = np.lexsort((e, s, d))
    for name, order in (("sorted", sorted_order), ("reversed", sorted_order[::-1]),
                        ("shuffled", rng.permutation(n))):
        entry = tuple(np.ascontiguousarray(a[order]) for a in (s, e, k, d))
        for by in MODES:
            got = check_marks([(entry[0], entry[1], None, entry[3])], (1,), by, wrap, name)[0]
            # without counts and at keep 1 the survivors are the first occurrences of the keys
            keys = [ref.key_of(by, a, b, c) for a, b, c in zip(*(v.tolist() for v in (entry[0], entry[1], entry[3])))]
            first = {}
            for i, key in enumerate(keys):
                first.setdefault(key, i)
            want = np.zeros(n, np.int32)
            want[list(first.values())] = 1
            assert np.array_equal(got, want), (name, by)
            check_marks([entry], (2, 3), by, wrap, name)


# ---- 3: runs and carries ----------------------------------------------------------------------------

def scenario_runs(wrap):
    R, _ = sizes()
    rng = np.random.default_rng(3)
    n = 2 * R + 5
    ones = np.ones(n, np.int8)
    # one key: one run across every workgroup, and no sort pass
    s, e = np.full(n, -40, np.int32), np.full(n, 17, np.int32)
    k = rng.integers(0, 6, n).astype(np.int32)
    for count in (None, k):
        got = check_marks([(s, e, count, ones)], (1, 5, n - 1, n, 2 ** 31 - 1), "fragment", wrap, "one key")[0]
        assert passes() == 0
        assert np.array_equal(got, np.ones(n, np.int32) if count is None else k)
    check_marks([(s, e, k, None)], (3,), "fragment", wrap, "one key, no strands")
    # all rows distinct
    s = (rng.permutation(n) * 3 - 1000).astype(np.int32)
    got = check_marks([(s, s + 5, k, ones)], (1, 2 ** 31 - 1), "five_prime", wrap, "distinct")[0]
    assert np.array_equal(got, k)
    # 5000 rows on one key among others
    s, e, k, d = pool_reads(rng, 3000)
    s = np.concatenate([s, np.full(5000, 123, np.int32)])
    e = np.concatenate([e, np.full(5000, 160, np.int32)])
    k = np.concatenate([k, rng.integers(0, 6, 5000).astype(np.int32)])
    d = np.concatenate([d, np.ones(5000, np.int8)])
    order = rng.permutation(8000)
    for by in MODES:
        check_marks([(s[order], e[order], k[order], d[order])], (1, 3, 4999), by, wrap, "5000 on one key")
        check_marks([(s[order], e[order], None, d[order])], (4999, 5000), by, wrap, "5000 on one key")
    # Sorted input stays where it is, so rows are positions: a run that reaches keep = 2 exactly at
    # the edge at 256, one that ends at a sort workgroup's last row R - 1 (and reaches keep = 300
    # there), one that begins at R, single rows everywhere else
    s = np.arange(n, dtype=np.int64) * 2
    s[254:294] = s[254]
    s[R - 300:R] = s[R - 300]
    s[R:R + 601] = s[R]
    assert (np.diff(s) >= 0).all()
    s = s.astype(np.int32)
    k = rng.integers(1, 6, n).astype(np.int32)
    k[R - 300] = 7                 # a row with more units than keep, at the head of a run
    for by in MODES:
        got = check_marks([(s, s + 30, None, ones)], (1, 2, 3, 300, 301), by, wrap, "edges")[0]
        assert got[R - 300:R].all() and got[R:R + 301].all() and not got[R + 301:R + 601].any()
        check_marks([(s, s + 30, k, ones)], (1, 3, 6, 7, 300), by, wrap, "edges, counted")
    # counts that sum to 2^31 - 1 in one contig
    s = np.array([5, 900, 5, 5], np.int32)
    k = np.array([2 ** 30, 0, 2 ** 30 - 2, 1], np.int32)
    assert int(k.sum()) == 2 ** 31 - 1
    got = check_marks([(s, s + 9, k, ones[:4])], (2 ** 30 + 5, 2 ** 31 - 1), "fragment", wrap, "2^31 - 1")[0]
    assert np.array_equal(got, k)
    got = check_marks([(s, s + 9, k, ones[:4])], (2 ** 30 + 5,), "five_prime", wrap, "2^31 - 1")[0]
    assert got.tolist() == [2 ** 30, 0, 5, 0]


# ---- 4: every digit -------------------------------------------------------------------------------

DIGIT_EDGES = (0, 7, 8, 15, 16, 23, 24, 30, 31)    # the bits the emulator rehearsal takes


def scenario_digits(wrap, bits=range(32)):
    """two keys that differ in one bit alone, each twice: at keep 1 the first of each survives"""
    cases = []
    for bit in bits:
        flip = -2 ** 31 if bit == 31 else 1 << bit
        a, b = 5, 5 ^ flip                      # chromStart; bit 31: a negative chromStart
        cases.append(("start", bit, [a, b, b, a], [2 ** 31 - 1] * 4, [1] * 4))
        a, b = 6, 6 ^ flip                      # chromEnd, behind the smallest chromStart
        cases.append(("end", bit, [-2 ** 31] * 4, [a, b, b, a], [1] * 4))
        cases.append(("end of minus reads", bit, [-2 ** 31] * 4, [a, b, b, a], [-1] * 4))
    cases.append(("strand", 0, [-3] * 4, [8] * 4, [1, -1, -1, 1]))
    for name, bit, s, e, d in cases:
        s, e, d = np.array(s, np.int32), np.array(e, np.int32), np.array(d, np.int8)
        got = check_marks([(s, e, None, d)], (1,), "fragment", wrap, (name, bit))[0]
        assert got.tolist() == [1, 1, 0, 0] and passes() == 1, (name, bit, passes())
        # two plus reads with equal starts and different ends, two minus reads with different starts
        # and equal ends: no duplicates by fragment, one of each pair by 5' end
        s2 = np.concatenate([s, [100, 100, 100, 90]]).astype(np.int32)
        e2 = np.concatenate([e, [130, 131, 131, 131]]).astype(np.int32)
        d2 = np.concatenate([d, [1, 1, -1, -1]]).astype(np.int8)
        got = check_marks([(s2, e2, None, d2)], (1,), "fragment", wrap, (name, bit))[0]
        assert got.tolist() == [1, 1, 0, 0, 1, 1, 1, 1]
        got = check_marks([(s2, e2, None, d2)], (1,), "five_prime", wrap, (name, bit))[0]
        assert got[4:].tolist() == [1, 0, 1, 0]
        if name != "end":          # (the plus reads of "end" share their 5' base)
            assert got[:4].tolist() == [1, 1, 0, 0], (name, bit)


# ---- 5: contigs -------------------------------------------------------------------------------------

def scenario_contigs(wrap):
    rng = np.random.default_rng(5)
    entry = pool_reads(rng, 700)
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int8))
    single = tuple(a[:1].copy() for a in entry)
    contigs = [entry, empty, tuple(a.copy() for a in entry), single]
    for by in MODES:
        together = check_marks(contigs, (1, 2), by, wrap, "four contigs")
        alone = check_marks([entry], (2,), by, wrap, "alone")[0]
        # nothing is grouped across contigs: identical reads give identical marks
        assert np.array_equal(together[0], alone) and np.array_equal(together[2], alone)
        assert together[1].shape == (0,) and together[3].tolist() == [min(int(entry[2][0]), 2)]
    # 300 contigs of 3 rows: the contig index crosses a digit
    many = []
    for c in range(300):
        s = np.array([40, 40, 41 + c % 2], np.int32)[rng.permutation(3)]
        many.append((s, s + 20, rng.integers(0, 4, 3).astype(np.int32), np.ones(3, np.int8)))
    for by in MODES:
        check_marks(many, (1, 3), by, wrap, "300 contigs")
        check_marks([(m[0], m[1], None, None) for m in many], (1,), "fragment", wrap, "300 contigs")


# ---- 6: refusals ------------------------------------------------------------------------------------

def scenario_refusals(wrap):
    from peaksegdisk_amd import _native
    assert _native.ERROR_DEDUP_ARGUMENTS == 25 and _native.ERROR_STRAND_ARGUMENTS == 24

    def reads(start, end, count=None):
        entry = (wrap(np.array(start, np.int32)), wrap(np.array(end, np.int32)))
        return entry if count is None else entry + (wrap(np.array(count, np.int32)),)

    def strand(values):
        return wrap(np.array(values, np.int8))

    good, good_strand = reads([10, 30, 20], [40, 60, 50]), strand([1, -1, 1])

    def refused(status, contigs, strands, keep, by, *words):
        st, _, _ = dedup_probe(contigs, strands, keep, by, wrap)
        err = _lib().peakseg_hip_last_error().decode()
        assert st == status, (st, err)
        for w in words:
            assert w in err, err

    refused(18, [good, reads([5, 7, 9, 9], [6, 8, 9, 9])], [good_strand, strand([1, 1, 1, 1])], 1,
            "five_prime", "contig 1", "read 2")
    refused(18, [reads([5, 7, 9], [6, 8, 10], [1, 0, -1]), good], None, 1, "fragment", "contig 0",
            "read 2", "negative")
    refused(24, [good, reads([5, 7, 9], [6, 8, 10])], [good_strand, strand([1, -1, 0])], 1, "fragment",
            "contig 1", "read 2", "strand")
    refused(24, [good, good], [good_strand, None], 1, "fragment", "contig 1", "NULL")
    n = 1000                      # the first bad read of a contig decides, whatever is wrong with it
    s = np.arange(n, dtype=np.int32) + 500
    e = s + 5
    e[900] = s[900]
    d = np.ones(n, np.int8)
    d[777] = 3
    refused(24, [good, (wrap(s), wrap(e))], [good_strand, wrap(d)], 2, "five_prime", "contig 1", "read 777")
    refused(18, [good, reads([5, 6, 300], [50, 60, 310], [2 ** 30, 2 ** 30 - 1, 1])],
            [good_strand, good_strand], 1, "five_prime", "contig 1", "2^31")
    refused(25, [good], [good_strand], 0, "five_prime", "keep")
    refused(25, [good], [good_strand], -2 ** 31, "fragment", "keep")
    refused(25, [good], [good_strand], 1, 2, "by")
    refused(25, [good], None, 1, "five_prime", "five_prime", "strands")
    # an output that overlaps an input: the reads' own array as out_count
    args = gr._read_arguments([good], [(0, 1)], "each")
    summary = np.full(4, SENTINEL, np.int64)
    st = _lib().peakseg_hip_reads_dedup(0, args[0], args[1], args[2], args[3], args[4], None, args[5], 0, 1,
                                        gx._pointers([good[1]]), summary.ctypes.data)
    assert st == 25 and "overlaps" in _lib().peakseg_hip_last_error().decode()
    assert host(good[1]).tolist() == [40, 60, 50] and (summary == SENTINEL).all()
    assert _lib().peakseg_hip_reads_dedup(0, 0, args[1], args[2], args[3], args[4], None, args[5], 0, 1,
                                          gx._pointers([good[1]]), summary.ctypes.data) == 9
    # whether the buffers fit is asked before anything is allocated
    old = os.environ.get("PEAKSEG_HIP_MAX_BYTES")
    os.environ["PEAKSEG_HIP_MAX_BYTES"] = "64"
    try:
        refused(14, [good], [good_strand], 1, "five_prime", "do not fit")
        st, _, _ = compact_probe([good], None, [wrap(np.array([1, 0, 1], np.int32))], wrap)
        assert st == 14
    finally:
        if old is None:
            del os.environ["PEAKSEG_HIP_MAX_BYTES"]
        else:
            os.environ["PEAKSEG_HIP_MAX_BYTES"] = old
    # the compaction
    st, _, _ = compact_probe([good], None, [good[0]], wrap)
    assert st == 0
    args = gr._read_arguments([good], [(0, 1)], "each")
    rows = np.full(1, SENTINEL, np.int64)
    keep_count = wrap(np.array([1, 0, 1], np.int32))
    outs = [wrap(np.full(3, SENTINEL, np.int32)) for _ in range(2)]
    st = _lib().peakseg_hip_reads_compact(0, args[0], args[1], args[2], args[3], None, args[5],
                                          gx._pointers([keep_count]), gx._pointers([outs[0]]),
                                          gx._pointers([outs[1]]), gx._pointers([keep_count]), None,
                                          rows.ctypes.data)
    assert st == 25 and "overlaps" in _lib().peakseg_hip_last_error().decode()
    assert (rows == SENTINEL).all() and host(keep_count).tolist() == [1, 0, 1]
    assert all((host(o) == SENTINEL).all() for o in outs)


# ---- 7: addresses -----------------------------------------------------------------------------------

def scenario_offsets(device_array):
    """Device arrays: an int32 address that is no multiple of 4 is refused; strand arrays that begin
    at each of the four byte offsets of a word give the reference's marks.  device_array(numpy array)
    -> (an object with the device address, that address)."""
    rng = np.random.default_rng(7)
    s, e, k, d = pool_reads(rng, 1500)
    n = len(s) - 8
    out = np.full(n, SENTINEL, np.int32)
    held = [device_array(v) for v in (s, e, k, d, out)]
    base = [h[1] for h in held]
    for lead in range(4):
        want, want_summary = ref.dedup(s[:n], e[:n], k[:n], d[lead:lead + n], 2, "five_prime")
        summary = np.full(4, SENTINEL, np.int64)
        one = lambda p: (ctypes.c_void_p * 1)(p)   # noqa: E731
        call = lambda shift_by: _lib().peakseg_hip_reads_dedup(   # noqa: E731
            0, 1, (ctypes.c_longlong * 1)(n), one(base[0] + shift_by), one(base[1]), one(base[2]),
            one(base[3] + lead), 1, 1, 2, one(base[4]), summary.ctypes.data)
        assert call(0) == 0, _lib().peakseg_hip_last_error()
        got = held[4][0]
        got = host(got) if not isinstance(got, np.ndarray) else got[-got.ctypes.data % 16:][:4 * n].view(np.int32)
        assert np.array_equal(got[:n], want) and summary.tolist() == want_summary, lead
        summary[:] = SENTINEL
        assert call(2) == 18 and "multiple of 4" in _lib().peakseg_hip_last_error().decode()
        assert (summary == SENTINEL).all()
    del held


# ---- 8: compaction ------------------------------------------------------------------------------------

def scenario_compaction(psd, wrap, n_values=None):
    rng = np.random.default_rng(8)
    for n in n_values or all_sizes():
        s, e, k, d = pool_reads(rng, n)
        by, keep = MODES[n % 2], 1 + n % 3
        out, summary = ref.dedup(s, e, k, d, keep, by)
        want = ref.compacted(s, e, out, d)
        count = wrap(k)
        got = psd.remove_duplicates((wrap(s), wrap(e), count), wrap(d), keep=keep, by=by)
        assert isinstance(got, psd.DuplicateRemoval) and len(got.reads) == 3
        for a, b in zip(got.reads + (got.strands,), want):
            assert type(a) is type(count) and np.array_equal(host(a), b), (n, by, keep)
            assert host(a).dtype == b.dtype
            if hasattr(count, "device"):
                assert a.device == count.device
        assert got.summary.to_numpy().tolist() == [summary] and list(got.summary.columns) == list(ref.SUMMARY)
        assert all(str(t) == "int64" for t in got.summary.dtypes)
        # compact=False: the rows stay, only count changes, zeros included
        kept = psd.remove_duplicates((wrap(s), wrap(e), count), wrap(d), keep=keep, by=by, compact=False)
        assert kept.reads[0] is not None and np.array_equal(host(kept.reads[0]), s)
        assert np.array_equal(host(kept.reads[2]), out) and np.array_equal(host(kept.strands), d)
        assert type(kept.reads[2]) is type(count)
        assert kept.summary.equals(got.summary)
    # without strands and without counts; a list of contigs gives lists
    s, e, k, d = pool_reads(rng, 900)
    out, summary = ref.dedup(s, e, None, None, 1, "fragment")
    got = psd.remove_duplicates([(wrap(s), wrap(e)), (wrap(s[:10]), wrap(e[:10]))])
    assert got.strands is None and len(got.reads) == 2 and len(got.summary) == 2
    for a, b in zip(got.reads[0], ref.compacted(s, e, out)[:3]):
        assert np.array_equal(host(a), b)
    assert got.summary.to_numpy()[0].tolist() == summary
    # the compaction on its own, on a hand-made keep_count: what is not positive goes
    R, _ = sizes()
    n = R + 70
    s, e, k, d = pool_reads(rng, n)
    keep_count = rng.integers(-2, 4, n).astype(np.int32)
    keep_count[[0, 255, 256, n - 1]] = [3, 0, 2, 1]
    for strands in (None, d):
        st, got, rows = compact_probe([(wrap(s), wrap(e)), (wrap(s[:5]), wrap(e[:5]))],
                                      None if strands is None else [wrap(strands), wrap(strands[:5])],
                                      [wrap(keep_count), wrap(np.zeros(5, np.int32))], wrap)
        assert st == 0, _lib().peakseg_hip_last_error()
        want = ref.compacted(s, e, keep_count, strands)
        assert rows.tolist() == [len(want[0]), 0] and (want[2] > 0).all()
        for a, b in zip(got[0], want):
            assert (a is None and b is None) or np.array_equal(a, b)


# ---- 9: composition -----------------------------------------------------------------------------------

def scenario_composition(psd, wrap):
    rng = np.random.default_rng(9)
    s, e, k, d = pool_reads(rng, 1500, span=1000)
    s, e, k = s + 600, e + 600, np.maximum(k, 1)     # (the pile-up takes no negative extent)
    extent = (int(s.min()), int(e.max()))
    # coverage_from_reads(max_duplicates=) is the numpy pile-up of the reference's marks
    for count in (None, k):
        out, _ = ref.dedup(s, e, count, None, 1, "fragment")
        frame = psd.coverage_from_reads(wrap(s), wrap(e), None if count is None else wrap(count),
                                        max_duplicates=1)
        cov = np.repeat(frame["count"].to_numpy(), (frame["chromEnd"] - frame["chromStart"]).to_numpy())
        assert int(frame["chromStart"].iloc[0]) == extent[0] and int(frame["chromEnd"].iloc[-1]) == extent[1]
        assert np.array_equal(cov, gr.numpy_pileup(s, e, out, *extent))
    assert not np.array_equal(cov, gr.numpy_pileup(s, e, k, *extent))
    # solved: the keyword against the removal done by hand
    reads = (wrap(s), wrap(e))
    removed = psd.remove_duplicates(reads, keep=2)
    assert int(removed.summary["kept"].iloc[0]) < len(s)
    got = psd.PeakSegFPOP_reads(reads, [0.0, 10.0], max_duplicates=2)
    expect = psd.PeakSegFPOP_reads(removed.reads, [0.0, 10.0])
    plain = psd.PeakSegFPOP_reads(reads, [0.0, 10.0])
    for a, b in zip(got, expect):
        assert a.segments.equals(b.segments) and len(b.segments) >= 1
    assert len(expect[0].segments) > 3 and not got[0].segments.equals(plain[0].segments)
    pset = psd.ProblemSet.from_reads([reads], [(0, 10.0)], max_duplicates=2)
    try:
        assert pset.contig_starts == [extent[0]] and pset.contig_bases == [extent[1] - extent[0]]
    finally:
        pset.close()
    # with strands the removal is by 5' end and comes before the extension
    out, _ = ref.dedup(s, e, None, d, 1, "five_prime")
    ext = xcorr_ref.extend(s, e, d, 36)
    frame = psd.coverage_from_reads(wrap(s), wrap(e), strands=wrap(d), fragment_length=36, max_duplicates=1)
    cov = np.repeat(frame["count"].to_numpy(), (frame["chromEnd"] - frame["chromStart"]).to_numpy())
    assert np.array_equal(cov, gr.numpy_pileup(ext[0], ext[1], out, *extent))
    # (the other order gives another coverage: extended reads of one 5' end are one fragment)
    other, _ = ref.dedup(ext[0], ext[1], None, d, 1, "fragment")
    assert np.array_equal(other, out)
    wrong, _ = ref.dedup(s, e, None, d, 1, "fragment")
    assert not np.array_equal(cov, gr.numpy_pileup(ext[0], ext[1], wrong, *extent))
    # strand_cross_correlation and extend_reads take the result, compacted or not
    for compact in (True, False):
        removed = psd.remove_duplicates(reads, wrap(d), keep=1, compact=compact)
        want = ref.compacted(s, e, out, d) if compact else (s, e, out, d)
        window = (0, extent[1])      # (the cross-correlation takes no negative extent)
        frames = psd.strand_cross_correlation(removed.reads, removed.strands, max_shift=50, extents=window)
        assert frames[0][list(xcorr_ref.COLUMNS)].to_numpy().tolist() == \
            xcorr_ref.table(want[0], want[1], want[2], want[3], *window, 50)
        longer = psd.extend_reads(removed.reads, removed.strands, 36)
        ext = xcorr_ref.extend(want[0], want[1], want[3], 36)
        assert np.array_equal(host(longer[0]), ext[0]) and np.array_equal(host(longer[1]), ext[1])
        assert longer[2] is removed.reads[2]
    with pytest.raises(psd.PeakSegError) as err:
        psd.remove_duplicates(reads, keep=0)
    assert err.value.status == 25 and "keep" in str(err.value)
    with pytest.raises(psd.PeakSegError) as err:
        psd.remove_duplicates(reads, by="five_prime")
    assert err.value.status == 25 and "strands" in str(err.value)
    with pytest.raises(psd.PeakSegError) as err:
        psd.PeakSegFPOP_reads(reads, [1.0], max_duplicates=0)
    assert err.value.status == 25


# ---- 10: the fixture, determinism, the synthetic reads ----------------------------------------------

def fixture_stranded():
    return gx.fixture_stranded()


def scenario_fixture(psd, wrap):
    s, e, k, d = fixture_stranded()
    for by in MODES:
        for count in (None, k):
            check_marks([(s, e, count, d)], (1, 3), by, wrap, ("fixture", by))
    # the fixture's rows are unique fragments: at keep 1 every count becomes 1
    got = psd.remove_duplicates((wrap(s), wrap(e), wrap(k)), keep=1)
    assert (host(got.reads[2]) == 1).all() and np.array_equal(host(got.reads[0]), s)
    assert got.summary.to_numpy().tolist() == [[int(k.sum()), len(s), len(s), len(s)]]
    # two calls give the same bytes
    reads, strands = [(wrap(s), wrap(e), wrap(k))], [wrap(d)]
    first = dedup_probe(reads, strands, 3, "five_prime", wrap)
    second = dedup_probe(reads, strands, 3, "five_prime", wrap)
    assert first[0] == 0 and first[1][0].tobytes() == second[1][0].tobytes()
    assert first[2].tobytes() == second[2].tobytes() and 0 < first[2][0, 1] < first[2][0, 0]


def scenario_synthetic(psd, wrap):
    from peaksegdisk_amd import synthetic
    s, e, d, dup = synthetic.duplicated_reads(11, 6000, 500000, share=0.2)
    assert dup == 1200
    for strands, by in ((wrap(d), None), (wrap(d), "fragment")):
        got = psd.remove_duplicates((wrap(s), wrap(e)), strands, by=by, compact=False)
        row = got.summary.iloc[0]
        assert (int(row["reads"]), int(row["kept"]), int(row["rows_kept"]), int(row["distinct"])) == \
            (6000, 4800, 4800, 4800)
        assert 5 * (int(row["reads"]) - int(row["distinct"])) == int(row["reads"])     # the stated fifth
        assert np.array_equal(host(got.reads[2]), ref.dedup(s, e, None, d, 1, "five_prime")[0])


# ---- MI355X --------------------------------------------------------------------------------------

_CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process
sys.path[:0] = [%(root)r, %(tests)r]
import test_gpu_dedup as gdd
gdd.child_main(sys.argv[1])
print("dedup-child ok")
"""


def run_child(which, timeout):
    import sys
    from conftest import ROOT
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code, which], capture_output=True, text=True,
                       timeout=timeout)
    print(p.stdout[-4000:])
    assert p.returncode == 0 and "dedup-child ok" in p.stdout, p.stdout[-3000:] + p.stderr[-6000:]


def child_main(which):
    import __graft_entry__ as entry
    entry.build_hip()
    entry.build_oracle()
    import peaksegdisk_amd as psd
    if which == "marks":
        scenario_sizes(as_cuda)
        scenario_order(as_cuda)
        scenario_runs(as_cuda)
        scenario_digits(as_cuda)
        scenario_contigs(as_cuda)
        scenario_refusals(as_cuda)
        scenario_offsets(gx.cuda_array)
    elif which == "end_to_end":
        scenario_compaction(psd, as_cuda)
        scenario_composition(psd, as_cuda)
        scenario_fixture(psd, as_cuda)
        scenario_synthetic(psd, as_cuda)
    else:
        raise ValueError(which)


def dedup_ms():
    ms = [ctypes.c_float() for _ in range(3)]
    _lib().peakseg_hip_reads_last_dedup_ms(*[ctypes.byref(m) for m in ms])
    return tuple(m.value for m in ms)


@GPU
def test_gpu_dedup_every_size_keep_and_mode_numpy(psd):
    scenario_sizes(as_numpy)
    print("last call: keys %.3f ms, sort %.3f ms, runs %.3f ms" % dedup_ms())


@GPU
def test_gpu_dedup_order_and_stability_numpy(psd):
    scenario_order(as_numpy)


@GPU
def test_gpu_dedup_runs_and_carries_numpy(psd):
    scenario_runs(as_numpy)


@GPU
def test_gpu_dedup_every_digit_numpy(psd):
    scenario_digits(as_numpy)


@GPU
def test_gpu_dedup_contigs_numpy(psd):
    scenario_contigs(as_numpy)


@GPU
def test_gpu_dedup_refusals_numpy(psd):
    scenario_refusals(as_numpy)


@GPU
def test_gpu_dedup_marks_and_refusals_cuda_tensors(psd):
    run_child("marks", 300)


@GPU
def test_gpu_dedup_compaction_numpy(psd):
    scenario_compaction(psd, as_numpy)


@GPU
def test_gpu_dedup_composition_numpy(psd):
    scenario_composition(psd, as_numpy)


@GPU
def test_gpu_dedup_fixture_and_determinism_numpy(psd):
    scenario_fixture(psd, as_numpy)


@GPU
def test_gpu_dedup_synthetic_share_numpy(psd):
    scenario_synthetic(psd, as_numpy)


@GPU
def test_gpu_dedup_end_to_end_cuda_tensors(psd):
    run_child("end_to_end", 300)


@GPU
def test_gpu_dedup_emulator_marks_are_the_devices(psd):
    """the emulator build of the same kernel source gives the device's out_count and summary of the
    fixture, byte for byte"""
    from conftest import ROOT
    from peaksegdisk_amd import _native
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["make", "-s", "-C", emu_dir], check=True)
    emu = _native.declare(ctypes.CDLL(os.path.join(emu_dir, "_build", "libpeaksegdisk_emu.so")))
    s, e, k, d = fixture_stranded()
    for by in MODES:
        for entry in ((s, e), (s, e, k)):
            st, device, summary = dedup_probe([entry], [d], 2, by, as_numpy)
            st_emu, emulated, summary_emu = dedup_probe([entry], [d], 2, by, as_numpy, lib=emu)
            assert st == 0 and st_emu == 0, (_lib().peakseg_hip_last_error(), emu.peakseg_hip_last_error())
            assert device[0].tobytes() == emulated[0].tobytes() and summary.tobytes() == summary_emu.tobytes()
            assert 0 < summary[0, 1] <= summary[0, 0]
