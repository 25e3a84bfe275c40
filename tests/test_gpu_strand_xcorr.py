"""Stranded single-end reads: the strand cross-correlation on the device, the fragment-length estimate
and the extension of reads.

The scenario functions are shared with the emulator rehearsal (tests/test_strand_xcorr_emu.py), which
runs them without a GPU on host arrays; the tests marked gpu run them on the MI355X with the reads
once as numpy arrays and once as cuda tensors (in a child process that imports torch first, as
tests/test_gpu_reads.py does).

Expected values never come from the library under test: tables, estimates and extended reads are
those of tests/xcorr_ref.py (numpy and Python integers; pinned in tests/test_strand_xcorr_cpu.py),
pile-ups those of test_gpu_reads.numpy_pileup.  Integer adds commute: every comparison is for
equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import test_gpu_dense as gd
import test_gpu_reads as gr
import xcorr_ref as ref
from conftest import GOLDEN

GPU = pytest.mark.gpu
SENTINEL = -7
LIMIT = 1023


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


def as_numpy(v):
    return np.ascontiguousarray(v)


def as_cuda(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0")


# ---- helpers ---------------------------------------------------------------------------------

def _pointers(values):
    return (ctypes.c_void_p * len(values))(*[gd._address(v)[0] if v is not None and len(v) else None
                                             for v in values])


def xcorr_probe(contigs, strands, extents, max_shift, lib=None):
    """-> (status, the tables int64 (C, max_shift + 1, 6) or None), marshalled here, not by the package"""
    args = gr._read_arguments(contigs, extents, "each")[:8]
    nc = len(contigs)
    table = np.full((nc, max(max_shift, 0) + 1, 6), SENTINEL, np.int64)
    st = (lib or _lib()).peakseg_hip_reads_strand_xcorr(
        0, *args[:5], _pointers(strands), *args[5:], max_shift, table.ctypes.data)
    if st != 0:
        assert (table == SENTINEL).all()      # a refused call has written nothing
        return st, None
    return st, table


def extend_probe(contigs, strands, lengths, wrap):
    """-> (status, [(chromStart, chromEnd) int32 numpy per contig])"""
    args = gr._read_arguments(contigs, [(0, 1)] * len(contigs), "each")
    nc = len(contigs)
    out = [[wrap(np.full(int(e[0].shape[0]), SENTINEL, np.int32)) for e in contigs] for _ in range(2)]
    st = _lib().peakseg_hip_reads_extend(0, args[0], args[1], args[2], args[3], _pointers(strands),
                                         args[5], (ctypes.c_int * nc)(*lengths), _pointers(out[0]),
                                         _pointers(out[1]))
    host = [tuple(np.asarray(out[j][c].cpu() if hasattr(out[j][c], "cpu") else out[j][c])
                  for j in range(2)) for c in range(nc)]
    return st, host


def reads_of_tags(rng, plus, minus, counted=True):
    """(chromStart, chromEnd, count, strand) of reads of length 1-100 whose 5' bases are `plus`
    (plus reads) and `minus` (minus reads), in a random order; counts 0-5, a zero among them"""
    plus, minus = np.asarray(plus, np.int64), np.asarray(minus, np.int64)
    n = len(plus) + len(minus)
    length = rng.integers(1, 101, n)
    start = np.concatenate([plus, minus + 1 - length[len(plus):]])
    end = np.concatenate([plus + length[:len(plus)], minus + 1])
    strand = np.concatenate([np.ones(len(plus), np.int8), -np.ones(len(minus), np.int8)])
    count = rng.integers(0, 6, n)
    order = rng.permutation(n)
    return (start[order].astype(np.int32), end[order].astype(np.int32),
            count[order].astype(np.int32) if counted else None, strand[order])


def check_tables(contigs_np, extents, max_shift, wrap, what):
    """one call against the reference; contigs_np: (chromStart, chromEnd, count or None, strand)"""
    wrapped = [tuple(wrap(v) for v in e[:3] if v is not None) for e in contigs_np]
    strands = [wrap(e[3]) for e in contigs_np]
    st, got = xcorr_probe(wrapped, strands, extents, max_shift)
    assert st == 0, (what, _lib().peakseg_hip_last_error())
    want = [ref.table(e[0], e[1], e[2], e[3], lo, hi, max_shift) for e, (lo, hi) in zip(contigs_np, extents)]
    for c, w in enumerate(want):
        assert got[c].tolist() == w, (what, c)
    return want


def tile_bases():
    return _lib().peakseg_hip_dense_tile_bases()


# ---- 1: the table, for every B and max_shift ----------------------------------------------------

SIZES = lambda T: (1, 2, 300, T - 1, T, T + 1, 2 * T + 5)   # noqa: E731
SHIFTS = (0, 1, 255, 256, 257, 1023)


def edge_reads(rng, lo, B, T, full_tile=None):
    """Reads whose tags lie at the first and last slot of every tile (both strands), one plus tag in
    the last slot of tile 0 with minus tags at every distance 0 .. 1023 behind it (the halo across
    one and two tile edges), 60 tags anywhere, and, with full_tile, a plus tag in every slot of that
    tile."""
    firsts = np.arange(0, B, T)
    lasts = np.minimum(firsts + T - 1, B - 1)
    plus = np.concatenate([firsts, lasts, rng.integers(0, B, 30)])
    minus = np.concatenate([firsts, lasts, rng.integers(0, B, 30)])
    if B >= T:
        behind = T - 1 + np.arange(1024)
        plus = np.concatenate([plus, [T - 1]])
        minus = np.concatenate([minus, behind[behind < B]])
    if full_tile is not None:
        plus = np.concatenate([plus, full_tile * T + np.arange(T)])
    return reads_of_tags(rng, lo + plus, lo + minus)


def scenario_table(wrap, sizes=None, shifts=SHIFTS):
    T = tile_bases()
    assert _lib().peakseg_hip_xcorr_max_shift() == LIMIT
    rng = np.random.default_rng(20250401)
    lo = 1000
    for B in sizes or SIZES(T):
        entry = edge_reads(rng, lo, B, T, full_tile=1 if B > 2 * T else None)
        if B > 2 * T:   # the list's capacity: a tile with a tag in every slot
            p, _ = ref.tags(entry[0], entry[1], entry[2], entry[3], lo, lo + B)
            assert np.count_nonzero(p[T:2 * T]) > T - T // 4
            entry = (entry[0], entry[1], np.maximum(entry[2], 1), entry[3])
            assert np.count_nonzero(ref.tags(*entry, lo, lo + B)[0][T:2 * T]) == T
        for S in shifts:
            want = check_tables([entry], [(lo, lo + B)], S, wrap, (B, S))[0]
            for s, row in enumerate(want):
                assert row[0] == max(B - s, 0)
                if B <= s:      # no pair: the row is all zero
                    assert row == [0] * 6
            if B >= T + 1024 and S == 1023:   # the halo did matter: the last shifts have a cross term
                assert all(want[s][5] > 0 for s in (0, 1, 1022, 1023))


# ---- 2: three contigs in one call -----------------------------------------------------------------

def scenario_three_contigs(wrap):
    """three contigs of different sizes in one call against three calls: one without a plus read
    (every correlation NaN), one without any read and a given extent; a 5' base one slot outside
    each end of the extent is no tag"""
    T = tile_bases()
    rng = np.random.default_rng(12)
    extents = [(500, 500 + 2 * T + 1), (90000, 90000 + T + 5), (7, 7 + 300)]
    lo, hi = extents[0]
    first = edge_reads(rng, lo, hi - lo, T)
    outside = reads_of_tags(rng, [lo - 1, hi], [lo - 1, hi])
    outside = outside[:2] + (np.full(4, 3, np.int32), outside[3])
    first = tuple(np.concatenate([a, b]) for a, b in zip(first, outside))
    lo1, hi1 = extents[1]
    second = reads_of_tags(rng, [], lo1 + rng.integers(0, hi1 - lo1, 200))
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int8))
    contigs = [first, second, empty]
    together = check_tables(contigs, extents, 400, wrap, "three")
    for c in range(3):
        alone = check_tables([contigs[c]], [extents[c]], 400, wrap, ("alone", c))[0]
        assert alone == together[c]
    # the reads outside are no tags: the table is that of the reads inside alone
    inside = tuple(a[:-4] for a in first)
    assert ref.table(*inside, lo, hi, 400) == together[0]
    assert all(math_isnan(ref.correlation(r)) for r in together[1])
    assert all(r[1:] == [0] * 5 for r in together[2]) and together[2][0][0] == 300
    assert any(r[5] > 0 for r in together[0])


def math_isnan(x):
    return x != x


# ---- 3: 64-bit arithmetic, contention, a long contig ----------------------------------------------

def scenario_wide(wrap):
    """products near 2^60 with the largest sum allowed (a read outside the extent counts towards
    it), 5000 reads on one 5' base, and a contig of 257 tiles"""
    T = tile_bases()
    lo, hi = 100, 100 + T + 50
    s = np.array([lo + T - 3, lo + T + 20 - 35, lo - 40], np.int32)     # plus, minus, plus outside
    e = np.array([lo + T + 30, lo + T + 21, lo - 2], np.int32)
    k = np.array([2 ** 30, 2 ** 30 - 2, 1], np.int32)
    d = np.array([1, -1, 1], np.int8)
    assert int(k.sum()) == 2 ** 31 - 1
    want = check_tables([(s, e, k, d)], [(lo, hi)], 400, wrap, "2^60")[0]
    assert want[23][5] == 2 ** 30 * (2 ** 30 - 2) and want[22][5] == 0 and want[0][1] == 2 ** 30
    assert want[0][2] == 2 ** 60
    # many atomics on one address
    s = np.concatenate([np.full(5000, 300), np.full(5000, 310)]).astype(np.int32)
    e = np.concatenate([np.full(5000, 340), np.full(5000, 391)]).astype(np.int32)
    d = np.concatenate([np.ones(5000, np.int8), -np.ones(5000, np.int8)])
    for k in (None, np.full(10000, 3, np.int32)):
        want = check_tables([(s, e, k, d)], [(250, 500)], 255, wrap, "one address")[0]
        w = 1 if k is None else 3
        assert want[90][5] == (5000 * w) ** 2 and want[89][5] == 0
    # more tiles than any stage of one workgroup per contig takes in one trip
    rng = np.random.default_rng(13)
    B = 257 * T
    plus = np.concatenate([rng.integers(0, B, 150), [0, B - 1, 256 * T - 1]])
    minus = np.concatenate([plus[:100] + rng.integers(0, 1024, 100), [0, B - 1, 256 * T + 5]])
    entry = reads_of_tags(rng, 9 + plus, 9 + np.minimum(minus, B - 1))
    want = check_tables([entry], [(9, 9 + B)], 1023, wrap, "257 tiles")[0]
    assert sum(r[5] > 0 for r in want) > 50


# ---- 4: refusals ------------------------------------------------------------------------------------

def scenario_refusals(wrap):
    from peaksegdisk_amd import _native
    assert _native.ERROR_STRAND_ARGUMENTS == 24 and _native.ERROR_READS_ARGUMENTS == 18
    text = _native.status_message(24, "f", "1", "d")
    assert text.startswith("error code 24") and "strand" in text

    def reads(start, end, count=None):
        entry = (wrap(np.array(start, np.int32)), wrap(np.array(end, np.int32)))
        return entry if count is None else entry + (wrap(np.array(count, np.int32)),)

    def strand(values):
        return wrap(np.array(values, np.int8))

    good, good_strand = reads([10, 30, 20], [40, 60, 50]), strand([1, -1, 1])
    two = [(0, 100), (0, 100)]

    def refused(status, contigs, strands, extents, max_shift, *words):
        st, _ = xcorr_probe(contigs, strands, extents, max_shift)
        err = _lib().peakseg_hip_last_error().decode()
        assert st == status, (st, err)
        for w in words:
            assert w in err, err

    refused(24, [good, reads([5, 7, 9], [6, 8, 10])], [good_strand, strand([1, -1, 0])], two, 10,
            "contig 1", "read 2", "strand")
    refused(24, [reads([5, 7, 9], [6, 8, 10]), good], [strand([1, 2, -1]), good_strand], two, 10,
            "contig 0", "read 1", "strand")
    refused(24, [good, good], [good_strand, None], two, 10, "contig 1", "NULL")
    refused(18, [good, reads([5, 7, 9, 9], [6, 8, 9, 9])], [good_strand, strand([1, 1, 1, 1])], two, 10,
            "contig 1", "read 2")
    refused(18, [reads([5, 7, 9], [6, 8, 10], [1, 0, -1]), good], [good_strand, good_strand], two, 10,
            "contig 0", "read 2", "negative")
    # the first bad read of a contig decides, whatever is wrong with it
    n = 1000
    s = np.arange(n, dtype=np.int32) + 500
    e = s + 5
    e[900] = s[900]
    d = np.ones(n, np.int8)
    d[777] = 3
    refused(24, [good, (wrap(s), wrap(e))], [good_strand, wrap(d)], two, 10, "contig 1", "read 777")
    # a sum of exactly 2^31: the read outside the extent counts
    refused(18, [good, reads([5, 6, 300], [50, 60, 310], [2 ** 30, 2 ** 30 - 1, 1])],
            [good_strand, good_strand], two, 10, "contig 1", "2^31")
    refused(24, [good], [good_strand], [(0, 100)], -1, "max_shift")
    refused(24, [good], [good_strand], [(0, 100)], LIMIT + 1, "max_shift")
    refused(24, [good, good], [good_strand, good_strand], [(0, 100), (50, 50)], 10, "contig 1")
    refused(24, [good, good], [good_strand, good_strand], [(0, 100), (60, 50)], 10, "contig 1")
    args = gr._read_arguments([good], [(0, 100)], "each")
    assert _lib().peakseg_hip_reads_strand_xcorr(0, 0, *args[1:5], _pointers([good_strand]), *args[5:8],
                                                 10, None) == 9
    # the extension
    st, _ = extend_probe([good, good], [good_strand, good_strand], [36, 0], wrap)
    err = _lib().peakseg_hip_last_error().decode()
    assert st == 24 and "contig 1" in err and "fragment_length" in err, err
    st, _ = extend_probe([good, good], [good_strand, strand([1, -1, -2])], [36, 36], wrap)
    err = _lib().peakseg_hip_last_error().decode()
    assert st == 24 and "contig 1" in err and "read 2" in err, err
    st, _ = extend_probe([good, reads([5, 9], [6, 9])], [good_strand, strand([1, 1])], [36, 36], wrap)
    err = _lib().peakseg_hip_last_error().decode()
    assert st == 18 and "contig 1" in err and "read 1" in err, err
    st, _ = extend_probe([good], [None], [36], wrap)
    assert st == 24 and "NULL" in _lib().peakseg_hip_last_error().decode()


def scenario_offsets(device_array):
    """Device arrays: an int32 address that is no multiple of 4 is refused; strand arrays that begin
    at each of the four byte offsets of a word give the same table.  device_array(numpy array) ->
    (an object with the device address, a function from it and a byte offset to an address)."""
    T = tile_bases()
    rng = np.random.default_rng(14)
    lo, hi = 1000, 1000 + T + 9
    s, e, k, d = edge_reads(rng, lo, hi - lo, T)
    n = len(s) - 8
    want = None
    held = [device_array(v) for v in (s, e, k, d)]
    base = [h[1] for h in held]
    nc = 1
    for lead in range(4):
        part = (s[:n], e[:n], k[:n], d[lead:lead + n])
        table = np.full((1, 401, 6), SENTINEL, np.int64)
        ptr = [(ctypes.c_void_p * nc)(base[j] + (lead if j == 3 else 0)) for j in range(4)]
        call = lambda shift_by: _lib().peakseg_hip_reads_strand_xcorr(   # noqa: E731
            0, nc, (ctypes.c_longlong * nc)(n), (ctypes.c_void_p * nc)(base[0] + shift_by), ptr[1],
            ptr[2], ptr[3], 1, (ctypes.c_int * nc)(lo), (ctypes.c_int * nc)(hi), 400, table.ctypes.data)
        assert call(0) == 0, _lib().peakseg_hip_last_error()
        assert table[0].tolist() == ref.table(*part, lo, hi, 400), lead
        table[:] = SENTINEL
        assert call(2) == 18 and "multiple of 4" in _lib().peakseg_hip_last_error().decode()
        assert (table == SENTINEL).all()
    del held, want


# ---- 5: the extension ---------------------------------------------------------------------------

LENGTHS = (1, 36, 150, 2 ** 31 - 1)


def limit_reads(rng):
    """300 reads around 10000 and reads within 150 of both int32 limits, both strands of each"""
    start = np.concatenate([rng.integers(9000, 11000, 300),
                            [-2 ** 31, -2 ** 31 + 1, -2 ** 31 + 100, 2 ** 31 - 120, 2 ** 31 - 40] * 2])
    length = np.concatenate([rng.integers(1, 101, 300), [30, 1, 36, 100, 39] * 2])
    strand = np.concatenate([np.where(rng.integers(0, 2, 300) > 0, 1, -1), [1] * 5, [-1] * 5])
    return start.astype(np.int32), (start + length).astype(np.int32), strand.astype(np.int8)


def scenario_extension(psd, wrap):
    rng = np.random.default_rng(15)
    s, e, d = limit_reads(rng)
    k = rng.integers(0, 4, len(s)).astype(np.int32)
    window = (9500, 10500)
    for length in LENGTHS:
        want = ref.extend(s, e, d, length)
        st, got = extend_probe([(wrap(s), wrap(e))], [wrap(d)], [length], wrap)
        assert st == 0, _lib().peakseg_hip_last_error()
        assert np.array_equal(got[0][0], want[0]) and np.array_equal(got[0][1], want[1]), length
        assert (want[0].astype(np.int64) < want[1]).all()
        if length > 200:     # clamped at both limits, not wrapped
            assert want[0].min() == -2 ** 31 and want[1].max() == 2 ** 31 - 1
        # the public function: the kind of memory it was given, the count as it is
        count = wrap(k)
        out = psd.extend_reads((wrap(s), wrap(e), count), wrap(d), length)
        assert type(out[0]) is type(count) and out[2] is count and len(out) == 3
        if hasattr(count, "device"):
            assert out[0].device == count.device and out[1].device == count.device
        # the pile-up of the extended reads is numpy's of the reference's
        st, cov, _, _, _, _ = gr.pileup_probe([tuple(out)], [window])
        assert st == 0 and np.array_equal(cov[0], gr.numpy_pileup(want[0], want[1], k, *window)), length
    # two contigs with a length each
    out = psd.extend_reads([(wrap(s), wrap(e)), (wrap(s[:50]), wrap(e[:50]))], [wrap(d), wrap(d[:50])],
                           [36, 150])
    for got, want in ((out[0], ref.extend(s, e, d, 36)), (out[1], ref.extend(s[:50], e[:50], d[:50], 150))):
        assert len(got) == 2
        for a, b in zip(got, want):
            assert np.array_equal(np.asarray(a.cpu() if hasattr(a, "cpu") else a), b)
    # solved: the keywords against the reference's extended reads
    inside = slice(0, 300)
    for length in (36, 150):
        want = ref.extend(s[inside], e[inside], d[inside], length)
        extent = (int(s[inside].min()), int(e[inside].max()))
        got = psd.PeakSegFPOP_reads((wrap(s[inside]), wrap(e[inside])), [0.0, 10.0], strands=wrap(d[inside]),
                                    fragment_length=length)
        expect = psd.PeakSegFPOP_reads((wrap(want[0]), wrap(want[1])), [0.0, 10.0], extents=extent)
        for a, b in zip(got, expect):
            assert a.segments.equals(b.segments) and len(b.segments) >= 1
        assert len(expect[0].segments) > 3
        frame = psd.coverage_from_reads(wrap(s[inside]), wrap(e[inside]), strands=wrap(d[inside]),
                                        fragment_length=length)
        assert frame.equals(psd.coverage_from_reads(wrap(want[0]), wrap(want[1]), extent=extent))
        pset = psd.ProblemSet.from_reads([(wrap(s[inside]), wrap(e[inside]))], [(0, 10.0)],
                                         strands=[wrap(d[inside])], fragment_length=length)
        try:
            assert pset.contig_starts == [extent[0]] and pset.contig_bases == [extent[1] - extent[0]]
        finally:
            pset.close()
    # exactly one of the two keywords
    reads = (wrap(s[inside]), wrap(e[inside]))
    with pytest.raises(ValueError, match="go together"):
        psd.PeakSegFPOP_reads(reads, [1.0], strands=wrap(d[inside]))
    with pytest.raises(ValueError, match="go together"):
        psd.PeakSegFPOP_reads(reads, [1.0], fragment_length=36)
    with pytest.raises(ValueError, match="go together"):
        psd.ProblemSet.from_reads([reads], [(0, 1.0)], fragment_length=36)
    with pytest.raises(ValueError, match="go together"):
        psd.ProblemSet.from_reads([reads], [(0, 1.0)], strands=[wrap(d[inside])])
    with pytest.raises(ValueError, match="go together"):
        psd.coverage_from_reads(reads[0], reads[1], strands=wrap(d[inside]))
    with pytest.raises(ValueError, match='"auto"'):
        psd.ProblemSet.from_reads([reads], [(0, 1.0)], strands=[wrap(d[inside])], fragment_length="long")
    with pytest.raises(ValueError, match="contig 0 has 300 chromStart and 299 strand"):
        psd.extend_reads(reads, wrap(d[:299]), 36)
    with pytest.raises(psd.PeakSegError) as err:
        psd.extend_reads(reads, wrap(d[inside]), 0)
    assert err.value.status == 24 and "fragment_length" in str(err.value)
    with pytest.raises(psd.PeakSegError) as err:
        psd.strand_cross_correlation(reads, wrap(d[inside]), max_shift=1024)
    assert err.value.status == 24 and "max_shift" in str(err.value)


# ---- 6: the fixture -----------------------------------------------------------------------------

_EXPECTED = {}


def fixture_stranded():
    s, e, k = gr.fixture_reads()
    return s, e, k, ref.hash_strands(len(s))


def expected(name):
    """the reference's tables of the fixture and of the synthetic sets, computed once, shared by the
    tests that need them and left unchanged"""
    if name not in _EXPECTED:
        from peaksegdisk_amd import synthetic
        if name == "fixture":
            s, e, k, d = fixture_stranded()
            _EXPECTED[name] = ref.table(s, e, None, d, gr.FIXTURE_LO, gr.FIXTURE_HI, 400)
        elif name == "both":
            s, e, d = synthetic.stranded_reads(3, 20000, 40, 25, 147, 0, 36, both=True)
            _EXPECTED[name] = ref.table(s, e, None, d, 0, 20000, 400)
        else:
            s, e, d = synthetic.stranded_reads(5, 60000, 120, 60, 150, 20, 36, both=False)
            _EXPECTED[name] = ref.table(s, e, None, d, 0, 60000, 400)
    return _EXPECTED[name]


def scenario_fixture(psd, wrap):
    s, e, k, d = fixture_stranded()
    assert 0.4 < (d > 0).mean() < 0.6
    want = expected("fixture")
    extent = (gr.FIXTURE_LO, gr.FIXTURE_HI)
    contig, strands = [(wrap(s), wrap(e))], [wrap(d)]
    st, first = xcorr_probe(contig, strands, [extent], 400)
    st2, second = xcorr_probe(contig, strands, [extent], 400)
    assert st == 0 and st2 == 0 and first[0].tolist() == want
    assert first.tobytes() == second.tobytes()
    # the public functions: the default extent is the fixture's own
    frames = psd.strand_cross_correlation((wrap(s), wrap(e)), wrap(d))
    assert len(frames) == 1 and list(frames[0].columns) == ["shift"] + list(ref.COLUMNS) + ["correlation"]
    assert frames[0][list(ref.COLUMNS)].to_numpy().tolist() == want
    assert frames[0]["shift"].tolist() == list(range(401))
    r = [ref.correlation(row) for row in want]
    assert np.array_equal(frames[0]["correlation"].to_numpy(), np.array(r), equal_nan=True)
    assert all(str(t) == "int64" for t in frames[0].dtypes[:7])
    # pooled over two contigs: the fixture twice, the second time with its counts as weights
    both = ref.pooled([want, ref.table(s, e, k, d, *extent, 400)])
    shift, length, r_best = ref.estimate(both, 30)
    got = psd.estimate_fragment_length([(wrap(s), wrap(e)), (wrap(s), wrap(e), wrap(k))],
                                       [wrap(d), wrap(d)], min_shift=30)
    assert (got.shift, got.fragment_length, got.correlation) == (shift, length, r_best)
    assert got.curve[list(ref.COLUMNS)].to_numpy().tolist() == both
    assert ref.estimate(want)[0] == psd.estimate_fragment_length((wrap(s), wrap(e)), wrap(d)).shift
    with pytest.raises(ValueError, match="finite"):
        psd.estimate_fragment_length((wrap(s[:3]), wrap(e[:3])), wrap(np.ones(3, np.int8)))


# ---- 7: recovery of a known fragment length -----------------------------------------------------

def scenario_recovery(psd, wrap):
    from peaksegdisk_amd import synthetic
    s, e, d = synthetic.stranded_reads(3, 20000, 40, 25, 147, 0, 36, both=True)
    extent = (0, 20000)
    got = psd.estimate_fragment_length((wrap(s), wrap(e)), wrap(d), extents=extent)
    want = expected("both")
    assert got.curve[list(ref.COLUMNS)].to_numpy().tolist() == want
    assert (got.shift, got.fragment_length) == ref.estimate(want)[:2] == (146, 147)
    assert got.correlation == ref.estimate(want)[2] == 1.0
    auto = psd.PeakSegFPOP_reads((wrap(s), wrap(e)), [0.0, 5.0], strands=wrap(d), fragment_length="auto",
                                 extents=extent)
    fixed = psd.PeakSegFPOP_reads((wrap(s), wrap(e)), [0.0, 5.0], strands=wrap(d), fragment_length=147,
                                  extents=extent)
    for a, b in zip(auto, fixed):
        assert a.segments.equals(b.segments)
    assert len(fixed[0].segments) > 3
    s, e, d = synthetic.stranded_reads(5, 60000, 120, 60, 150, 20, 36, both=False)
    st, table = xcorr_probe([(wrap(s), wrap(e))], [wrap(d)], [(0, 60000)], 400)
    assert st == 0 and table[0].tolist() == expected("single")


# ---- MI355X --------------------------------------------------------------------------------------

_CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process
sys.path[:0] = [%(root)r, %(tests)r]
import test_gpu_strand_xcorr as gx
gx.child_main(sys.argv[1])
print("strand-child ok")
"""


def run_child(which, timeout):
    import sys
    from conftest import ROOT
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code, which], capture_output=True, text=True,
                       timeout=timeout)
    print(p.stdout[-4000:])
    assert p.returncode == 0 and "strand-child ok" in p.stdout, p.stdout[-3000:] + p.stderr[-6000:]


def cuda_array(v):
    t = as_cuda(v)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr()


def child_main(which):
    import __graft_entry__ as entry
    entry.build_hip()
    entry.build_oracle()
    import peaksegdisk_amd as psd
    if which == "tables":
        scenario_table(as_cuda)
        scenario_three_contigs(as_cuda)
        scenario_wide(as_cuda)
        scenario_refusals(as_cuda)
        scenario_offsets(cuda_array)
    elif which == "end_to_end":
        scenario_extension(psd, as_cuda)
        scenario_fixture(psd, as_cuda)
        scenario_recovery(psd, as_cuda)
    else:
        raise ValueError(which)


def xcorr_ms():
    ms = [ctypes.c_float(), ctypes.c_float()]
    _lib().peakseg_hip_reads_last_xcorr_ms(ctypes.byref(ms[0]), ctypes.byref(ms[1]))
    return ms[0].value, ms[1].value


@GPU
def test_gpu_xcorr_table_every_size_and_shift_numpy(psd):
    scenario_table(as_numpy)
    print("last call: tags %.3f ms, cross-correlation %.3f ms" % xcorr_ms())


@GPU
def test_gpu_xcorr_three_contigs_numpy(psd):
    scenario_three_contigs(as_numpy)


@GPU
def test_gpu_xcorr_wide_products_contention_long_contig_numpy(psd):
    scenario_wide(as_numpy)
    print("last call: tags %.3f ms, cross-correlation %.3f ms" % xcorr_ms())


@GPU
def test_gpu_xcorr_refusals_numpy(psd):
    scenario_refusals(as_numpy)


@GPU
def test_gpu_xcorr_tables_and_refusals_cuda_tensors(psd):
    run_child("tables", 300)


@GPU
def test_gpu_strand_extension_numpy(psd):
    scenario_extension(psd, as_numpy)


@GPU
def test_gpu_xcorr_fixture_numpy(psd):
    scenario_fixture(psd, as_numpy)


@GPU
def test_gpu_xcorr_recovery_numpy(psd):
    scenario_recovery(psd, as_numpy)


@GPU
def test_gpu_strand_end_to_end_cuda_tensors(psd):
    run_child("end_to_end", 300)


@GPU
def test_gpu_xcorr_emulator_table_is_the_devices(psd):
    """the emulator build of the same kernel source gives the device's table of the fixture, byte
    for byte"""
    from conftest import ROOT
    from peaksegdisk_amd import _native
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["make", "-s", "-C", emu_dir], check=True)
    emu = _native.declare(ctypes.CDLL(os.path.join(emu_dir, "_build", "libpeaksegdisk_emu.so")))
    s, e, k, d = fixture_stranded()
    extent = [(gr.FIXTURE_LO, gr.FIXTURE_HI)]
    for entry in ((s, e), (s, e, k)):
        st, device = xcorr_probe([entry], [d], extent, 400)
        st_emu, emulated = xcorr_probe([entry], [d], extent, 400, lib=emu)
        assert st == 0 and st_emu == 0, (_lib().peakseg_hip_last_error(), emu.peakseg_hip_last_error())
        assert device.tobytes() == emulated.tobytes() and device[0, :, 5].any()
