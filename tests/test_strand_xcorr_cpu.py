"""Stranded reads without a device: the reference of tests/xcorr_ref.py pinned against the
definitions word for word and against known answers, the synthetic stranded reads, the exact choice
of the shift in peaksegdisk_amd.strand, and what the library refuses before it looks for a device."""
import ctypes
import math

import numpy as np
import pytest

import xcorr_ref as ref


@pytest.fixture(scope="module")
def psd():
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd
    return peaksegdisk_amd


def test_symbols_and_status_text(psd):
    from peaksegdisk_amd import _native as native
    for name in ("peakseg_hip_reads_strand_xcorr", "peakseg_hip_reads_extend",
                 "peakseg_hip_xcorr_max_shift", "peakseg_hip_reads_last_xcorr_ms"):
        assert hasattr(native.lib, name) and name in native.EXPORTED_SYMBOLS
    assert native.ERROR_STRAND_ARGUMENTS == 24
    assert native.lib.peakseg_hip_xcorr_max_shift() == 1023
    text = native.status_message(24, "f", "1", "d")
    assert text.startswith("error code 24") and "strand" in text and "fragment_length" in text
    for name in ("strand_cross_correlation", "estimate_fragment_length", "extend_reads",
                 "FragmentLength"):
        assert name in psd.__all__ and hasattr(psd, name)


def test_reference_table_is_the_definition_word_for_word():
    rng = np.random.default_rng(1)
    for B, S in ((1, 3), (2, 2), (7, 10), (40, 12), (40, 39), (40, 40)):
        n = 3 * B
        start = rng.integers(-3, B + 3, n)
        length = rng.integers(1, 6, n)
        strand = np.where(rng.integers(0, 2, n) > 0, 1, -1)
        count = rng.integers(0, 4, n)
        p, m = ref.tags(start, start + length, count, strand, 0, B)
        # the tags, by a loop over the reads
        p2, m2 = [0] * B, [0] * B
        for i in range(n):
            at = start[i] if strand[i] > 0 else start[i] + length[i] - 1
            if 0 <= at < B:
                (p2 if strand[i] > 0 else m2)[at] += int(count[i])
        assert p.tolist() == p2 and m.tolist() == m2
        assert ref.table_of_tags(p, m, S) == ref.table_by_loops(p, m, S)


def test_reference_known_answers():
    # one plus tag at 2 (count 3), one minus tag at 5 (count 4), on 8 bases
    rows = ref.table([2, 1], [9, 6], [3, 4], [1, -1], 0, 8, 8)
    assert rows[3] == [5, 3, 9, 4, 16, 12]
    assert rows[0] == [8, 3, 9, 4, 16, 0]
    assert rows[6] == [2, 0, 0, 0, 0, 0] and rows[5] == [3, 3, 9, 4, 16, 0]
    assert rows[8] == [0] * 6
    # r of row 3: (5 * 12 - 12) / sqrt((45 - 9) (80 - 16))
    assert ref.correlation(rows[3]) == 48 / (math.sqrt(36.0) * math.sqrt(64.0)) == 1.0
    assert math.isnan(ref.correlation(rows[6])) and math.isnan(ref.correlation(rows[8]))
    assert ref.estimate(rows) == (3, 4, 1.0)
    with pytest.raises(ValueError):
        ref.estimate(rows, 6)
    # the extension: clamped, not wrapped
    s, e = ref.extend([10, 10, 2 ** 31 - 50, -2 ** 31 + 5], [20, 20, 2 ** 31 - 10, -2 ** 31 + 9],
                      [1, -1, 1, -1], 100)
    assert s.tolist() == [10, -80, 2 ** 31 - 50, -2 ** 31] and \
        e.tolist() == [110, 20, 2 ** 31 - 1, -2 ** 31 + 9]


def test_exact_choice_where_floats_tie(psd):
    """two shifts whose correlations round to the same double: the integers decide, and equal ones
    go to the smaller shift"""
    from peaksegdisk_amd import strand
    big = 2 ** 60
    # r^2 = num^2 / (vx vy): rows built so that vx = vy = pairs sq - sum^2 and num differ by one
    def row(num_extra):
        pairs, total, sq = 4, 2 * big, 2 * big * big
        cross = (total * total + num_extra) // pairs
        assert (total * total + num_extra) % pairs == 0
        return [pairs, total, sq, total, sq, cross]
    rows = [row(4 * big), row(4 * big + 4), row(4 * big + 4), row(0)]
    r = [strand.correlation(x) for x in rows]
    assert r[0] == r[1] == r[2] and strand.moments(rows[0])[0] < strand.moments(rows[1])[0]
    assert strand.choose_shift(rows) == 1 == ref.estimate(rows)[0]
    assert strand.choose_shift(rows, 2) == 2 == ref.estimate(rows, 2)[0]
    # negative correlations: the sign first, then the smaller magnitude is the larger r
    neg = [[4, 8, 24, 8, 24, 10], [4, 8, 24, 8, 24, 14], [4, 8, 24, 8, 24, 0]]
    assert [strand.moments(x)[0] for x in neg] == [-24, -8, -64]
    assert strand.choose_shift(neg) == 1 == ref.estimate(neg)[0]
    with pytest.raises(ValueError, match="finite"):
        strand.choose_shift([[4, 8, 16, 8, 24, 10]])
    # pooled sums may pass 2^63: Python integers
    top = [[2 ** 62, 2 ** 62, 2 ** 62, 1, 1, 2 ** 62]] * 1
    both = strand.pooled([np.array(top, dtype=np.int64)] * 4)
    assert both == ref.pooled([top] * 4) == [[2 ** 64, 2 ** 64, 2 ** 64, 4, 4, 2 ** 64]]
    frame = strand.curve_frame(both)
    assert frame["pairs"].iloc[0] == 2 ** 64 and frame["sum_minus"].dtype == np.int64


def test_synthetic_stranded_reads_and_the_pinned_recovery(psd):
    from peaksegdisk_amd import synthetic
    s, e, d = synthetic.stranded_reads(3, 20000, 40, 25, 147, 0, 36, both=True)
    assert len(s) == 2000 and s.dtype == np.int32 and e.dtype == np.int32 and d.dtype == np.int8
    assert (d[:1000] == 1).all() and (d[1000:] == -1).all() and ((e - s) == 36).all()
    assert ((e[1000:] - s[:1000]) == 147).all() and s.min() >= 0 and e.max() <= 20000
    u = synthetic.uniform01(3, 11, 40)
    site = 147 + np.floor(u * (20000 - 2 * 147 - 2)).astype(np.int64)
    frag = s[:1000].astype(np.int64)
    assert ((np.repeat(site, 25) - frag >= 0) & (np.repeat(site, 25) - frag < 147)).all()
    rows = ref.table(s, e, None, d, 0, 20000, 400)
    shift, length, r = ref.estimate(rows)
    assert (shift, length) == (146, 147) and abs(r - 1.0) < 1e-12
    others = sorted(ref.correlation(x) for j, x in enumerate(rows) if j != 146)
    assert abs(others[-1] - 0.149) < 0.001
    # one read per fragment, jittered lengths: the generator's rules
    s, e, d = synthetic.stranded_reads(5, 60000, 120, 60, 150, 20, 36, both=False)
    assert len(s) == 7200 and set(d.tolist()) == {1, -1}
    assert ((synthetic.uniform01(5, 14, 7200) < 0.5) == (d > 0)).all()
    length = 150 + np.floor(synthetic.uniform01(5, 12, 7200) * 41).astype(np.int64) - 20
    assert length.min() == 130 and length.max() == 170
    site = 170 + np.floor(synthetic.uniform01(5, 11, 120) * (60000 - 342)).astype(np.int64)
    fs = np.repeat(site, 60) - np.floor(synthetic.uniform01(5, 13, 7200) * length).astype(np.int64)
    assert np.array_equal(np.where(d > 0, s, e - length), fs)
    again = synthetic.stranded_reads(5, 60000, 120, 60, 150, 20, 36, both=False)
    assert all(np.array_equal(a, b) for a, b in zip((s, e, d), again))


def test_fixture_strands_by_hash(psd):
    d = ref.hash_strands(8)
    from peaksegdisk_amd.synthetic import splitmix64
    assert d.tolist() == [1 if int(splitmix64(1, np.uint64(i))) % 2 == 0 else -1 for i in range(8)]


def test_refusals_come_before_the_device(psd):
    from peaksegdisk_amd import _native as native
    lib = native.lib
    s, e = np.array([10, 30], np.int32), np.array([40, 60], np.int32)
    d = np.array([1, -1], np.int8)
    one = lambda v: (ctypes.c_void_p * 1)(v.ctypes.data if v is not None else None)   # noqa: E731
    n = (ctypes.c_longlong * 1)(2)
    lo, hi = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(100)
    table = np.zeros((1, 11, 6), np.int64)

    def xcorr(n_contigs=1, n_reads=n, start=s, strand=d, lo=lo, hi=hi, max_shift=10, device=1 << 20):
        return lib.peakseg_hip_reads_strand_xcorr(device, n_contigs, n_reads, one(start), one(e), None,
                                                  one(strand), 0, lo, hi, max_shift, table.ctypes.data)
    assert xcorr(n_contigs=0) == 9
    assert xcorr(n_reads=(ctypes.c_longlong * 1)(-1)) == 18
    assert xcorr(start=None) == 18 and "chromStart" in native.last_error()
    assert xcorr(strand=None) == 24 and "contig 0" in native.last_error()
    assert xcorr(max_shift=-1) == 24 and xcorr(max_shift=1024) == 24
    assert "max_shift" in native.last_error()
    assert xcorr(hi=(ctypes.c_int * 1)(0)) == 24 and "contig 0" in native.last_error()
    assert xcorr(lo=(ctypes.c_int * 1)(-5)) == 18
    assert xcorr() == 12            # everything the host can see is in order: the device is asked for
    out = [np.zeros(2, np.int32), np.zeros(2, np.int32)]

    def extend(length=36, strand=d, device=1 << 20):
        return lib.peakseg_hip_reads_extend(device, 1, n, one(s), one(e), one(strand), 0,
                                            (ctypes.c_int * 1)(length), one(out[0]), one(out[1]))
    assert extend(length=0) == 24 and "fragment_length" in native.last_error()
    assert extend(strand=None) == 24
    assert extend() == 12
    assert not table.any() and not out[0].any()
    # the Python layer
    with pytest.raises(ValueError, match="go together"):
        psd.PeakSegFPOP_reads((s, e), [1.0], strands=d)
    with pytest.raises(ValueError, match="go together"):
        psd.ProblemSet.from_reads([(s, e)], [(0, 1.0)], fragment_length=5)
    with pytest.raises(ValueError, match="dtype int16, not int8"):
        psd.ProblemSet.from_reads([(s, e)], [(0, 1.0)], strands=[d.astype(np.int16)], fragment_length=5)
    with pytest.raises(ValueError, match="min_shift"):
        psd.estimate_fragment_length((s, e), d, max_shift=10, min_shift=11)
    with pytest.raises(ValueError, match="an integer, or one per contig"):
        psd.extend_reads((s, e), d, 36.5)
