"""Duplicate removal without a device: the reference of tests/dedup_ref.py pinned against hand-written
answers and the bundled fixture, the synthetic reads with a stated share of duplicates, and what the
library refuses before it looks for a device."""
import ctypes

import numpy as np
import pytest

import dedup_ref as ref
import test_gpu_reads as gr


@pytest.fixture(scope="module")
def psd():
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd
    return peaksegdisk_amd


ROWS = ([5, 5, 5, 5, 5], [9, 9, 8, 9, 9], [2, 1, 1, 1, 3], [1, 1, 1, -1, 1])


def test_reference_known_answers():
    s, e, k, d = ROWS
    out, summary = ref.dedup(s, e, k, d, 2, "fragment")
    assert out.tolist() == [2, 0, 1, 1, 0] and summary == [8, 4, 3, 3]
    # by 5' end the plus rows share base 5; the minus row's is 8
    out, summary = ref.dedup(s, e, k, d, 2, "five_prime")
    assert out.tolist() == [2, 0, 0, 1, 0] and summary == [8, 3, 2, 2]
    assert ref.key_of("five_prime", 5, 9, -1) == (8, -1) and ref.key_of("five_prime", 5, 9, 1) == (5, 1)
    # a row larger than keep is cut, the next of its key gets nothing; keep beyond every sum: no change
    out, _ = ref.dedup([1, 1, 1], [4, 4, 4], [5, 2, 1], None, 3, "fragment")
    assert out.tolist() == [3, 0, 0]
    out, summary = ref.dedup(s, e, k, d, 2 ** 31 - 1, "fragment")
    assert out.tolist() == k and summary == [8, 8, 5, 3]
    # a row of count 0 opens no key
    out, summary = ref.dedup([1, 1], [4, 4], [0, 2], None, 1, "fragment")
    assert out.tolist() == [0, 1] and summary == [2, 1, 1, 1]
    # no counts: every read counts 1; no strands: every read is plus
    out, summary = ref.dedup([3, 3, -7, 3], [5, 5, 5, 6], None, None, 1, "fragment")
    assert out.tolist() == [1, 0, 1, 1] and summary == [4, 3, 3, 3]
    got = ref.compacted([3, 3, -7, 3], [5, 5, 5, 6], out, [1, 1, -1, 1])
    assert [a.tolist() for a in got] == [[3, -7, 3], [5, 5, 6], [1, 1, 1], [1, -1, 1]]


def test_reference_on_the_fixture():
    """the fixture's rows are unique (chromStart, chromEnd): at keep = 1 every count becomes 1"""
    s, e, k = gr.fixture_reads()
    assert len(set(zip(s.tolist(), e.tolist()))) == len(s) and (k > 0).all()
    out, summary = ref.dedup(s, e, k, None, 1, "fragment")
    assert (out == 1).all()
    assert summary == [int(k.sum()), len(s), len(s), len(s)]


def test_symbols_and_status_text(psd):
    from peaksegdisk_amd import _native as native
    for name in ("peakseg_hip_reads_dedup", "peakseg_hip_reads_compact", "peakseg_hip_dedup_block_rows",
                 "peakseg_hip_dedup_scan_span", "peakseg_hip_reads_last_dedup_ms",
                 "peakseg_hip_reads_last_dedup_passes"):
        assert hasattr(native.lib, name) and name in native.EXPORTED_SYMBOLS
    assert native.ERROR_DEDUP_ARGUMENTS == 25
    text = native.status_message(25, "f", "1", "d")
    assert text.startswith("error code 25") and "keep" in text and "five_prime" in text
    R, P = native.lib.peakseg_hip_dedup_block_rows(), native.lib.peakseg_hip_dedup_scan_span()
    assert R >= 256 and R % 256 == 0 and P >= 1
    for name in ("remove_duplicates", "DuplicateRemoval"):
        assert name in psd.__all__ and hasattr(psd, name)


def test_synthetic_duplicated_reads(psd):
    from peaksegdisk_amd import synthetic
    s, e, d, dup = synthetic.duplicated_reads(7, 5000, 400000, share=0.2)
    assert dup == 1000 and len(s) == len(e) == len(d) == 5000 and ((e - s) == 36).all()
    assert set(d.tolist()) == {1, -1} and s.dtype == np.int32 and d.dtype == np.int8
    for by in ("fragment", "five_prime"):
        _, summary = ref.dedup(s, e, None, d, 1, by)
        assert summary == [5000, 4000, 4000, 4000]
    again = synthetic.duplicated_reads(7, 5000, 400000, share=0.2)
    assert all(np.array_equal(a, b) for a, b in zip((s, e, d), again[:3]))
    assert not np.array_equal(s, np.sort(s))        # shuffled
    with pytest.raises(ValueError, match="do not fit"):
        synthetic.duplicated_reads(7, 5000, 100)


def test_refusals_come_before_the_device(psd):
    from peaksegdisk_amd import _native as native
    lib = native.lib
    s, e = np.array([10, 30], np.int32), np.array([40, 60], np.int32)
    d = np.array([1, -1], np.int8)
    out = np.full(2, -7, np.int32)
    summary = np.full(4, -7, np.int64)
    one = lambda v: (ctypes.c_void_p * 1)(v.ctypes.data if v is not None else None)   # noqa: E731
    n = (ctypes.c_longlong * 1)(2)

    def dedup(n_contigs=1, n_reads=n, start=s, strand=d, by=1, keep=1, out=out, device=1 << 20):
        return lib.peakseg_hip_reads_dedup(device, n_contigs, n_reads, one(start), one(e), None,
                                           None if strand is None else one(strand), 0, by, keep,
                                           one(out), summary.ctypes.data)
    assert dedup(n_contigs=0) == 9
    assert dedup(n_reads=(ctypes.c_longlong * 1)(-1)) == 18
    assert dedup(n_reads=(ctypes.c_longlong * 1)(2 ** 31)) == 25 and "2^31" in native.last_error()
    assert dedup(keep=0) == 25 and "keep" in native.last_error()
    assert dedup(keep=-3) == 25
    assert dedup(by=2) == 25 and "by" in native.last_error()
    assert dedup(strand=None) == 25 and "five_prime" in native.last_error()
    assert dedup(start=None) == 18 and "contig 0" in native.last_error()
    assert dedup(out=None) == 18
    assert dedup(out=s) == 25 and "overlaps" in native.last_error()
    both = np.zeros(4, np.int32)
    assert dedup(start=both[:2], out=both[1:3]) == 25 and "overlaps" in native.last_error()
    assert dedup(strand=None, by=0) == 12      # fragments need no strands
    assert dedup() == 12            # everything the host can see is in order: the device is asked for
    assert (out == -7).all() and (summary == -7).all()
    rows = np.full(1, -7, np.int64)
    keep_count = np.array([1, 0], np.int32)
    outs = [np.full(2, -7, np.int32) for _ in range(3)]

    def compact(keep=keep_count, out_start=outs[0], device=1 << 20):
        return lib.peakseg_hip_reads_compact(device, 1, n, one(s), one(e), None, 0, one(keep),
                                             one(out_start), one(outs[1]), one(outs[2]), None,
                                             rows.ctypes.data)
    assert compact(keep=None) == 18
    assert compact(out_start=e) == 25 and "overlaps" in native.last_error()
    assert compact() == 12
    assert (rows == -7).all() and all((o == -7).all() for o in outs)
    # the Python layer
    with pytest.raises(ValueError, match="neither"):
        psd.remove_duplicates((s, e), d, by="start")
    with pytest.raises(ValueError, match="keep"):
        psd.remove_duplicates((s, e), d, keep=2 ** 31)
    with pytest.raises(ValueError, match="keep"):
        psd.remove_duplicates((s, e), d, keep=1.5)
    with pytest.raises(ValueError, match="contig 0 has 2 chromStart and 1 strand"):
        psd.remove_duplicates((s, e), d[:1])
