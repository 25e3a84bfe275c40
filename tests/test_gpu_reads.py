"""Coverage from aligned reads: the pile-up on the device, ProblemSet.from_reads,
PeakSegFPOP_reads and coverage_from_reads.

The scenario functions are shared with the emulator rehearsal (tests/test_reads_emu.py), which runs
them without a GPU on host arrays; the tests marked gpu run them on the MI355X with the reads once
as numpy arrays and once as cuda tensors (in a child process that imports torch first, as
tests/test_gpu_dense.py does).

Expected values never come from the library under test: the pile-up is compared with numpy_pileup
below (np.add.at on a difference array and cumsum, the clipping done in numpy; checked against a
base-by-base loop in tests/test_reads_cpu.py), its encoding with test_gpu_dense.rle, solved sets
with ProblemSet.from_dense on the numpy pile-up (which tests/test_gpu_dense.py pins to the oracle),
and one solved problem with the oracle's own files.  Integer adds commute: every comparison is for
equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import test_gpu_dense as gd
from conftest import GOLDEN
from test_gpu_dense import as_cuda, as_numpy

GPU = pytest.mark.gpu
FIXTURE_LO, FIXTURE_HI = 175434087, 175507002
WINDOW = (FIXTURE_LO + 20000, FIXTURE_LO + 50000)
PENALTIES = [0.0, 100.0, 10000.0, float("inf")]


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


# ---- helpers ---------------------------------------------------------------------------------

def numpy_pileup(start, end, count, lo, hi, mode="each"):
    """The coverage of [lo, hi), int32: +count at chromStart, -count at chromEnd, cumulative sum
    (the reference's vignette), with reads clipped to the extent and, for mode "end", a read
    standing for its last base."""
    e = np.asarray(end, dtype=np.int64)
    s = e - 1 if mode == "end" else np.asarray(start, dtype=np.int64)
    k = np.ones(len(e), np.int64) if count is None else np.asarray(count, dtype=np.int64)
    inside = (e > lo) & (s < hi)
    diff = np.zeros(hi - lo + 1, np.int64)
    np.add.at(diff, np.maximum(s[inside], lo) - lo, k[inside])
    np.add.at(diff, np.minimum(e[inside], hi) - lo, -k[inside])
    cov = np.cumsum(diff)[:-1]
    assert cov.min() >= 0 and cov.max() < 2 ** 31
    return cov.astype(np.int32)


def fixture_reads():
    d = np.load(os.path.join(GOLDEN, "ChIPreads_H3K4me3.npz"))
    return d["chromStart"], d["chromEnd"], d["count"]


def _read_arguments(contigs, extents, mode):
    """the read arguments of the C ABI from wrapped arrays, marshalled here (not by the package)"""
    nc = len(contigs)
    where = [gd._address(v) for entry in contigs for v in entry if v is not None]
    assert len({w for _, w in where}) <= 1
    on_device = where[0][1] if where else 0
    ptrs = [(ctypes.c_void_p * nc)(*[gd._address(entry[j])[0] if j < len(entry) and
                                     entry[j] is not None and len(entry[j]) else None
                                     for entry in contigs]) for j in range(3)]
    n_reads = (ctypes.c_longlong * nc)(*[int(entry[0].shape[0]) for entry in contigs])
    lo = (ctypes.c_int * nc)(*[e[0] for e in extents])
    hi = (ctypes.c_int * nc)(*[e[1] for e in extents])
    return [nc, n_reads, ptrs[0], ptrs[1], ptrs[2], on_device, lo, hi, {"each": 0, "end": 1}.get(mode, mode)]


SENTINEL = -7


def pileup_probe(contigs, extents, mode="each"):
    """-> (status, coverage per contig, runs int64[C], count, weight, run_end (concatenated))"""
    args = _read_arguments(contigs, extents, mode)
    bases = [max(int(hi) - int(lo), 0) for lo, hi in extents]
    total = sum(bases)
    cov = np.full(max(total, 1), SENTINEL, np.int32)
    runs = np.zeros(len(contigs), np.int64)
    out = [np.full(max(total, 1), SENTINEL, np.int32) for _ in range(3)]
    st = _lib().peakseg_hip_reads_pileup_probe(0, *args, cov.ctypes.data, runs.ctypes.data,
                                               out[0].ctypes.data, out[1].ctypes.data,
                                               out[2].ctypes.data)
    if st != 0:
        # a refused call has written nothing: nothing was launched after the refusal
        assert (cov == SENTINEL).all() and all((o == SENTINEL).all() for o in out) and not runs.any()
        return st, None, runs, None, None, None
    offs = np.concatenate([[0], np.cumsum(bases)])
    k = int(runs.sum())
    return st, [cov[offs[c]:offs[c + 1]] for c in range(len(contigs))], runs, out[0][:k], \
        out[1][:k], out[2][:k]


def check_pileup(contigs_np, extents, mode, wrap, what):
    """one probe call against numpy: the coverage and its run-length encoding"""
    wrapped = [tuple(None if v is None else wrap(v) for v in entry) for entry in contigs_np]
    st, cov, runs, count, weight, run_end = pileup_probe(wrapped, extents, mode)
    assert st == 0, (what, _lib().peakseg_hip_last_error())
    want = [numpy_pileup(e[0], e[1], e[2] if len(e) > 2 else None, lo, hi, mode)
            for e, (lo, hi) in zip(contigs_np, extents)]
    for c, w in enumerate(want):
        assert np.array_equal(cov[c], w), (what, c)
    enc = [gd.rle(w) for w in want]
    assert runs.tolist() == [len(x[0]) for x in enc], what
    assert np.array_equal(count, np.concatenate([x[0] for x in enc])), what
    assert np.array_equal(weight, np.concatenate([x[1] for x in enc])), what
    assert np.array_equal(run_end, np.concatenate([x[2] for x in enc])), what
    return want


def reads_around(rng, lo, hi, n, tile):
    """n unsorted reads of length 1-150 drawn around [lo, hi), with the cases that matter forced in:
    a start at lo, an end exactly at hi, a straddler of each edge, reads wholly outside on either
    side (touching the extent included), and one across every tile border of the extent"""
    start = rng.integers(lo - 160, hi + 10, n)
    length = rng.integers(1, 151, n)
    forced = [(lo, 1), (lo, 40), (hi - 1, 1), (max(lo, hi - 30), min(30, hi - lo)),
              (lo - 20, 50), (hi - 7, 100), (lo - 160, 500 + (hi - lo)),
              (lo - 30, 30), (lo - 100, 10), (hi, 25), (hi + 5, 1)]
    forced += [(b - 3, 10) for b in range(lo + tile, hi, tile)]
    for j, (s, ln) in enumerate(forced):
        start[j], length[j] = s, ln
    order = rng.permutation(n)
    start, length = start[order], length[order]
    count = rng.integers(0, 6, n)
    return start.astype(np.int32), (start + length).astype(np.int32), count.astype(np.int32)


# ---- the pile-up against numpy -----------------------------------------------------------------

def scenario_pileup(wrap):
    T = _lib().peakseg_hip_dense_tile_bases()
    rng = np.random.default_rng(20250301)
    lo = 1000
    for n_bases in (1, T - 1, T, T + 1, 2 * T + 1):
        s, e, k = reads_around(rng, lo, lo + n_bases, 300, T)
        for mode in ("each", "end"):
            for entry in ((s, e), (s, e, k)):
                cov = check_pileup([entry], [(lo, lo + n_bases)], mode, wrap,
                                   (n_bases, mode, len(entry)))[0]
                assert len(entry) == 3 or cov.max() > 0
    # an extent that starts at 0, and a None in the count's place
    s, e, k = reads_around(rng, 200, 200 + T + 9, 300, T)
    check_pileup([(s, e, None)], [(0, T + 300)], "each", wrap, "extent from 0")


def scenario_three_contigs(wrap):
    """three contigs of different extents in one call against three calls: a tile's carry must not
    leak into the next contig; the middle one has no read inside its extent"""
    T = _lib().peakseg_hip_dense_tile_bases()
    rng = np.random.default_rng(11)
    extents = [(500, 500 + 2 * T + 1), (90000, 90000 + T + 5), (7, 7 + T - 1)]
    contigs = [reads_around(rng, lo, hi, 400, T) for lo, hi in extents]
    s = rng.integers(0, 80000, 50).astype(np.int32)          # all in front of [90000, ...)
    contigs[1] = (s, (s + 100).astype(np.int32), contigs[1][2][:50].copy())
    for mode in ("each", "end"):
        together = check_pileup(contigs, extents, mode, wrap, ("three", mode))
        for c in range(3):
            alone = check_pileup([contigs[c]], [extents[c]], mode, wrap, ("alone", c, mode))[0]
            assert np.array_equal(alone, together[c])
        assert not together[1].any() and together[0].any() and together[2].any()
    wrapped = [tuple(wrap(v) for v in entry) for entry in contigs]
    runs = pileup_probe(wrapped, extents)[2]
    assert runs[1] == 1
    # a contig without any read at all
    empty = np.zeros(0, np.int32)
    check_pileup([contigs[0], (empty, empty)], [extents[0], (40, 40 + T + 1)], "each", wrap,
                 "no reads")


LONG_TILES = 3 * 256        # of the long contig: the scan of the tile sums takes 4 tiles per thread


def long_contig_reads(weighted):
    """(contigs, extents) of scenario_long_contig: a contig of LONG_TILES tiles and half a tile more
    and a short one behind it.  The long one has 30000 short reads (reads_around: one across every
    tile border), 20 reads that each span hundreds of tiles, and single-base reads on the last base
    in front of a tile wherever the coverage there would equal that in front of the tile before."""
    T = _lib().peakseg_hip_dense_tile_bases()
    rng = np.random.default_rng(20250302)
    lo = 5000
    hi = lo + LONG_TILES * T + T // 2 + 1
    s, e, k = reads_around(rng, lo, hi, 30000, T)
    first = rng.integers(lo - 50, lo + 200 * T, 20)
    first[0] = lo + T // 3                                   # from the first tile to the last
    last = np.minimum(first + rng.integers(150 * T, 600 * T, 20), hi + 77)
    last[0] = hi - 9
    s = np.concatenate([s, first.astype(np.int32)])
    e = np.concatenate([e, last.astype(np.int32)])
    k = np.concatenate([k, rng.integers(1, 9, 20).astype(np.int32)])
    cov = numpy_pileup(s, e, k if weighted else None, lo, hi)
    n_tiles = -(-(hi - lo) // T)
    carry = cov[T - 1::T][:n_tiles - 1].astype(np.int64)     # in front of tiles 1, 2, ...
    more = []
    for t in range(1, len(carry)):                           # (carry[t - 1] is final when t is reached)
        if carry[t] == carry[t - 1]:
            carry[t] += 1
            more.append(lo + (t + 1) * T - 1)
    more = np.array(more, dtype=np.int32)
    s, e = np.concatenate([s, more]), np.concatenate([e, more + 1])
    k = np.concatenate([k, np.ones(len(more), np.int32)])
    order = rng.permutation(len(s))
    long_one = (s[order], e[order], k[order]) if weighted else (s[order], e[order])
    short_extent = (300, 300 + T + 5)
    short_one = reads_around(rng, short_extent[0], short_extent[1], 300, T)
    return [long_one, short_one if weighted else short_one[:2]], [(lo, hi), short_extent]


def scenario_long_contig(wrap):
    """A contig of more than 256 tiles: a thread of tile_scan_kernel takes a share of several tiles
    and walks it twice, and the carry it writes must advance from tile to tile.  Every read counting
    1, and count as weights."""
    T = _lib().peakseg_hip_dense_tile_bases()
    for weighted in (False, True):
        contigs, extents = long_contig_reads(weighted)
        want = check_pileup(contigs, extents, "each", wrap, ("long contig", weighted))
        # what the scenario is for did occur, from the numpy pile-up: a share of several tiles, and
        # in front of every tile a coverage that is not zero and not that of the tile before
        n_tiles = -(-len(want[0]) // T)
        assert n_tiles > 256 and -(-n_tiles // 256) >= 2, n_tiles
        carry = want[0][T - 1::T][:n_tiles - 1].astype(np.int64)
        assert len(carry) == n_tiles - 1 and carry.min() > 0 and np.all(np.diff(carry) != 0)
        assert len(set(carry.tolist())) > 8
        assert len(want[1]) == T + 5 and want[1].any()       # (its first tile is not the call's first)


def scenario_one_address(wrap):
    """5000 identical reads and 5000 reads of length 1 at one base: many adds to one address"""
    s = np.concatenate([np.full(5000, 300), np.full(5000, 350)]).astype(np.int32)
    e = np.concatenate([np.full(5000, 420), np.full(5000, 351)]).astype(np.int32)
    k = np.full(10000, 3, np.int32)
    for entry in ((s, e), (s, e, k)):
        cov = check_pileup([entry], [(250, 500)], "each", wrap, "one address")[0]
        w = 1 if len(entry) == 2 else 3
        assert cov[49] == 0 and cov[50] == 5000 * w and cov[100] == 10000 * w and cov[170] == 0


def scenario_device_offsets(wrap):
    """device read arrays that begin at each of the four 4-byte offsets of a 16-byte line"""
    T = _lib().peakseg_hip_dense_tile_bases()
    rng = np.random.default_rng(5)
    s, e, k = reads_around(rng, 1000, 1000 + T + 9, 300 + 16, T)
    base = [wrap(v) for v in (s, e, k)]
    assert base[0].data_ptr() % 16 == 0
    for lead in range(4):
        part = [b[lead:lead + 300] for b in base]
        st, cov, _, _, _, _ = pileup_probe([tuple(part)], [(1000, 1000 + T + 9)])
        want = numpy_pileup(s[lead:lead + 300], e[lead:lead + 300], k[lead:lead + 300], 1000,
                            1000 + T + 9)
        assert st == 0 and np.array_equal(cov[0], want), lead


# ---- refusals -----------------------------------------------------------------------------------

def _create(contigs, extents, mode, problems):
    args = _read_arguments(contigs, extents, mode)
    n = len(problems)
    pc = (ctypes.c_int * n)(*[c for c, _ in problems])
    pp = (ctypes.c_double * n)(*[p for _, p in problems])
    h = ctypes.c_void_p()
    st = _lib().peakseg_hip_problem_set_create_reads(0, *args, n, pc, pp, 0, ctypes.byref(h))
    if st == 0:
        _lib().peakseg_hip_problem_set_destroy(h)
    else:
        assert not h.value
    return st


def scenario_refusals(wrap):
    from peaksegdisk_amd import _native
    assert _native.ERROR_READS_ARGUMENTS == 18
    good = (wrap(np.array([10, 30, 20], np.int32)), wrap(np.array([40, 60, 50], np.int32)))

    def refused(contigs, extents, mode, *words):
        st = pileup_probe(contigs, extents, mode)[0]
        err = _lib().peakseg_hip_last_error().decode()
        assert st == 18, (st, err)
        for w in words:
            assert w in err, err
        assert _create(contigs, extents, mode, [(0, 1.0)]) == 18
        # penalties are refused before any of it
        assert _create(contigs, extents, mode, [(0, 1.0), (0, float("nan"))]) == 1
        assert _create(contigs, extents, mode, [(0, -0.5)]) == 2

    def reads(start, end, count=None):
        entry = (wrap(np.array(start, np.int32)), wrap(np.array(end, np.int32)))
        return entry if count is None else entry + (wrap(np.array(count, np.int32)),)

    two = [(0, 100), (0, 100)]
    refused([good, reads([5, 7, 9, 9], [6, 8, 9, 9])], two, "each", "contig 1", "read 2")
    refused([good, reads([5, 9], [6, 8])], two, "end", "contig 1", "read 1")
    refused([reads([5, 7, 9], [6, 8, 10], [1, 0, -1]), good], two, "each", "contig 0", "read 2",
            "negative")
    # a bad read far from the first slice, and outside the extent
    n = 1000
    s = np.arange(n, dtype=np.int32) + 500
    e = s + 5
    e[777] = s[777]
    e[900] = s[900] - 1
    refused([good, (wrap(s), wrap(e))], two, "each", "contig 1", "read 777")
    refused([good, reads([5, 6], [50, 60], [2 ** 30, 2 ** 30])], two, "each", "contig 1", "2^31")
    refused([good, good], [(0, 100), (50, 50)], "each", "contig 1")
    refused([good, good], [(0, 100), (60, 50)], "each", "contig 1")
    refused([good, good], [(0, 100), (-1, 50)], "each", "contig 1")
    refused([good], [(0, 100)], 2, "bases_counted")
    # just below the limit: accepted, exact
    st, cov, runs, count, _, _ = pileup_probe(
        [reads([5, 6], [50, 60], [2 ** 30, 2 ** 30 - 1])], [(0, 100)])
    assert st == 0 and cov[0][5] == 2 ** 30 and cov[0][6] == 2 ** 31 - 1 and cov[0][59] == 2 ** 30 - 1
    assert count.tolist() == [0, 2 ** 30, 2 ** 31 - 1, 2 ** 30 - 1, 0]
    assert _create([good], [(0, 100)], "each", [(0, 1.0), (0, float("inf"))]) == 0
    # no contig: the reference's "no data"
    args = _read_arguments([good], [(0, 100)], "each")
    args[0] = 0
    assert _lib().peakseg_hip_reads_pileup_probe(0, *args, None, None, None, None, None) == 9


def scenario_python_refusals(psd, wrap):
    from peaksegdisk_amd import ProblemSet
    s, e = np.array([10, 30], np.int32), np.array([40, 60], np.int32)
    one = [(0, 1.0)]
    with pytest.raises(ValueError, match="contig 1 chromEnd has dtype int64"):
        ProblemSet.from_reads([(wrap(s), wrap(e)), (wrap(s), e.astype(np.int64))], one)
    with pytest.raises(ValueError, match="contig 0 chromStart is not a contiguous 1-d"):
        ProblemSet.from_reads([(np.zeros((2, 2), np.int32), wrap(e))], one)
    with pytest.raises(ValueError, match="contig 0 has 2 chromStart and 1 count"):
        ProblemSet.from_reads([(s, e, np.ones(1, np.int32))], one)
    empty = np.zeros(0, np.int32)
    with pytest.raises(ValueError, match="contig 1 has no reads"):
        ProblemSet.from_reads([(wrap(s), wrap(e)), (wrap(empty), wrap(empty))], one)
    with pytest.raises(ValueError, match="bases_counted"):
        ProblemSet.from_reads([(wrap(s), wrap(e))], one, bases_counted="all")
    with pytest.raises(ValueError, match="must be integer"):
        psd.PeakSegFPOP_reads((s.astype(float), e), [1.0])
    with pytest.raises(ValueError, match="must fit 32-bit"):
        psd.PeakSegFPOP_reads((s.astype(np.int64), e.astype(np.int64) + 2 ** 40), [1.0])
    with pytest.raises(ValueError, match="pen.num"):
        psd.PeakSegFPOP_reads((s, e), [-1.0])
    if wrap is as_cuda:
        with pytest.raises(ValueError, match="contig 1 is in host memory but contig 0 is in device"):
            ProblemSet.from_reads([(wrap(s), wrap(e)), (s, e)], one)
        with pytest.raises(ValueError, match="contig 0 is in host memory but contig 0 is in device"):
            ProblemSet.from_reads([(wrap(s), e)], one)
    with pytest.raises(psd.PeakSegError) as err:
        psd.PeakSegFPOP_reads((wrap(s), wrap(s)), [1.0])
    assert err.value.status == 18 and "read 0" in str(err.value)


# ---- end to end ----------------------------------------------------------------------------------

_EXPECTED = {}
CONFIGS = [("each", False), ("end", False), ("each", True)]  # (bases_counted, count as weights)


def expected_fits(psd, extent):
    """from_dense on the numpy pile-ups of the fixture, one contig per entry of CONFIGS, at
    PENALTIES: computed once per extent, shared by the tests that need it and left unchanged"""
    if extent not in _EXPECTED:
        s, e, k = fixture_reads()
        lo, hi = extent
        covs = [numpy_pileup(s, e, k if weighted else None, lo, hi, mode) for mode, weighted in CONFIGS]
        pset = psd.ProblemSet.from_dense(covs, [(c, p) for c in range(3) for p in PENALTIES])
        try:
            pset.solve()
            _EXPECTED[extent] = (pset.segment_columns(), pset.segment_columns(first_chromStart=[lo] * 3),
                                 [pset.loss(p) for p in range(3 * len(PENALTIES))],
                                 pset.segment_stats(first_chromStart=[lo] * 3))
        finally:
            pset.close()
    return _EXPECTED[extent]


def scenario_fixture(psd, wrap, extents):
    """from_reads against from_dense on the numpy pile-up: the two "each" configurations as the two
    contigs of one call, the "end" configuration in a call of its own"""
    s, e, k = fixture_reads()
    n_pen = len(PENALTIES)
    for extent in extents:
        plain, genomic, losses, stats = expected_fits(psd, extent)
        whole = extent == (FIXTURE_LO, FIXTURE_HI)
        for mode, configs in (("each", [0, 2]), ("end", [1])):
            assert all(CONFIGS[c][0] == mode for c in configs)
            contigs = [(wrap(s), wrap(e), wrap(k)) if CONFIGS[c][1] else (wrap(s), wrap(e))
                       for c in configs]
            pset = psd.ProblemSet.from_reads(
                contigs, [(j, p) for j in range(len(configs)) for p in PENALTIES],
                extents=None if whole else [extent] * len(configs), bases_counted=mode)
            try:
                assert pset.contig_starts == [extent[0]] * len(configs)
                assert pset.contig_bases == [extent[1] - extent[0]] * len(configs)
                pset.solve()
                got_plain = pset.segment_columns()
                got_genomic = pset.segment_columns(first_chromStart=pset.contig_starts)
                got_stats = pset.segment_stats(first_chromStart=pset.contig_starts)
                for j, c in enumerate(configs):
                    for q in range(n_pen):
                        p, ref = j * n_pen + q, c * n_pen + q
                        what = (extent, CONFIGS[c], PENALTIES[q])
                        for got, want in ((got_plain, plain), (got_genomic, genomic), (got_stats, stats)):
                            assert len(got[p]) == len(want[ref])
                            for a, b in zip(got[p], want[ref]):
                                assert a.dtype == b.dtype and np.array_equal(a, b), what
                        assert np.array_equal(pset.loss(p), losses[ref]), what
                    # the models are not all trivial: the comparison says something
                    assert len(got_plain[j * n_pen][0]) > 3 and len(got_plain[j * n_pen + 3][0]) == 1
                    assert got_genomic[j * n_pen][1][0] == extent[1]
            finally:
                pset.close()


def scenario_api(psd, wrap, tmp_path, oracle_det):
    """PeakSegFPOP_reads against PeakSegFPOP_dense of the numpy pile-up, coverage_from_reads against
    the numpy run-length frame, and one problem against the oracle's own files.  The window at
    penalty 100 is the problem the oracle solves too; the other configurations (count as weights,
    "end", converted int64 input with the default extent) use a 3000-base part of it."""
    import pandas as pd
    s, e, k = fixture_reads()
    lo, hi = WINDOW
    small = (lo + 12000, lo + 15000)
    cov = numpy_pileup(s, e, None, lo, hi)
    cov_end = numpy_pileup(s, e, k, lo, hi, "end")
    pens = [[100.0, float("inf")], [50.0]]
    got = psd.PeakSegFPOP_reads([(wrap(s), wrap(e)), (wrap(s), wrap(e), wrap(k))], pens,
                                chrom="chr2", extents=[WINDOW, small], bases_counted="each",
                                stats=True)
    got_end = psd.PeakSegFPOP_reads((wrap(s), wrap(e), wrap(k)), pens[1], chrom="chr2",
                                    extents=small, bases_counted="end", stats=True)
    want = psd.PeakSegFPOP_dense([cov, numpy_pileup(s, e, k, *small)], pens, chrom="chr2",
                                 chrom_starts=[lo, small[0]], stats=True)
    want_end = psd.PeakSegFPOP_dense(numpy_pileup(s, e, k, small[0], small[1], "end"), pens[1],
                                     chrom="chr2", chrom_starts=[small[0]], stats=True)
    assert [len(g) for g in got] == [2, 1] and len(got_end) == 1

    def same(fit, ref, what):
        keep = [n for n in ref.loss.columns if n != "seconds"]
        for a, b in ((fit.segments, ref.segments), (fit.loss[keep], ref.loss[keep]),
                     (fit.stats, ref.stats)):
            assert a.equals(b), what
            assert list(a.dtypes) == list(b.dtypes), what
        assert list(fit.loss.columns) == list(ref.loss.columns), what
    for c in range(2):
        for j in range(len(pens[c])):
            same(got[c][j], want[c][j], (c, j))
    same(got_end[0], want_end[0], "end")
    assert len(got[0][0].segments) > 3 and got[0][0].segments["chromEnd"].iloc[0] == hi
    # int64 reads are converted; the default extent is the reads' own
    inside = (s >= small[0]) & (e <= small[1])
    conv = psd.PeakSegFPOP_reads((s[inside].astype(np.int64), e[inside].astype(np.int64)), [50.0])
    lo2, hi2 = int(s[inside].min()), int(e[inside].max())
    ref = psd.PeakSegFPOP_dense(numpy_pileup(s[inside], e[inside], None, lo2, hi2), [50.0],
                                chrom_starts=[lo2])
    assert conv[0].segments.equals(ref[0].segments) and len(ref[0].segments) >= 3
    assert conv[0].segments["chrom"].iloc[0] == "chrUnknown"

    # the coverage frame: what writeBedGraph accepts
    frame = psd.coverage_from_reads(wrap(s), wrap(e), chrom="chr2", extent=WINDOW)
    count, weight, ends = gd.rle(cov)
    ref = pd.DataFrame({"chrom": "chr2", "chromStart": (lo + ends - weight).astype(np.int32),
                        "chromEnd": (lo + ends).astype(np.int32), "count": count})
    assert frame.equals(ref) and list(frame.dtypes) == list(ref.dtypes)
    assert (frame["count"] == 0).any()
    assert (frame["chromStart"].to_numpy()[1:] == frame["chromEnd"].to_numpy()[:-1]).all()
    weighted = psd.coverage_from_reads(wrap(s), wrap(e), wrap(k), extent=WINDOW, bases_counted="end")
    count, weight, ends = gd.rle(cov_end)
    assert weighted["count"].tolist() == count.tolist() and \
        weighted["chromEnd"].tolist() == (lo + ends).tolist()
    whole = psd.coverage_from_reads(wrap(s), wrap(e))
    assert len(whole) == 12051 and whole["count"].max() == 203
    assert (whole["chromStart"].iloc[0], whole["chromEnd"].iloc[-1]) == (FIXTURE_LO, FIXTURE_HI)
    assert int((whole["count"].astype(np.int64) * (whole["chromEnd"] - whole["chromStart"])).sum()) \
        == 1147017

    # the oracle on that frame
    d = tmp_path / "oracle"
    d.mkdir(parents=True)
    bg = str(d / "coverage.bedGraph")
    psd.writeBedGraph(frame, bg)
    assert oracle_det.solve(bg, "100") == 0
    oracle = pd.read_csv(bg + "_penalty=100_segments.bed", sep="\t", header=None,
                         names=psd.col_name_list["segments"], na_filter=False,
                         float_precision="round_trip")
    fit = got[0][0]
    assert fit.segments.equals(oracle), "the oracle's segments"
    assert list(fit.segments.dtypes) == list(oracle.dtypes)
    loss = gd.read_loss(bg + "_penalty=100_loss.tsv").split("\t")
    for j, name in enumerate(psd.col_name_list["loss"]):
        assert float(fit.loss[name].iloc[0]) == float(loss[j]), name


def pileup_ms():
    ms = [ctypes.c_float(), ctypes.c_float()]
    _lib().peakseg_hip_reads_last_pileup_ms(ctypes.byref(ms[0]), ctypes.byref(ms[1]))
    return ms[0].value, ms[1].value


# ---- MI355X ----------------------------------------------------------------------------------

_CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process
sys.path[:0] = [%(root)r, %(tests)r]
import test_gpu_reads as gr
gr.child_main(sys.argv[1], sys.argv[2])
print("reads-child ok")
"""


def run_child(which, tmp_path, timeout):
    import sys
    from conftest import ROOT
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code, which, str(tmp_path)], capture_output=True,
                       text=True, timeout=timeout)
    print(p.stdout[-4000:])
    assert p.returncode == 0 and "reads-child ok" in p.stdout, p.stdout[-3000:] + p.stderr[-6000:]


def child_main(which, tmp):
    import pathlib
    import __graft_entry__ as entry
    from conftest import Oracle
    entry.build_hip()
    entry.build_oracle()
    import peaksegdisk_amd as psd
    if which == "pileup":
        scenario_pileup(as_cuda)
        scenario_three_contigs(as_cuda)
        scenario_one_address(as_cuda)
        scenario_long_contig(as_cuda)
        scenario_device_offsets(as_cuda)
        scenario_refusals(as_cuda)
        scenario_python_refusals(psd, as_cuda)
    elif which == "end_to_end":
        scenario_fixture(psd, as_cuda, [WINDOW, (FIXTURE_LO, FIXTURE_HI)])
        scenario_api(psd, as_cuda, pathlib.Path(tmp), Oracle("det"))
    else:
        raise ValueError(which)


@GPU
def test_gpu_reads_pileup_numpy(psd):
    scenario_pileup(as_numpy)
    scenario_three_contigs(as_numpy)
    scenario_one_address(as_numpy)
    print("pile-up of the last call: scatter %.3f ms, scans %.3f ms" % pileup_ms())


@GPU
def test_gpu_reads_long_contig_numpy(psd):
    scenario_long_contig(as_numpy)
    print("pile-up of the last call: scatter %.3f ms, scans %.3f ms" % pileup_ms())


@GPU
def test_gpu_reads_refusals_numpy(psd):
    scenario_refusals(as_numpy)
    scenario_python_refusals(psd, as_numpy)


@GPU
def test_gpu_reads_pileup_and_refusals_cuda_tensors(psd, tmp_path):
    run_child("pileup", tmp_path, 300)


@GPU
def test_gpu_reads_fixture_numpy(psd):
    scenario_fixture(psd, as_numpy, [WINDOW, (FIXTURE_LO, FIXTURE_HI)])


@GPU
def test_gpu_reads_api_and_oracle_numpy(psd, tmp_path, oracle_det):
    scenario_api(psd, as_numpy, tmp_path, oracle_det)


@GPU
def test_gpu_reads_end_to_end_cuda_tensors(psd, tmp_path):
    run_child("end_to_end", tmp_path, 300)
