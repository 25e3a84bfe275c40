"""ProblemSet.region_stats: bases, sum and maximum of caller-chosen regions, computed on the device
from the resident runs.

The scenario functions are shared with the emulator rehearsal (tests/test_regions_emu.py), which
runs them without a GPU on host arrays; the tests marked gpu run them on the MI355X with the regions
once as numpy arrays (in this process) and once as cuda tensors (in a child process that imports
torch first, as tests/test_gpu_dense.py does).

The yardstick is consensus_ref.region_ref(): a slice of the per-base vector.  Integer arithmetic, so
the comparisons are for equality.  The contigs have at most three tiles of runs and are built run by
run, so that the regions can aim at run ends, at the tiles' boundaries and at the threshold between
the regions a thread finishes alone and those that go through the fold.  Two scenarios leave the
sizes at which every loop makes one trip: more work items than three times the fold's grid (read
from the library, not assumed), and more than 65536 regions through the top-level scan."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from consensus_ref import region_ref, region_ref_prefix
from test_gpu_dense import as_cuda, as_numpy, rle

GPU = pytest.mark.gpu


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


def tile_runs():
    return int(_lib().peakseg_hip_region_stats_tile_runs())


# ---- the contigs -----------------------------------------------------------------------------

def runs_vector(rng, n_runs, top=50, widest=4):
    """(count, weight, per-base vector) of n_runs runs: neighbours differ, so the encoder finds
    exactly these runs"""
    count = rng.integers(0, top, n_runs).astype(np.int64)
    same = np.flatnonzero(count[1:] == count[:-1]) + 1
    while len(same):
        count[same] = (count[same] + 1 + rng.integers(0, top - 1, len(same))) % top
        same = np.flatnonzero(count[1:] == count[:-1]) + 1
    weight = rng.integers(1, widest + 1, n_runs).astype(np.int64)
    return count, weight, np.repeat(count, weight).astype(np.int32)


def make_contigs():
    """four contigs: three tiles of runs; a filler that leaves its successor at run offset 3 modulo 4;
    two and a half tiles at that unaligned offset; five runs of counts near 2^31"""
    tile = tile_runs()
    rng = np.random.default_rng(1704)
    contigs = [runs_vector(rng, 3 * tile - 72), runs_vector(rng, tile + 3),
               runs_vector(rng, 2 * tile + tile // 2)]
    big = np.array([2147483647, 2147483600, 2000000000, 7, 2147483646], dtype=np.int64)
    contigs.append((big, np.array([3, 2, 4, 1, 5], dtype=np.int64),
                    np.repeat(big, [3, 2, 4, 1, 5]).astype(np.int32)))
    # the largest count of contigs 0 and 2 in runs of their own, four bases wide: regions cut them
    for c, j in ((0, 700), (2, 1500)):
        count, weight, _ = contigs[c]
        count[j], weight[j] = 1000000, 4
        contigs[c] = (count, weight, np.repeat(count, weight).astype(np.int32))
    offsets = np.concatenate([[0], np.cumsum([len(c[0]) for c in contigs])])[:-1]
    assert [int(o) % 4 for o in offsets[:3]] == [0, 0, 3]
    for count, weight, vector in contigs:
        got = rle(vector)
        assert np.array_equal(got[0], count) and np.array_equal(got[1], weight)
        assert len(count) <= 3 * tile
    return contigs, [int(o) for o in offsets]


FIRSTS = [1000, 0, 123456, 2147483647 - 15]


def aimed_regions(count, weight, first, run_offset, peak_run, rng):
    """the regions of one contig, as (start, end) int32 arrays in shuffled order"""
    tile, small = tile_runs(), 16
    end = np.cumsum(weight)
    start = end - weight
    n, bases = len(count), int(end[-1])
    lead = run_offset % 4
    rows = []

    def runs(j0, j1, cut0=0, cut1=0):     # runs j0 .. j1, less cut0 / cut1 bases at the edges
        rows.append((first + int(start[j0]) + cut0, first + int(end[j1]) - cut1))

    wide = [j for j in range(n) if weight[j] >= 3]
    for j in wide[:3]:
        runs(j, j, 1, 1)                                    # inside one run, both edges cut
    runs(6, 8), runs(11, 40), runs(0, n - 1)                # on run ends; the contig itself
    rows += [(first - 10, first + 5), (first + bases - 7, first + bases + 100),
             (first - 100, first - 1), (first - 50, first), (first + bases, first + bases + 5),
             (first - 3, first + bases + 3)]
    for k in range(1, small + 6):                           # the threshold of the lone thread
        runs(50, 50 + k - 1)
        runs(wide[5], wide[5] + k, 1, 0)
    for boundary in (tile - lead, 2 * tile - lead):         # the first run of tiles 1 and 2
        if boundary + 8 >= n:
            continue
        for d in range(-3, 4):
            runs(2, boundary + d)                           # the span ends around the boundary
            runs(boundary + d, n - 3)                       # ... and begins around it
            runs(boundary + d - 40, boundary + d)
            if weight[boundary + d] >= 2:
                runs(3, boundary + d, 0, 1)
                runs(boundary + d, n - 2, 1, 0)
    runs(100, n - 100)                                      # two tiles and more
    if peak_run is not None:                                # the maximum in a cut edge run
        runs(peak_run, peak_run + 40, 2, 0)
        runs(peak_run - 40, peak_run, 0, 3)
        runs(peak_run, peak_run + 3, 3, 0)
        runs(peak_run - 30, peak_run - 1), runs(peak_run + 1, peak_run + 30)   # ... and just outside
    rows += [rows[4], rows[4], rows[7]]                     # identical
    runs(200, 900), runs(300, 800), runs(400, 700), runs(450, 451)            # nested
    for _ in range(150):
        a = int(rng.integers(-20, bases + 10))
        rows.append((first + a, first + a + int(rng.integers(1, bases // 2))))
    order = rng.permutation(len(rows))
    cols = np.array(rows, dtype=np.int64)[order]
    assert np.all(cols[:, 0] < cols[:, 1]) and np.all(cols < 2 ** 31)
    return as_numpy(cols[:, 0]), as_numpy(cols[:, 1])


def wrap_regions(regions, wrap):
    return [None if e is None else tuple(wrap(a) for a in e) for e in regions]


def check_regions(pset, contigs, regions, firsts, wrap, what="", ref=region_ref):
    got = pset.region_stats(wrap_regions(regions, wrap), first_chromStart=firsts)
    assert len(got) == len(contigs)
    for c, (entry, (_, _, vector)) in enumerate(zip(regions, contigs)):
        starts, ends = entry if entry is not None else (np.zeros(0, np.int32),) * 2
        want = ref(vector, 0 if firsts is None else firsts[c], starts, ends)
        for name, w, dt in zip(("bases", "sum", "max"), want, (np.int32, np.int64, np.int32)):
            g = got[c][name]
            assert g.dtype == dt and len(g) == len(starts), (what, c, name)
            bad = np.flatnonzero(g != w)
            assert len(bad) == 0, (what, c, name, bad[:5].tolist(), g[bad[:5]].tolist(),
                                   w[bad[:5]].tolist(), starts[bad[:5]].tolist(), ends[bad[:5]].tolist())
    return got


# ---- scenario 1: aimed regions on an unsolved and on a solved set ----------------------------

def scenario_aimed(psd, wrap):
    contigs, offsets = make_contigs()
    rng = np.random.default_rng(8)
    regions = [aimed_regions(*contigs[0][:2], FIRSTS[0], offsets[0], 700, rng), None,
               aimed_regions(*contigs[2][:2], FIRSTS[2], offsets[2], 1500, rng)]
    last = FIRSTS[3]                        # the contig of counts near 2^31, up to coordinate 2^31 - 1
    regions.append((as_numpy([last, last + 1, last - 5, last + 3, last + 14]),
                    as_numpy([last + 15, last + 4, last + 2, last + 9, last + 15])))
    pset = psd.ProblemSet.from_dense([as_numpy(c[2]) for c in contigs],
                                     [(0, 5.0), (2, 50.0), (1, float("inf"))])
    try:
        got = check_regions(pset, contigs, regions, FIRSTS, wrap, "unsolved")
        assert got[3]["sum"][0] > 2 ** 32 and got[3]["max"][0] == 2147483647
        assert len(got[1]["bases"]) == 0
        # what the scenario is for did occur: a maximum that sits in a cut edge run, and nothing outside
        assert np.sum(got[0]["max"] == 1000000) >= 4 and np.sum(got[2]["max"] == 1000000) >= 4
        assert np.sum(got[0]["bases"] == 0) >= 3
        pset.solve()
        columns_before = pset.segment_columns(first_chromStart=FIRSTS)
        stats_before = pset.segment_stats(first_chromStart=FIRSTS)
        again = check_regions(pset, contigs, regions, FIRSTS, wrap, "solved")
        for a, b in zip(got, again):                          # repeated calls: identical arrays
            assert all(np.array_equal(a[k], b[k]) for k in ("bases", "sum", "max"))
        total = sum(len(r[0]) for r in regions if r is not None)
        kept = [np.empty(total, dt) for dt in (np.int32, np.int64, np.int32)]
        assert _lib().peakseg_hip_problem_set_packed_region_stats_download(
            pset._h, *[a.ctypes.data for a in kept]) == 0
        assert np.array_equal(kept[1], np.concatenate([g["sum"] for g in again]))
        columns_after = pset.segment_columns(first_chromStart=FIRSTS)
        stats_after = pset.segment_stats(first_chromStart=FIRSTS)
        for before, after in ((columns_before, columns_after), (stats_before, stats_after)):
            for x, y in zip(before, after):
                assert all(np.array_equal(p, q) for p, q in zip(x, y))
        # without first_chromStart the contigs begin at 0
        zero = [None if r is None else (as_numpy(r[0].astype(np.int64) - f), as_numpy(r[1].astype(np.int64) - f))
                for r, f in zip(regions[:3], FIRSTS)] + [None]
        check_regions(pset, contigs, zero, None, wrap, "no first")
        ms = ctypes.c_float(-1.0)
        assert _lib().peakseg_hip_region_stats_last_ms(ctypes.byref(ms)) == 0 and ms.value >= 0.0
    finally:
        pset.close()


# ---- scenario 2: very many small regions, and one region per contig --------------------------

def scenario_many_small(psd, wrap):
    """a region per window of one to three runs (more than one workgroup of them), and the contig as
    one region"""
    tile = tile_runs()
    rng = np.random.default_rng(3)
    contigs = [runs_vector(rng, 2 * tile + 100), runs_vector(rng, 777)]
    regions = []
    for count, weight, _ in contigs:
        end = np.cumsum(weight)
        start = end - weight
        width = rng.integers(1, 4, len(count))
        last = np.minimum(np.arange(len(count)) + width - 1, len(count) - 1)
        regions.append((as_numpy(start), as_numpy(end[last])))
    pset = psd.ProblemSet.from_dense([as_numpy(c[2]) for c in contigs], [(0, 1.0)])
    try:
        check_regions(pset, contigs, regions, None, wrap, "windows")
        whole = [(as_numpy([0]), as_numpy([len(c[2])])) for c in contigs]
        got = check_regions(pset, contigs, whole, None, wrap, "whole")
        assert got[0]["sum"][0] == int(contigs[0][2].astype(np.int64).sum())
    finally:
        pset.close()


# ---- scenarios 3 and 4: past one trip of the fold, past one trip of the top-level scan -------

SMALL = 16      # region_stats.h: a region of at most this many runs is its thread's alone


def fold_grid():
    return int(_lib().peakseg_hip_region_stats_last_fold_grid())


def region_tiles(weight, first, run_offset, starts, ends):
    """the (region, tile) items of every region of one contig, by the header's formula: j0 the first
    run that ends after a, j1 the first that ends at or after b; at most SMALL runs: none; else the
    tiles of the contig's 16-byte aligned range that the whole runs j0 + 1 .. j1 - 1 meet"""
    tile = tile_runs()
    run_end = np.cumsum(weight)
    a = np.maximum(np.asarray(starts, np.int64) - first, 0)
    b = np.minimum(np.asarray(ends, np.int64) - first, int(run_end[-1]))
    j0 = np.searchsorted(run_end, a, side="right")
    j1 = np.minimum(np.searchsorted(run_end, b, side="left"), len(run_end) - 1)
    lead = run_offset % 4
    tiles = (j1 - 1 + lead) // tile - (j0 + 1 + lead) // tile + 1
    return np.where((b > a) & (j1 - j0 >= SMALL), tiles, 0).astype(np.int64)


def run_regions(weight, first, j0, j1):
    """the regions that are exactly the runs j0[i] .. j1[i] of a contig"""
    end = np.cumsum(weight)
    return first + (end - weight)[j0], first + end[j1]


def long_regions(rng, n_runs, n):
    """n spans of more than SMALL runs: a third within a tile's worth, the rest of any length"""
    tile = tile_runs()
    length = np.where(rng.random(n) < 0.33, rng.integers(SMALL + 1, tile // 2, n),
                      rng.integers(SMALL + 1, n_runs, n))
    j0 = (rng.random(n) * (n_runs - length)).astype(np.int64)
    return j0, j0 + length - 1


def two_contigs():
    """contigs 0 and 2 of make_contigs(): three tiles of runs, and two and a half tiles at run offset
    3 modulo 4; -> (contigs, offsets, the indices of the two)"""
    contigs, offsets = make_contigs()
    assert offsets[0] % 4 == 0 and offsets[2] % 4 == 3
    return contigs, offsets, (0, 2)


def packed(regions):
    """the regions of a call in the order of the packed columns: contig after contig"""
    return [r for r in regions if r is not None]


def scenario_fold_trips(psd, wrap):
    """More (region, tile) items than three times the fold's grid, and no multiple of it: every
    workgroup makes three or four trips through its loop, the last of them partial, and a region's
    tiles go to workgroups in different trips."""
    contigs, offsets, use = two_contigs()
    pset = psd.ProblemSet.from_dense([as_numpy(c[2]) for c in contigs], [(0, 5.0)])
    try:
        # the grid of this device: a call whose bound on the items (regions x tiles of the contig,
        # 16384 x 3) is far above eight workgroups per compute unit, so that the grid is the device's
        count, weight, _ = contigs[0]
        at = np.arange(16384) % len(count)
        dry = [None] * len(contigs)
        dry[0] = tuple(as_numpy(x) for x in run_regions(weight, FIRSTS[0], at, at))
        check_regions(pset, contigs, dry, FIRSTS, wrap, "dry", region_ref_prefix)
        grid = fold_grid()
        assert 0 < grid < 16384 and grid % 8 == 0, grid
        rng = np.random.default_rng(77)
        want_items = 3 * grid + grid // 3 + 1
        rows = {c: [] for c in use}
        for c in use:
            count, weight, _ = contigs[c]
            n, first, bases = len(count), FIRSTS[c], int(weight.sum())
            j0, j1 = long_regions(rng, n, want_items // 6)
            s, e = run_regions(weight, first, j0, j1)
            cut = rng.integers(0, 2, (2, len(s)))                       # some edges cut a run
            s = s + cut[0] * (weight[j0] > 1)
            e = e - cut[1] * (weight[j1] > 1)
            rows[c] += list(zip(s.tolist(), e.tolist()))
            k0 = rng.integers(0, n - 3, len(s) // 3)                    # small ones between them
            s, e = run_regions(weight, first, k0, k0 + rng.integers(0, 3, len(k0)))
            rows[c] += list(zip(s.tolist(), e.tolist()))
            for _ in range(len(k0) // 2):                               # ... and regions of no base
                a = int(rng.integers(1, 500))
                rows[c].append((first - a - 40, first - a) if a % 2 else
                               (first + bases + a, first + bases + a + 40))
            rows[c] += [rows[c][int(i)] for i in rng.integers(0, want_items // 6, 120)]   # repeated
        # top up with regions of one item each until the count is what was aimed at
        def build():
            out = [None] * len(contigs)
            for c in use:
                cols = np.array(rows[c], dtype=np.int64)
                order = np.random.default_rng(5 + c).permutation(len(cols))
                out[c] = (as_numpy(cols[order, 0]), as_numpy(cols[order, 1]))
            return out

        def items_of(regions):
            return [region_tiles(contigs[c][1], FIRSTS[c], offsets[c], *regions[c]) for c in use]
        regions = build()
        items = int(sum(t.sum() for t in items_of(regions)))
        assert items < want_items, (items, want_items)
        count, weight, _ = contigs[2]
        for k in range(want_items - items):
            j0 = 40 + 7 * (k % 100)
            s, e = run_regions(weight, FIRSTS[2], np.array([j0]), np.array([j0 + SMALL + 3 + k % 50]))
            rows[2].append((int(s[0]), int(e[0])))
        regions = build()
        tiles = np.concatenate(items_of(regions))
        items = int(tiles.sum())
        # what the scenario is for did occur, from its own inputs
        print("fold grid", grid, "items", items, "regions", len(tiles))
        assert items >= 3 * grid and items % grid != 0, (items, grid)
        assert np.sum(tiles == 1) > 100 and np.sum(tiles == 2) > 100 and np.sum(tiles == 3) > 100
        blocks = [tiles[k:k + 256] for k in range(0, len(tiles), 256)]
        gaps = 0
        for block in blocks:                        # off[]: zeros between non-zero entries of a block
            nz = np.flatnonzero(block)
            gaps += len(nz) > 1 and int(np.sum(block[nz[0]:nz[-1]] == 0)) > 0
        assert gaps == len(blocks), (gaps, len(blocks))
        item0 = np.cumsum(tiles) - tiles            # a region's first item; its trip: item // grid
        flat = np.concatenate([np.stack([np.full(len(r[0]), c), r[0], r[1]], axis=1)
                               for c, r in enumerate(regions) if r is not None])
        _, inverse = np.unique(flat, axis=0, return_inverse=True)
        inverse = inverse.reshape(-1)
        other_trip = 0
        for k in np.flatnonzero(np.bincount(inverse) > 1):
            same = np.flatnonzero((inverse == k) & (tiles > 0))
            other_trip += len(set((item0[same] // grid).tolist())) > 1
        assert other_trip >= 20, other_trip         # equal regions whose items differ in their trip
        got = check_regions(pset, contigs, regions, FIRSTS, wrap, "fold trips")
        assert fold_grid() == grid
        assert np.sum(got[0]["bases"] == 0) > 50 and np.sum(got[2]["max"] == 1000000) > 50
    finally:
        pset.close()


N_SCAN_TOP = 773 * 256 + 57     # more than 3 x 65536 + 1000: 774 blocks, 4 to a thread, the last 2


def scenario_scan_top(psd, wrap):
    """More than 65536 regions, so that a thread of the top-level scan has several blocks: windows of
    one to three runs, and a few hundred long regions, whose work items hang on the prefix sums
    across the threads' shares and within them."""
    contigs, offsets, use = two_contigs()
    n = N_SCAN_TOP
    n_blocks = (n + 255) // 256
    per = (n_blocks + 255) // 256
    assert n >= 3 * 65536 + 1000 and n_blocks > 256 and per == 4 and n_blocks % per != 0
    rng = np.random.default_rng(78)
    n_first = n // 2 + 31                                   # contig 0's regions come first
    contig_of = np.where(np.arange(n) < n_first, use[0], use[1])
    is_long = np.zeros(n, bool)
    is_long[rng.choice(n, 300, replace=False)] = True
    forced = [5, n - 3, 8 * 256 + 7, 9 * 256 + 100]         # first block, last block, two blocks of thread 2
    assert forced[2] // 256 // per == forced[3] // 256 // per and forced[3] // 256 == forced[2] // 256 + 1
    is_long[forced] = True
    regions = [None] * len(contigs)
    tiles = []
    for c in use:
        count, weight, _ = contigs[c]
        mine = np.flatnonzero(contig_of == c)
        j0 = rng.integers(0, len(count) - 3, len(mine))
        j1 = j0 + rng.integers(0, 3, len(mine))
        lj0, lj1 = long_regions(rng, len(count), len(mine))
        far = is_long[mine]
        j0, j1 = np.where(far, lj0, j0), np.where(far, lj1, j1)
        s, e = run_regions(weight, FIRSTS[c], j0, j1)
        regions[c] = (as_numpy(s), as_numpy(e))
        tiles.append(region_tiles(weight, FIRSTS[c], offsets[c], s, e))
    tiles = np.concatenate(tiles)
    # what the scenario is for did occur
    assert len(tiles) == n and np.all(tiles[forced] > 0) and np.sum(tiles > 0) >= 300
    assert np.sum(tiles == 0) > n - 400
    by_block = np.add.reduceat(tiles, np.arange(0, n, 256))
    assert len(by_block) == n_blocks > 256 and np.sum(by_block > 0) > 100 and np.sum(by_block == 0) > 100
    share = np.add.reduceat(by_block, np.arange(0, n_blocks, per))
    assert np.sum(share > 0) > 50 and share[-1] > 0 and len(share) < 256
    pset = psd.ProblemSet.from_dense([as_numpy(c[2]) for c in contigs], [(0, 5.0)])
    try:
        check_regions(pset, contigs, regions, FIRSTS, wrap, "scan top", region_ref_prefix)
    finally:
        pset.close()
    for c in use:                                           # the yardstick of this size against the slices
        pick = rng.choice(len(regions[c][0]), 2000, replace=False)
        s, e = regions[c][0][pick], regions[c][1][pick]
        for x, y in zip(region_ref_prefix(contigs[c][2], FIRSTS[c], s, e), region_ref(contigs[c][2], FIRSTS[c], s, e)):
            assert np.array_equal(x, y)


SCENARIOS = [scenario_aimed, scenario_many_small, scenario_fold_trips, scenario_scan_top]


# ---- scenario 5: refusals --------------------------------------------------------------------

def raw_pack(pset, n_regions, arrays, on_device):
    """the C entry as it is: arrays[c] = two addresses; -> its return value"""
    nc = len(n_regions)
    out = [ctypes.c_void_p() for _ in range(3)]
    cols = [(ctypes.c_void_p * nc)(*[arrays[c][j] for c in range(nc)]) for j in range(2)]
    return _lib().peakseg_hip_problem_set_pack_region_stats(
        pset._h, None, (ctypes.c_longlong * nc)(*n_regions), *cols, on_device, None,
        *[ctypes.byref(q) for q in out])


def scenario_refusals(psd, wrap, device_side):
    """device_side(array) -> (address the library may read as device memory, what keeps it alive),
    or None where there is no such memory at hand"""
    from peaksegdisk_amd import _native
    assert _native.ERROR_REGION_ARGUMENTS == 22
    text = _native.status_message(22, "f", "1", "d")
    assert text.startswith("error code 22") and "chromStart >= chromEnd" in text
    rng = np.random.default_rng(5)
    contigs = [runs_vector(rng, 300), runs_vector(rng, 200)]
    good = (as_numpy([5, 50]), as_numpy([8, 90]))
    bad_cases = [("equal", (as_numpy([5, 9, 30]), as_numpy([8, 9, 40])), "region 1"),
                 ("reversed", (as_numpy([5, 9, 30, 2]), as_numpy([8, 19, 29, 1])), "region 2")]
    pset = psd.ProblemSet.from_dense([as_numpy(c[2]) for c in contigs], [(0, 1.0), (1, 1.0)])
    try:
        sides = [0] + ([1] if device_side is not None else [])
        for on_device in sides:
            def address(a):
                return (a.ctypes.data, a) if not on_device else device_side(a)
            keep = [address(a) for a in good]
            assert raw_pack(pset, [2, 2], [[k[0] for k in keep]] * 2, on_device) == 4
            for name, entry, needle in bad_cases:
                bad = [address(a) for a in entry]
                st = raw_pack(pset, [2, len(entry[0])], [[k[0] for k in keep], [k[0] for k in bad]],
                              on_device)
                message = _lib().peakseg_hip_last_error().decode()
                assert st == -22, (name, on_device, st, message)
                assert "contig 1" in message and needle in message, (name, on_device, message)
                out = [np.zeros(8, dt) for dt in (np.int32, np.int64, np.int32)]   # nothing packed
                assert _lib().peakseg_hip_problem_set_packed_region_stats_download(
                    pset._h, *[a.ctypes.data for a in out]) == -1
            st = raw_pack(pset, [2, -1], [[k[0] for k in keep], (0, 0)], on_device)
            assert st == -22 and "contig 1" in _lib().peakseg_hip_last_error().decode()
            st = raw_pack(pset, [2, 2], [[k[0] for k in keep], (keep[0][0], 0)], on_device)
            assert st == -22 and "NULL" in _lib().peakseg_hip_last_error().decode()
            if on_device:   # an address that is no multiple of 4
                st = raw_pack(pset, [2, 0], [(keep[0][0] + 2, keep[1][0]), (0, 0)], 1)
                assert st == -22 and "multiple of 4" in _lib().peakseg_hip_last_error().decode()
        # the Python entry names the status and checks the shapes itself
        with pytest.raises(RuntimeError, match="region 1") as ei:
            pset.region_stats(wrap_regions([good, bad_cases[0][1]], wrap))
        assert ei.value.status == 22
        with pytest.raises(ValueError, match="one entry per contig"):
            pset.region_stats([good])
        with pytest.raises(ValueError, match="2 chromStart and 3 chromEnd"):
            pset.region_stats([good, (good[0], bad_cases[0][1][1])])
        with pytest.raises(ValueError, match="int32"):
            pset.region_stats([good, (good[0].astype(np.int64), good[1])])
        with pytest.raises(RuntimeError, match="32-bit"):
            pset.region_stats([good, good], first_chromStart=[0, 2147483647 - 10])
        check_regions(pset, contigs, [good, good], None, wrap, "after")   # the set still answers
    finally:
        pset.close()
    count, weight, _ = rle(contigs[1][2])
    plain = psd.ProblemSet([(count, weight)], [(0, 1.0)])
    try:
        with pytest.raises(RuntimeError, match="dense") as ei:
            plain.region_stats([good])
        assert ei.value.status == _native.ERROR_DEVICE_SOLVER     # (the entry returned -1)
        out = [ctypes.c_void_p() for _ in range(3)]
        ptrs = [(ctypes.c_void_p * 1)(a.ctypes.data) for a in good]
        assert _lib().peakseg_hip_problem_set_pack_region_stats(
            plain._h, None, (ctypes.c_longlong * 1)(2), *ptrs, 0, None,
            *[ctypes.byref(q) for q in out]) == -1
    finally:
        plain.close()


# ---- scenario 6: the torch_device form (GPU only) --------------------------------------------

def scenario_torch_device(psd, wrap):
    """the tensors alias the packed buffers and hold what the download returns"""
    import torch
    rng = np.random.default_rng(9)
    contigs = [runs_vector(rng, 1500), runs_vector(rng, 40)]
    regions = [(as_numpy([0, 10, 300]), as_numpy([len(contigs[0][2]), 11, 2000])),
               (as_numpy([-5]), as_numpy([30]))]
    pset = psd.ProblemSet.from_dense([as_numpy(c[2]) for c in contigs], [(0, 1.0)])
    try:
        want = check_regions(pset, contigs, regions, None, wrap, "torch")
        offs, bases, total, largest = pset.region_stats(wrap_regions(regions, wrap),
                                                        torch_device="cuda:0")
        assert offs.tolist() == [0, 3, 4]
        assert [t.dtype for t in (bases, total, largest)] == [torch.int32, torch.int64, torch.int32]
        assert bases.device.type == "cuda"
        kept = [t.cpu().numpy() for t in (bases, total, largest)]
        addresses = [t.data_ptr() for t in (bases, total, largest)]
        again = pset.region_stats(wrap_regions(regions, wrap), torch_device="cuda:0")
        assert [t.data_ptr() for t in again[1:]] == addresses      # the library's own buffers
    finally:
        pset.close()
    for name, got in zip(("bases", "sum", "max"), kept):
        assert np.array_equal(got, np.concatenate([w[name] for w in want]))


# ---- MI355X ----------------------------------------------------------------------------------

def cuda_side(a):
    t = as_cuda(a)
    return t.data_ptr(), t


_CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process
sys.path[:0] = [%(root)r, %(tests)r]
import test_gpu_regions as gr
gr.child_main()
print("regions-child ok")
"""


def child_main():
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd as psd
    for scenario in SCENARIOS:
        scenario(psd, as_cuda)
    scenario_refusals(psd, as_cuda, cuda_side)
    scenario_torch_device(psd, as_cuda)
    scenario_torch_device(psd, as_numpy)


@GPU
@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__[len("scenario_"):])
def test_gpu_regions_numpy(psd, scenario):
    scenario(psd, as_numpy)


@GPU
def test_gpu_regions_refusals_host_arrays(psd):
    scenario_refusals(psd, as_numpy, None)


@GPU
def test_gpu_regions_cuda_tensors(psd):
    """every scenario again with the regions in cuda tensors read in place, the refusals of device
    arrays, and the torch_device form of region_stats()"""
    import sys
    from conftest import ROOT
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(p.stdout[-4000:])
    assert p.returncode == 0 and "regions-child ok" in p.stdout, p.stdout[-3000:] + p.stderr[-6000:]
