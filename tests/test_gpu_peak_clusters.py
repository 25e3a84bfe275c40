"""ProblemSet.peak_clusters: the clusters of overlapping peaks over the members of a group and the
cluster-by-member matrix, computed on the device from the resident tables.

The scenario functions are shared with the emulator rehearsal (tests/test_peak_clusters_emu.py).
The probe scenarios hand the cluster kernels peak lists that no small solve yields; the solve
scenarios go through whole sets, and first assert from the models' own segments that the
configuration they are about (peaks that abut across samples, nested peaks, a chain, a cluster that
hangs over a member's end, a member without peaks, two members on one contig) did occur.

The yardsticks are consensus_ref.cluster_ref() -- a plain sorted sweep -- and
consensus_ref.region_ref() -- a slice of the per-base vector.  Integer arithmetic: equality."""
import ctypes
import os

import numpy as np
import pytest

from consensus_ref import cluster_ref, cluster_ref_sorted, region_ref
from test_gpu_dense import as_cuda, as_numpy

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


# ---- the probe -------------------------------------------------------------------------------

def probe(members):
    """members: a list of (peak_start, peak_end); -> (status or clusters, table [k, 4], m_peaks [k, m])"""
    m = len(members)
    keep = [(as_numpy(ps), as_numpy(pe)) for ps, pe in members]
    total = sum(len(ps) for ps, _ in keep)
    cols = [np.full(max(total, 1), -7, np.int32) for _ in range(4)]
    m_peaks = np.full(max(total * m, 1), -7, np.int32)
    k = _lib().peakseg_hip_peak_clusters_probe(
        0, m, (ctypes.c_longlong * max(m, 1))(*[len(ps) for ps, _ in keep]),
        (ctypes.c_void_p * max(m, 1))(*[ps.ctypes.data if len(ps) else 0 for ps, _ in keep]),
        (ctypes.c_void_p * max(m, 1))(*[pe.ctypes.data if len(pe) else 0 for _, pe in keep]),
        *[a.ctypes.data for a in cols], m_peaks.ctypes.data)
    if k < 0:
        return int(k), None, None
    return int(k), np.stack([a[:k] for a in cols], axis=1).astype(np.int64), \
        m_peaks[:k * m].reshape(k, m).astype(np.int64)


def check_probe(members, what, ref=cluster_ref):
    k, table, m_peaks = probe(members)
    want_table, want_peaks = ref(members)
    assert k == len(want_table), (what, k, len(want_table), _lib().peakseg_hip_last_error().decode())
    assert np.array_equal(table, want_table), (what, table[:8].tolist(), want_table[:8].tolist())
    assert np.array_equal(m_peaks, want_peaks), what
    return table, m_peaks


def random_peaks(rng, n, lo, hi):
    """n sorted disjoint peaks in [lo, hi); neighbours may abut"""
    cuts = np.sort(rng.choice(np.arange(lo, hi), size=2 * n, replace=False))
    start, end = cuts[0::2].copy(), cuts[1::2].copy()
    glue = rng.random(n - 1) < 0.1                 # some peaks end where the next begins
    end[:-1][glue] = start[1:][glue]
    return start, end


def scenario_probe_small(psd, wrap):
    none = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert probe([])[0] == 0                                                    # an empty group
    table, _ = check_probe([([10, 30, 50], [20, 40, 60])], "one member")
    assert len(table) == 3
    table, m_peaks = check_probe([([10], [20]), none, ([15], [30])], "a member without peaks")
    assert table.tolist() == [[10, 30, 2, 2]] and m_peaks.tolist() == [[1, 0, 1]]
    assert probe([none, none])[0] == 0
    table, _ = check_probe([([10], [20]), ([20], [30])], "abutting")
    assert table.tolist() == [[10, 20, 1, 1], [20, 30, 1, 1]]
    table, _ = check_probe([([10, 20], [20, 30]), ([5], [10])], "abutting within and across")
    assert len(table) == 3
    table, _ = check_probe([([10], [20]), ([10], [20]), ([40], [50])], "identical")
    assert table.tolist() == [[10, 20, 2, 2], [40, 50, 1, 1]]
    table, _ = check_probe([([10], [100]), ([20, 40, 60], [30, 50, 70]), ([45], [46])], "nested")
    assert table.tolist() == [[10, 100, 5, 3]]
    table, m_peaks = check_probe([([10], [20]), ([18], [32]), ([30], [40])], "chain")
    assert table.tolist() == [[10, 40, 3, 3]]
    table, _ = check_probe([([10, 19], [19, 30]), ([19], [25])], "equal start after an abutting end")
    assert table.tolist() == [[10, 19, 1, 1], [19, 30, 2, 2]]
    top = 2 ** 31 - 1
    table, _ = check_probe([([top - 100, top - 40], [top - 50, top]), ([top - 60], [top - 45]),
                            ([0], [1])], "coordinates near 2^31 - 1")
    assert table.tolist() == [[0, 1, 1, 1], [top - 100, top - 45, 2, 2], [top - 40, top, 1, 1]]
    # repeated calls: identical arrays
    members = [([10, 50], [20, 60]), ([15, 55], [30, 58])]
    first, again = probe(members), probe(members)
    assert first[0] == again[0] and all(np.array_equal(a, b) for a, b in zip(first[1:], again[1:]))


def scenario_probe_wide(psd, wrap):
    """a cluster that joins peaks of all of 65 and of 257 members: across a wave and a workgroup"""
    for m in (65, 257):
        members = []
        for k in range(m):
            ps, pe = [5 + k % 3, 1000 + 2 * k, 90000 + 10 * k], [9 + k % 3, 1003 + 2 * k, 90005 + 10 * k]
            if k % 7 == 0:
                ps.append(200000 + k), pe.append(200001 + k)
            members.append((ps, pe))
        table, m_peaks = check_probe(members, "%d members" % m)
        assert [m, m] in table[:, 2:].tolist()                  # every member in one cluster
        assert np.sum(table[:, 3] == 1) >= m                    # ... and clusters of one


def scenario_probe_random(psd, wrap):
    """3 members x about 3000 random peaks: many workgroups, every kind of contact by chance"""
    rng = np.random.default_rng(41)
    members = [random_peaks(rng, n, 0, 60000) for n in (3000, 2900, 3100)]
    table, m_peaks = check_probe(members, "random")
    assert len(table) > 256 and table[:, 2].max() >= 4 and (m_peaks == 0).any()
    sparse = [random_peaks(rng, n, 0, 2000000) for n in (3000, 50, 1)]
    table, _ = check_probe(sparse, "sparse")
    assert np.sum(table[:, 3] == 1) >= 1000      # (the 50 wide peaks of the second member join the rest)


def sparse_peaks(rng, n, hi, widest):
    """n sorted disjoint peaks of 1 to `widest` bases scattered over [0, hi): a peak that would reach
    into the next one ends where that begins"""
    start = np.unique(rng.integers(0, hi - widest, n + n // 8))
    assert len(start) >= n
    start = np.sort(rng.choice(start, n, replace=False))
    end = start + rng.integers(1, widest + 1, n)
    end[:-1] = np.minimum(end[:-1], start[1:])
    return start, end


def scenario_probe_scan_top(psd, wrap):
    """More than 2 x 65536 peaks in the members of one group (the probe takes one group per call;
    two calls with different member counts): mark_kernel runs more than 256 workgroups, so a thread
    of the top-level scan of the lead flags has several blocks, and a peak's cluster index hangs on
    the prefix sums across the threads' shares."""
    rng = np.random.default_rng(43)
    for sizes in ((50000, 45000, 40300), (70000, 66000)):
        n = sum(sizes)
        n_blocks = (n + 1 + 255) // 256             # (an entry more than peaks: "all of them")
        per = (n_blocks + 255) // 256
        assert n > 2 * 65536 and n_blocks > 256 and per == 3 and n_blocks % per != 0, (n, n_blocks)
        members = [sparse_peaks(rng, k, 60000000, 300) for k in sizes]
        table, m_peaks = check_probe(members, "%d peaks" % n, cluster_ref_sorted)
        # lead flags of both kinds in every block: a cluster per lead, fewer clusters than peaks,
        # and in every stretch of 256 peaks of a member one that leads and one that does not
        assert n // 2 < len(table) < n - n // 20, (n, len(table))
        leads = np.concatenate([np.isin(ps, table[:, 0]) for ps, _ in members])
        by_block = np.add.reduceat(leads.astype(np.int64), np.arange(0, n, 256))
        assert by_block[:-1].min() > 0 and by_block[:-1].max() < 256
        assert table[:, 2].max() >= 3 and (m_peaks == 0).any() and (table[:, 3] == len(sizes)).any()
    # the yardstick of this size against the sweep, on a part cluster_ref() can afford
    part = [(ps[:700], pe[:700]) for ps, pe in members]
    for x, y in zip(cluster_ref_sorted(part), cluster_ref(part)):
        assert np.array_equal(x, y)


def scenario_probe_refusals(psd, wrap):
    for members, needle in (([([10, 15], [20, 30])], "member 0"), ([([1], [5]), ([7], [7])], "member 1"),
                            ([([-4], [5])], "member 0")):
        k, _, _ = probe(members)
        assert k == -22 and needle in _lib().peakseg_hip_last_error().decode()


# ---- whole sets ------------------------------------------------------------------------------

def steps(length, first, bumps, ripple=()):
    """step-function coverage: 2 everywhere, and (start, end, height) bumps in genomic coordinates;
    a bump in `ripple` alternates height, height + 1 from base to base: a run per base"""
    v = np.full(length, 2, dtype=np.int32)
    for k, (a, b, h) in enumerate(bumps):
        v[a - first:b - first] = h
        if k in ripple:
            v[a - first + 1:b - first:2] = h + 1
    return v


#            first  length  bumps
SAMPLES = [(1000, 20000, [(2000, 2500, 50), (3000, 3600, 60), (5000, 5400, 50), (8000, 9500, 70),
                          (12000, 12500, 50), (15000, 15100, 4)]),
           (1500, 15000, [(2500, 2800, 40), (3100, 3300, 90), (5300, 5700, 50), (12000, 12500, 30)]),
           (500, 8700, [(700, 900, 30), (5600, 6000, 45), (8500, 9100, 55)]),
           (0, 6000, [(1000, 1400, 50), (3000, 3500, 50)]),
           (200, 5000, [(1300, 1800, 50), (4000, 4100, 80)]),
           (0, 4000, [(1000, 1500, 50)])]
#            contig, penalty
PROBLEMS = [(0, 10.0), (1, 10.0), (2, 10.0), (0, 2000.0), (5, 10.0), (3, 10.0), (4, 10.0),
            (3, float("inf"))]
GROUPS = [0, 0, 0, 0, -1, 1, 1, 1]


def member_peaks(columns):
    """the peaks of a model in increasing coordinates"""
    start, end = np.asarray(columns[0], np.int64), np.asarray(columns[1], np.int64)
    return start[1::2][::-1], end[1::2][::-1]


def check_clusters(pset, vectors, firsts, groups, columns, result, what=""):
    n_groups = max(groups) + 1
    assert len(result) == n_groups
    for g in range(n_groups):
        members = [p for p in range(len(groups)) if groups[p] == g]
        entry = result[g]
        assert entry["members"].tolist() == members
        want_table, want_peaks = cluster_ref([member_peaks(columns[p]) for p in members])
        frame = entry["clusters"]
        assert list(frame.columns) == ["clusterStart", "clusterEnd", "peaks", "samples"]
        assert all(frame[n].dtype == np.int32 for n in frame.columns)
        assert np.array_equal(frame.to_numpy().astype(np.int64).reshape(-1, 4), want_table), (what, g)
        k = len(want_table)
        assert entry["peaks"].shape == (k, len(members)) and entry["peaks"].dtype == np.int32
        assert np.array_equal(entry["peaks"], want_peaks), (what, g)
        assert entry["sum"].dtype == np.int64 and entry["bases"].dtype == entry["max"].dtype == np.int32
        for j, p in enumerate(members):
            c = pset.problems[p][0]
            want = region_ref(vectors[c], firsts[c], want_table[:, 0], want_table[:, 1])
            for name, w in zip(("bases", "sum", "max"), want):
                assert np.array_equal(entry[name][:, j], w), (what, g, p, name,
                                                              entry[name][:, j].tolist(), w.tolist())


def scenario_sets(psd, wrap):
    firsts = [s[0] for s in SAMPLES]
    vectors = [steps(length, first, bumps, ripple=(3,) if c == 0 else ())
               for c, (first, length, bumps) in enumerate(SAMPLES)]
    assert all(len(v) <= 20000 for v in vectors) and 4 <= len(vectors) <= 8
    pset = psd.ProblemSet.from_dense([wrap(v) for v in vectors], PROBLEMS)
    try:
        with pytest.raises(RuntimeError) as ei:                       # not solved
            pset.peak_clusters(GROUPS, first_chromStart=firsts)
        assert ei.value.status == 13
        pset.solve()
        columns = pset.segment_columns(first_chromStart=firsts)
        # the configuration this scenario is about, from the models themselves
        peaks = [list(zip(*(x.tolist() for x in member_peaks(c)))) for c in columns]
        for p, (c, pen) in enumerate(PROBLEMS):
            want = [(a, b) for a, b, h in SAMPLES[c][2]]
            if pen == 2000.0:
                want = want[:-1]                                      # the weak bump is not worth it
            if pen == float("inf"):
                want = []                                             # a trivial model
            assert peaks[p] == want, (p, peaks[p], want)
        assert (2000, 2500) in peaks[0] and (2500, 2800) in peaks[1]          # abut across samples
        assert (3000, 3600) in peaks[0] and (3100, 3300) in peaks[1]          # nested
        assert (5000, 5400) in peaks[0] and (5300, 5700) in peaks[1] and (5600, 6000) in peaks[2]  # chain
        assert (8000, 9500) in peaks[0] and firsts[2] + len(vectors[2]) == 9200   # hangs over the end
        assert PROBLEMS[0][0] == PROBLEMS[3][0] and len(peaks[7]) == 0 and GROUPS[4] == -1
        stats_before = pset.segment_stats(first_chromStart=firsts)
        result = pset.peak_clusters(wrap(GROUPS) if wrap is as_numpy else GROUPS, first_chromStart=firsts)
        check_clusters(pset, vectors, firsts, GROUPS, columns, result, "sets")
        table = result[0]["clusters"]
        assert [2000, 2500, 2, 2] in table.to_numpy().tolist()        # not joined with [2500, 2800)
        assert [5000, 6000, 4, 4] in table.to_numpy().tolist()
        over = table["clusterStart"].tolist().index(8000)
        assert table["clusterEnd"][over] == 9500 and result[0]["bases"][over].tolist() == [1500, 1500, 1200, 1500]
        assert result[0]["bases"][0].tolist() == [0, 0, 200, 0]       # [700, 900): before two firsts
        assert result[1]["peaks"][:, 2].tolist() == [0] * len(result[1]["clusters"])
        assert len(result[0]["clusters"]) != len(result[1]["clusters"])
        again = pset.peak_clusters(GROUPS, first_chromStart=firsts)   # repeated calls: identical arrays
        for a, b in zip(result, again):
            assert a["clusters"].equals(b["clusters"])
            assert all(np.array_equal(a[n], b[n]) for n in ("peaks", "bases", "sum", "max"))
        stats_after = pset.segment_stats(first_chromStart=firsts)
        for x, y in zip(stats_before, stats_after):
            assert all(np.array_equal(p, q) for p, q in zip(x, y))
        # other groupings of the same set: everything in one group; a group that is empty; no group
        for groups in ([0] * 8, [2, 2, 0, 0, -1, -1, 2, 0], [-1] * 8):
            result = pset.peak_clusters(groups, first_chromStart=firsts)
            if max(groups) < 0:
                assert result == []
                continue
            check_clusters(pset, vectors, firsts, groups, columns, result, str(groups))
        assert len(pset.peak_clusters([2, 2, 0, 0, -1, -1, 2, 0], first_chromStart=firsts)[1]["clusters"]) == 0
        ms = ctypes.c_float(-1.0)
        assert _lib().peakseg_hip_peak_clusters_last_ms(ctypes.byref(ms)) == 0 and ms.value >= 0.0
    finally:
        pset.close()


def raw_clusters(pset, n_groups, group):
    out = [ctypes.c_void_p() for _ in range(8)]
    g = as_numpy(group)
    return _lib().peakseg_hip_problem_set_pack_peak_clusters(
        pset._h, None, n_groups, g.ctypes.data if len(g) else None, None, None,
        *[ctypes.byref(q) for q in out])


def nothing_packed(pset):
    out = [np.zeros(64, dt) for dt in (np.int32,) * 6 + (np.int64, np.int32)]
    return _lib().peakseg_hip_problem_set_packed_peak_clusters_download(
        pset._h, *[a.ctypes.data for a in out]) == -1


def scenario_set_refusals(psd, wrap):
    from peaksegdisk_amd import _native
    from test_gpu_dense import rle
    vectors = [steps(length, first, bumps) for first, length, bumps in SAMPLES[3:5]]
    pset = psd.ProblemSet.from_dense([as_numpy(v) for v in vectors], [(0, 10.0), (1, 10.0)])
    try:
        assert raw_clusters(pset, 1, [0, 0]) == -1                     # not solved
        pset.solve()
        assert raw_clusters(pset, 1, [0, 0]) == 3 and not nothing_packed(pset)
        for n_groups, group, needle in ((1, [0, 1], "problem 1"), (2, [-2, 1], "problem 0"),
                                        (-1, [0, 0], "-1 groups")):
            st = raw_clusters(pset, n_groups, group)
            message = _lib().peakseg_hip_last_error().decode()
            assert st == -22 and needle in message, (st, message)
            assert nothing_packed(pset)
        with pytest.raises(RuntimeError, match="problem 0") as ei:
            pset.peak_clusters([-3, 0])
        assert ei.value.status == 22
        with pytest.raises(ValueError, match="one group per problem"):
            pset.peak_clusters([0])
        with pytest.raises(ValueError, match="integers"):
            pset.peak_clusters([0.5, 1])
        with pytest.raises(RuntimeError, match="32-bit"):
            pset.peak_clusters([0, 0], first_chromStart=[0, 2147483647 - 10])
        assert len(pset.peak_clusters([0, 0])[0]["clusters"]) == 3     # the set still answers
        room = pset.hbm_bytes
    finally:
        pset.close()
    count, weight, _ = rle(vectors[0])
    plain = psd.ProblemSet([(count, weight)], [(0, 10.0)])
    try:
        plain.solve()
        with pytest.raises(RuntimeError, match="dense"):
            plain.peak_clusters([0])
        assert raw_clusters(plain, 1, [0]) == -1
    finally:
        plain.close()
    # a matrix that does not fit: the same set again, allowed 8 bytes less than everything it held
    # after its matrix was there
    os.environ["PEAKSEG_HIP_MAX_BYTES"] = str(room - 8)
    try:
        capped = psd.ProblemSet.from_dense([as_numpy(v) for v in vectors], [(0, 10.0), (1, 10.0)])
    finally:
        del os.environ["PEAKSEG_HIP_MAX_BYTES"]
    try:
        capped.solve()
        with pytest.raises(RuntimeError, match="do not fit") as ei:
            capped.peak_clusters([0, 0])
        assert ei.value.status == _native.ERROR_DEVICE_MEMORY == 14
        assert nothing_packed(capped)
    finally:
        capped.close()


def scenario_api(psd, wrap):
    """consensus_peaks_dense and consensus_peaks_reads: samples in, consensus peaks and matrix out"""
    firsts = [s[0] for s in SAMPLES[:3]]
    vectors = [steps(length, first, bumps) for first, length, bumps in SAMPLES[:3]]
    out = psd.consensus_peaks_dense([wrap(v) for v in vectors], penalties=10.0, chrom="chr7",
                                    chrom_starts=firsts)
    assert len(out.groups) == 1 and len(out.fits) == 3
    assert list(out.clusters.columns) == ["chrom", "clusterStart", "clusterEnd", "peaks", "samples"]
    assert set(out.clusters["chrom"]) == {"chr7"} and set(out.fits[1].segments["chrom"]) == {"chr7"}
    members = []
    for fit in out.fits:
        seg = fit.segments[fit.segments["status"] == "peak"]
        members.append((seg["chromStart"].to_numpy()[::-1], seg["chromEnd"].to_numpy()[::-1]))
    want_table, want_peaks = cluster_ref(members)
    assert np.array_equal(out.clusters.iloc[:, 1:].to_numpy().astype(np.int64), want_table)
    assert np.array_equal(out.peaks, want_peaks) and out.groups[0]["samples"].tolist() == [0, 1, 2]
    for j in range(3):
        want = region_ref(vectors[j], firsts[j], want_table[:, 0], want_table[:, 1])
        for name, w in zip(("bases", "sum", "max"), want):
            assert np.array_equal(getattr(out, name)[:, j], w), (j, name)
    two = psd.consensus_peaks_dense([wrap(v) for v in vectors], penalties=[10.0, 10.0, 1e9],
                                    groups=[1, 1, 0], chrom=["chrA", "chrB"], chrom_starts=firsts)
    assert len(two.groups) == 2 and len(two.groups[0]["clusters"]) == 0
    assert two.groups[0]["peaks"].shape == (0, 1) and set(two.groups[1]["clusters"]["chrom"]) == {"chrB"}
    with pytest.raises(ValueError, match="2 groups"):
        two.clusters
    # the same coverage as reads: one read per base and count
    reads = []
    for v, first in zip(vectors, firsts):
        at = np.arange(len(v), dtype=np.int64) + first
        reads.append((as_numpy(at), as_numpy(at + 1), as_numpy(v)))
    from_reads = psd.consensus_peaks_reads([tuple(wrap(a) for a in r) for r in reads], penalties=10.0,
                                           chrom="chr7")
    assert from_reads.clusters.equals(out.clusters)
    assert all(np.array_equal(getattr(from_reads, n), getattr(out, n)) for n in ("peaks", "bases", "sum", "max"))


PROBE_SCENARIOS = [scenario_probe_small, scenario_probe_wide, scenario_probe_random,
                   scenario_probe_scan_top, scenario_probe_refusals]
SET_SCENARIOS = [scenario_sets, scenario_set_refusals, scenario_api]
SCENARIOS = PROBE_SCENARIOS + SET_SCENARIOS


# ---- MI355X ----------------------------------------------------------------------------------

@GPU
@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__[len("scenario_"):])
def test_gpu_peak_clusters(psd, scenario):
    scenario(psd, as_numpy)


_CHILD = r"""
import sys
import torch                      # first: one HIP runtime in the process
sys.path[:0] = [%(root)r, %(tests)r]
import test_gpu_peak_clusters as gc
gc.child_main()
print("clusters-child ok")
"""


def child_main():
    import torch
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd as psd
    scenario_api(psd, as_cuda)
    # the torch_device form: tensors that alias the library's buffers
    firsts = [s[0] for s in SAMPLES]
    vectors = [steps(length, first, bumps) for first, length, bumps in SAMPLES]
    pset = psd.ProblemSet.from_dense([as_cuda(v) for v in vectors], PROBLEMS)
    try:
        pset.solve()
        want = pset.peak_clusters(GROUPS, first_chromStart=firsts)
        out = pset.peak_clusters(GROUPS, first_chromStart=firsts, torch_device="cuda:0")
        c_off, e_off, tensors = out[0], out[1], out[2:]
        assert [t.dtype for t in tensors] == [torch.int32] * 6 + [torch.int64, torch.int32]
        assert c_off.tolist() == [0, len(want[0]["clusters"]), len(want[0]["clusters"]) + len(want[1]["clusters"])]
        kept = [t.cpu().numpy() for t in tensors]
        again = pset.peak_clusters(GROUPS, first_chromStart=firsts, torch_device="cuda:0")
        assert [t.data_ptr() for t in again[2:]] == [t.data_ptr() for t in tensors]
    finally:
        pset.close()
    for g in (0, 1):
        rows, cells = slice(c_off[g], c_off[g + 1]), slice(e_off[g], e_off[g + 1])
        assert np.array_equal(np.stack([a[rows] for a in kept[:4]], axis=1), want[g]["clusters"].to_numpy())
        for a, name in zip(kept[4:], ("peaks", "bases", "sum", "max")):
            assert np.array_equal(a[cells].reshape(want[g][name].shape), want[g][name])


@GPU
def test_gpu_peak_clusters_cuda_tensors(psd):
    """the consensus entries with the samples in cuda tensors, and the torch_device form"""
    import subprocess
    import sys
    from conftest import ROOT
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(p.stdout[-4000:])
    assert p.returncode == 0 and "clusters-child ok" in p.stdout, p.stdout[-3000:] + p.stderr[-6000:]
