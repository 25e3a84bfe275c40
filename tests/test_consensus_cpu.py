"""What region_stats(), peak_clusters() and the consensus entries check without a device: the
symbols, the status, the argument checks of the Python layer (which come before any device work),
and the yardsticks of tests/consensus_ref.py against cases worked by hand."""
import ctypes

import numpy as np
import pytest

from consensus_ref import cluster_ref, region_ref


@pytest.fixture(scope="module")
def psd():
    import __graft_entry__ as entry
    entry.build_hip()
    import peaksegdisk_amd
    return peaksegdisk_amd


def test_symbols_and_status(psd):
    from peaksegdisk_amd import _native as native
    assert native.ERROR_REGION_ARGUMENTS == 22
    for name in ("peakseg_hip_problem_set_pack_region_stats",
                 "peakseg_hip_problem_set_packed_region_stats_download",
                 "peakseg_hip_region_stats_tile_runs", "peakseg_hip_region_stats_last_ms",
                 "peakseg_hip_region_stats_last_fold_grid",
                 "peakseg_hip_problem_set_pack_peak_clusters",
                 "peakseg_hip_problem_set_packed_peak_clusters_download",
                 "peakseg_hip_peak_clusters_last_ms", "peakseg_hip_peak_clusters_probe"):
        assert hasattr(native.lib, name) and name in native.EXPORTED_SYMBOLS
    for name in ("consensus_peaks_dense", "consensus_peaks_reads", "ConsensusPeaks"):
        assert name in psd.__all__ and hasattr(psd, name)
    assert hasattr(psd.ProblemSet, "region_stats") and hasattr(psd.ProblemSet, "peak_clusters")
    text = native.status_message(22, "f", "1", "d")
    assert text.startswith("error code 22") and "group" in text and "region" in text
    assert native.lib.peakseg_hip_region_stats_tile_runs() % 4 == 0
    assert native.lib.peakseg_hip_region_stats_last_fold_grid() >= 0
    ms = ctypes.c_float(-1.0)
    assert native.lib.peakseg_hip_region_stats_last_ms(ctypes.byref(ms)) == 0 and ms.value >= 0.0
    assert native.lib.peakseg_hip_peak_clusters_last_ms(ctypes.byref(ms)) == 0 and ms.value >= 0.0


def test_entries_refuse_without_a_set(psd):
    """the C entries check their arguments before they look for a device"""
    from peaksegdisk_amd import _native as native
    lib = native.lib
    out = [ctypes.c_void_p() for _ in range(8)]
    assert lib.peakseg_hip_problem_set_pack_region_stats(
        None, None, None, None, None, 0, None, *[ctypes.byref(q) for q in out[:3]]) == -1
    assert lib.peakseg_hip_problem_set_pack_peak_clusters(
        None, None, 1, None, None, None, *[ctypes.byref(q) for q in out]) == -1
    assert lib.peakseg_hip_problem_set_packed_region_stats_download(None, None, None, None) == -1
    assert lib.peakseg_hip_problem_set_packed_peak_clusters_download(None, *[None] * 8) == -1
    # the probe checks the lists on the host
    ps, pe = np.array([10, 15], np.int32), np.array([20, 30], np.int32)
    st = lib.peakseg_hip_peak_clusters_probe(
        0, 1, (ctypes.c_longlong * 1)(2), (ctypes.c_void_p * 1)(ps.ctypes.data),
        (ctypes.c_void_p * 1)(pe.ctypes.data), None, None, None, None, None)
    assert st == -22 and "member 0" in native.last_error() and "peak 1" in native.last_error()
    assert lib.peakseg_hip_peak_clusters_probe(0, -1, None, None, None, None, None, None, None, None) == -22


def test_consensus_argument_checks(psd):
    vecs = [np.array([1, 1, 9, 9, 1], np.int32)] * 3
    with pytest.raises(ValueError, match="exactly one of penalties and penalty_model"):
        psd.consensus_peaks_dense(vecs)
    with pytest.raises(ValueError, match="exactly one of penalties and penalty_model"):
        psd.consensus_peaks_dense(vecs, penalties=1.0, penalty_model={"intercept": 0.0, "weights": {}})
    with pytest.raises(ValueError, match="one per sample"):
        psd.consensus_peaks_dense(vecs, penalties=[1.0, 2.0])
    with pytest.raises(ValueError, match="one number per sample"):
        psd.consensus_peaks_dense(vecs, penalties=[[1.0], [2.0], [3.0]])
    with pytest.raises(ValueError):                                   # a penalty that is no penalty
        psd.consensus_peaks_dense(vecs, penalties=[1.0, -2.0, 3.0])
    with pytest.raises(ValueError, match=r"groups: one per sample \(2 values, 3 samples\)"):
        psd.consensus_peaks_dense(vecs, penalties=1.0, groups=[0, 1])
    with pytest.raises(ValueError, match="groups must be integers"):
        psd.consensus_peaks_dense(vecs, penalties=1.0, groups=[0.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="sample 1 is in group -2"):
        psd.consensus_peaks_dense(vecs, penalties=1.0, groups=[0, -2, 1])
    with pytest.raises(ValueError, match=r"chrom: one name, or one per group \(1 names, 2 groups\)"):
        psd.consensus_peaks_dense(vecs, penalties=1.0, groups=[0, 1, 1], chrom=["chr1"])
    with pytest.raises(ValueError, match="chrom.starts: one per sample"):
        psd.consensus_peaks_dense(vecs, penalties=1.0, chrom_starts=[0])
    with pytest.raises(ValueError, match="at least one sample"):
        psd.consensus_peaks_dense([], penalties=1.0)
    with pytest.raises(ValueError, match="a list of vectors"):
        psd.consensus_peaks_dense(vecs[0], penalties=1.0)
    with pytest.raises(ValueError, match="must be integer"):
        psd.consensus_peaks_dense([np.array([1.5, 2.0])], penalties=1.0)
    reads = [(np.array([0, 5], np.int32), np.array([10, 20], np.int32))] * 2
    with pytest.raises(ValueError, match="exactly one of penalties and penalty_model"):
        psd.consensus_peaks_reads(reads)
    with pytest.raises(ValueError, match="one per sample"):
        psd.consensus_peaks_reads(reads, penalties=[1.0])
    with pytest.raises(ValueError, match="a list of samples"):
        psd.consensus_peaks_reads(reads[0], penalties=1.0)
    with pytest.raises(ValueError, match="groups: one per sample"):
        psd.consensus_peaks_reads(reads, penalties=1.0, groups=[0])


def test_consensus_arguments_default_groups(psd):
    from peaksegdisk_amd import api
    pens, groups, chrom = api._consensus_arguments(3, 5.0, None, None, "chrX")
    assert pens == [[5.0]] * 3 and groups.tolist() == [0, 0, 0] and chrom == ["chrX"]
    assert groups.dtype == np.int32
    pens, groups, chrom = api._consensus_arguments(3, [1, 2.5, 3], None, [1, -1, 0], ["a", "b"])
    assert pens == [[1], [2.5], [3]] and groups.tolist() == [1, -1, 0] and chrom == ["a", "b"]
    model = {"intercept": 1.0, "weights": {"log.bases": 0.5}}
    pens, groups, chrom = api._consensus_arguments(2, None, model, [-1, -1], "c")
    assert pens == [[float("inf")]] * 2 and chrom == []
    only = psd.ConsensusPeaks([{"clusters": "t", "peaks": 1, "bases": 2, "sum": 3, "max": 4}], [])
    assert (only.clusters, only.peaks, only.bases, only.sum, only.max) == ("t", 1, 2, 3, 4)
    with pytest.raises(ValueError, match="0 groups"):
        psd.ConsensusPeaks([], []).clusters


def test_region_reference_by_hand():
    #  base   100 101 102 103 104 105
    vector = [3, 3, 7, 7, 7, 1]
    starts = [100, 101, 103, 90, 104, 106, 50, 99, 102]
    ends = [106, 103, 104, 101, 200, 110, 60, 300, 103]
    bases, total, largest = region_ref(vector, 100, starts, ends)
    assert bases.tolist() == [6, 2, 1, 1, 2, 0, 0, 6, 1]
    assert total.tolist() == [28, 10, 7, 3, 8, 0, 0, 28, 7]
    assert largest.tolist() == [7, 7, 7, 3, 7, 0, 0, 7, 7]
    assert bases.dtype == np.int32 and total.dtype == np.int64 and largest.dtype == np.int32
    big = region_ref([2147483647] * 3, 0, [0], [3])
    assert big[1].tolist() == [3 * 2147483647] and big[2].tolist() == [2147483647]


def test_cluster_reference_by_hand():
    a = ([10, 30, 60], [20, 40, 70])
    b = ([20, 35, 90], [25, 62, 95])        # abuts a's first, joins a's second and third
    c = ([], [])
    table, m_peaks = cluster_ref([a, b, c])
    assert table.tolist() == [[10, 20, 1, 1], [20, 25, 1, 1], [30, 70, 3, 2], [90, 95, 1, 1]]
    assert m_peaks.tolist() == [[1, 0, 0], [0, 1, 0], [2, 1, 0], [0, 1, 0]]
    table, m_peaks = cluster_ref([([5], [9]), ([5], [9])])
    assert table.tolist() == [[5, 9, 2, 2]] and m_peaks.tolist() == [[1, 1]]
    table, m_peaks = cluster_ref([])
    assert table.shape == (0, 4) and m_peaks.shape == (0, 0)
    table, _ = cluster_ref([([1], [10]), ([2], [3]), ([9], [12]), ([12], [13])])   # nested, chained, abutting
    assert table.tolist() == [[1, 12, 3, 3], [12, 13, 1, 1]]


def test_prefix_region_reference_equals_the_slices():
    """region_ref_prefix() against region_ref(): the by-hand cases, and random regions of every
    length (a base, a power of two, one more, the contig and beyond both ends) on vectors of 1, 2,
    1000 and 4097 bases, with counts up to 2^31 - 1"""
    from consensus_ref import region_ref_prefix
    vector = [3, 3, 7, 7, 7, 1]
    starts = [100, 101, 103, 90, 104, 106, 50, 99, 102]
    ends = [106, 103, 104, 101, 200, 110, 60, 300, 103]
    for got, want in zip(region_ref_prefix(vector, 100, starts, ends), region_ref(vector, 100, starts, ends)):
        assert got.dtype == want.dtype and got.tolist() == want.tolist()
    rng = np.random.default_rng(12)
    for n, first in ((1, 0), (2, 5), (1000, 77), (4097, 2147483647 - 4097)):
        v = rng.integers(0, 2147483648, n).astype(np.int32)
        a = np.concatenate([rng.integers(first - 20, first + n + 10, 2999), [first - 3]])
        width = np.concatenate([rng.integers(1, n + 40, 2000), 2 ** rng.integers(0, 13, 500),
                                2 ** rng.integers(0, 13, 499) + rng.integers(-1, 2, 499), [n + 6]])
        b = np.minimum(a + np.maximum(width, 1), 2 ** 31 - 1)
        keep = a < b
        got, want = region_ref_prefix(v, first, a[keep], b[keep]), region_ref(v, first, a[keep], b[keep])
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (n, first)
        assert (want[0] == 0).any() and (want[0] == n).any()
    empty = region_ref_prefix([], 0, [0, 5], [3, 9])
    assert [x.tolist() for x in empty] == [[0, 0]] * 3
    assert [len(x) for x in region_ref_prefix(vector, 0, [], [])] == [0, 0, 0]


def test_sorted_cluster_reference_equals_the_sweep():
    """cluster_ref_sorted() against cluster_ref(): the by-hand cases and random members with
    abutting, nested, chained and identical peaks"""
    from consensus_ref import cluster_ref_sorted
    cases = [[([10, 30, 60], [20, 40, 70]), ([20, 35, 90], [25, 62, 95]), ([], [])],
             [([5], [9]), ([5], [9])], [], [([], []), ([], [])],
             [([1], [10]), ([2], [3]), ([9], [12]), ([12], [13])],
             [([10, 19], [19, 30]), ([19], [25])]]
    rng = np.random.default_rng(13)
    for n, top in ((40, 300), (300, 2000), (300, 20000)):
        members = []
        for _ in range(4):
            cuts = np.sort(rng.choice(np.arange(top), size=2 * n, replace=False))
            start, end = cuts[0::2].copy(), cuts[1::2].copy()
            glue = rng.random(n - 1) < 0.2
            end[:-1][glue] = start[1:][glue]
            members.append((start, end))
        members.append(members[0])
        cases.append(members)
    for members in cases:
        table, m_peaks = cluster_ref_sorted(members)
        want_table, want_peaks = cluster_ref(members)
        assert table.dtype == want_table.dtype and table.shape == want_table.shape
        assert np.array_equal(table, want_table) and np.array_equal(m_peaks, want_peaks)
    assert len(cluster_ref(cases[-1])[0]) > 50
