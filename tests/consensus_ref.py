"""The numpy yardsticks of region_stats() and peak_clusters(): nothing here comes from the library.

region_ref() expands nothing cleverly: it takes the per-base coverage vector of a contig and slices
it.  cluster_ref() is a plain sweep over the peaks of all members sorted by start.  Everything is
integer arithmetic, so the tests compare for equality."""
import numpy as np


def region_ref(vector, first, starts, ends):
    """(bases int32[], sum int64[], max int32[]) of the regions [starts[i], ends[i]) of a contig
    whose per-base counts are `vector` and whose first base is at `first`"""
    v = np.asarray(vector, dtype=np.int64)
    n = len(starts)
    bases, total, largest = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int32)
    for i in range(n):
        a = max(int(starts[i]) - int(first), 0)
        b = min(int(ends[i]) - int(first), len(v))
        if b > a:
            part = v[a:b]
            bases[i], total[i], largest[i] = b - a, part.sum(), part.max()
    return bases, total, largest


def region_ref_prefix(vector, first, starts, ends):
    """region_ref() for very many regions: the sum from the prefix sums of the per-base vector, the
    maximum from a table of the maxima of all windows of 2^k bases (two windows cover a region).
    tests/test_consensus_cpu.py holds it against region_ref()."""
    v = np.asarray(vector, dtype=np.int64)
    a = np.maximum(np.asarray(starts, np.int64) - int(first), 0)
    b = np.minimum(np.asarray(ends, np.int64) - int(first), len(v))
    inside = b > a
    a, b = np.where(inside, a, 0), np.where(inside, b, 1 if len(v) else 0)
    prefix = np.concatenate([[0], np.cumsum(v)])
    levels = [v]
    while 2 << (len(levels) - 1) <= len(v):
        half, last = 1 << (len(levels) - 1), levels[-1]
        levels.append(np.maximum(last[:-half], last[half:]))
    k = np.zeros(len(a), np.int64)
    if len(v):
        k = np.floor(np.log2(np.maximum(b - a, 1))).astype(np.int64)
        k = np.where((1 << k) > b - a, k - 1, k)           # (log2 of an integer near a power of two)
        k = np.where((2 << k) <= b - a, k + 1, k)
    largest = np.zeros(len(a), np.int64)
    for level in np.unique(k) if len(v) else []:
        at = np.flatnonzero(k == level)
        table = levels[int(level)]
        largest[at] = np.maximum(table[a[at]], table[b[at] - (1 << int(level))])
    bases = np.where(inside, b - a, 0)
    total = np.where(inside, prefix[b] - prefix[a], 0)
    return bases.astype(np.int32), total.astype(np.int64), np.where(inside, largest, 0).astype(np.int32)


def cluster_ref_sorted(members):
    """cluster_ref() for very many peaks, as array operations: all peaks sorted by start; a peak
    opens a cluster where it starts at or after the largest end before it.  The matrix counts each
    member's peaks in the cluster they fell into: a peak that meets a cluster's span meets one of its
    peaks (the span is their union) and so belongs to it, which is cluster_ref()'s condition.
    tests/test_consensus_cpu.py holds it against cluster_ref()."""
    n_members = len(members)
    s = np.concatenate([np.asarray(ps, np.int64) for ps, _ in members] + [np.zeros(0, np.int64)])
    e = np.concatenate([np.asarray(pe, np.int64) for _, pe in members] + [np.zeros(0, np.int64)])
    m = np.concatenate([np.full(len(ps), j, np.int64) for j, (ps, _) in enumerate(members)] +
                       [np.zeros(0, np.int64)])
    if len(s) == 0:
        return np.zeros((0, 4), np.int64), np.zeros((0, n_members), np.int64)
    order = np.lexsort((m, e, s))
    s, e, m = s[order], e[order], m[order]
    opens = np.concatenate([[True], s[1:] >= np.maximum.accumulate(e)[:-1]])
    cluster = np.cumsum(opens) - 1
    k = int(cluster[-1]) + 1
    m_peaks = np.zeros((k, n_members), np.int64)
    np.add.at(m_peaks, (cluster, m), 1)
    table = np.stack([s[opens], np.maximum.reduceat(e, np.flatnonzero(opens)),
                      np.bincount(cluster, minlength=k), (m_peaks > 0).sum(axis=1)], axis=1)
    return table.astype(np.int64), m_peaks


def cluster_ref(members):
    """members: a list of (peak_start, peak_end) arrays, each sorted and disjoint.
    -> (table int64 [k, 4]: clusterStart, clusterEnd, peaks, samples in increasing clusterStart,
        m_peaks int64 [k, len(members)]: member m's peaks with ps < clusterEnd && clusterStart < pe)"""
    rows = sorted((int(s), int(e), m) for m, (ps, pe) in enumerate(members) for s, e in zip(ps, pe))
    clusters = []       # [start, end, peaks, set of members]
    for s, e, m in rows:
        if clusters and s < clusters[-1][1]:      # overlaps what the sweep has open
            c = clusters[-1]
            c[1], c[2] = max(c[1], e), c[2] + 1
            c[3].add(m)
        else:
            clusters.append([s, e, 1, {m}])
    table = np.array([[c[0], c[1], c[2], len(c[3])] for c in clusters], dtype=np.int64).reshape(-1, 4)
    m_peaks = np.zeros((len(clusters), len(members)), dtype=np.int64)
    for k, c in enumerate(clusters):
        for m, (ps, pe) in enumerate(members):
            ps, pe = np.asarray(ps, np.int64), np.asarray(pe, np.int64)
            m_peaks[k, m] = int(np.sum((ps < c[1]) & (c[0] < pe)))
    return table, m_peaks
