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
