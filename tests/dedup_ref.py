"""The contract of duplicate removal (include/peaksegdisk_hip.h) restated in
plain Python: a dict of running sums per key, walked in input order.  What the device's out_count,
summary and compacted reads are compared with; pinned against hand-written answers in
tests/test_dedup_cpu.py.  Nothing here calls the library under test."""
import numpy as np

SUMMARY = ("reads", "kept", "rows_kept", "distinct")


def key_of(by, start, end, strand):
    """fragment: (chromStart, chromEnd, strand); five_prime: (5' base, strand), the 5' base
    chromStart of a plus read and chromEnd - 1 of a minus read"""
    if by == "fragment":
        return (start, end, strand)
    if by == "five_prime":
        return (start if strand > 0 else end - 1, strand)
    raise ValueError(by)


def counts_of(n, count):
    return np.ones(n, np.int64) if count is None else np.asarray(count, np.int64)


def before_sums(start, end, count, strand, by):
    """One contig: before(i) = the sum of c(j) over j < i with key(j) = key(i), int64.  count None:
    every read counts 1; strand None: every read is plus (fragment only)."""
    n = len(start)
    assert strand is not None or by == "fragment"
    start, end = [int(v) for v in start], [int(v) for v in end]
    count = counts_of(n, count).tolist()
    strand = [1] * n if strand is None else [int(v) for v in strand]
    assert all(s < e for s, e in zip(start, end)) and all(c >= 0 for c in count)
    assert all(d in (1, -1) for d in strand) and sum(count) < 2 ** 31
    seen = {}
    before = np.zeros(n, np.int64)
    for i in range(n):
        key = key_of(by, start[i], end[i], strand[i])
        before[i] = seen.get(key, 0)
        seen[key] = int(before[i]) + count[i]
    return before


def marks(before, count, keep):
    """(out_count int32, [reads, kept, rows_kept, distinct]) of one contig at `keep`:
    out_count(i) = min(c(i), max(keep - before(i), 0))"""
    assert keep >= 1
    c = counts_of(len(before), count)
    out = np.minimum(c, np.maximum(int(keep) - before, 0))
    return out.astype(np.int32), [int(c.sum()), int(out.sum()), int((out > 0).sum()),
                                  int(((c > 0) & (before == 0)).sum())]


def dedup(start, end, count, strand, keep, by):
    return marks(before_sums(start, end, count, strand, by), count, keep)


def compacted(start, end, keep_count, strand=None):
    """the rows with keep_count > 0, in order: (chromStart, chromEnd, count, strand or None)"""
    rows = np.flatnonzero(np.asarray(keep_count) > 0)
    return (np.asarray(start)[rows], np.asarray(end)[rows], np.asarray(keep_count)[rows],
            None if strand is None else np.asarray(strand)[rows])
