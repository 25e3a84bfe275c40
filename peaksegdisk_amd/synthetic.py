"""Seeded synthetic coverage for the benchmark configurations.

Piecewise-constant Poisson coverage: background and peak segments alternate, segment lengths
are geometric (mean 2000 bins background / 200 bins peak), rates are U(0.2,1.0) background /
U(4,20) peak, counts ~ Poisson(rate), bin widths ~ U{1..49} bases, bins contiguous from 0.

The random stream is a counter-based splitmix64 implemented here (not numpy's generator), so
a (seed, n_bins) pair names the same data on every machine; tests pin a sha256.
"""
import hashlib

import numpy as np

_GOLD = np.uint64(0x9E3779B97F4A7C15)


def splitmix64(seed, idx):
    """splitmix64 output for state seed + (idx+1)*golden; idx: uint64 array."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.asarray(idx, dtype=np.uint64) + np.uint64(1)) * _GOLD
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uniform01(seed, stream, n, offset=0):
    """n doubles in (0,1) from stream `stream` of `seed`."""
    idx = np.arange(offset, offset + n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        s = np.uint64(seed) ^ (np.uint64(stream) * np.uint64(0xD1B54A32D192ED03))
    u = splitmix64(s, idx) >> np.uint64(11)
    return (u.astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def poisson_from_uniform(lam, u):
    """Poisson counts by CDF inversion (lam <= ~30 here)."""
    lam = np.asarray(lam, dtype=np.float64)
    p = np.exp(-lam)
    cdf = p.copy()
    count = np.zeros(lam.shape, dtype=np.int32)
    active = u > cdf
    k = 0
    while active.any() and k < 400:
        k += 1
        p = p * lam / k
        cdf = cdf + p
        count[active] += 1
        active = active & (u > cdf)
    return count


def poisson_coverage(n_bins, seed=1):
    """Returns (chromStart, chromEnd, count) int32 arrays of length n_bins."""
    n_bins = int(n_bins)
    # enough alternating segments to cover n_bins (mean pair length 2200)
    n_seg = max(16, int(n_bins / 1100.0 * 1.5) + 16)
    while True:
        u_len = uniform01(seed, 1, n_seg)
        u_rate = uniform01(seed, 2, n_seg)
        is_peak = (np.arange(n_seg) % 2) == 1
        mean_len = np.where(is_peak, 200.0, 2000.0)
        q = 1.0 / mean_len
        length = 1 + np.floor(np.log(u_len) / np.log1p(-q)).astype(np.int64)
        if int(length.sum()) >= n_bins:
            break
        n_seg *= 2
    rate = np.where(is_peak, 4.0 + 16.0 * u_rate, 0.2 + 0.8 * u_rate)
    seg_of_bin = np.repeat(np.arange(n_seg), length)[:n_bins]
    lam = rate[seg_of_bin]
    count = poisson_from_uniform(lam, uniform01(seed, 3, n_bins))
    width = 1 + np.floor(uniform01(seed, 4, n_bins) * 49.0).astype(np.int64)
    chrom_end = np.cumsum(width)
    chrom_start = chrom_end - width
    if chrom_end[-1] >= 2 ** 31:
        raise ValueError("synthetic contig exceeds int32 coordinates")
    return chrom_start.astype(np.int32), chrom_end.astype(np.int32), count.astype(np.int32)


def poisson_reads(n_bins, seed=1):
    """Aligned reads placed by poisson_coverage's piecewise rate: every bin of that coverage starts
    `count` reads at positions uniform over the bin, lengths uniform on 20..115 (ChIPreads' range).
    Returns (chromStart, chromEnd) int32 arrays sorted by chromStart and the extent (0, the
    coverage's last chromEnd); reads that run over the extent's end are left to be clipped."""
    cs, ce, cnt = poisson_coverage(n_bins, seed=seed)
    n = int(cnt.sum(dtype=np.int64))
    bin_of = np.repeat(np.arange(len(cnt)), cnt)
    width = (ce - cs).astype(np.int64)[bin_of]
    start = cs.astype(np.int64)[bin_of] + np.floor(uniform01(seed, 5, n) * width).astype(np.int64)
    length = 20 + np.floor(uniform01(seed, 6, n) * 96.0).astype(np.int64)
    order = np.argsort(start, kind="stable")
    start, end = start[order], (start + length)[order]
    if n and end.max() >= 2 ** 31:
        raise ValueError("synthetic reads exceed int32 coordinates")
    return start.astype(np.int32), end.astype(np.int32), (0, int(ce[-1]))


def stranded_reads(seed, bases, n_sites, per_site, d, jitter, read_length, both):
    """Single-end reads around binding sites on [0, bases): (chromStart, chromEnd) int32 and the
    strand int8 (+1 / -1).  uK is uniform01(seed, K, n).  Sites:
    d + jitter + floor(u11 (bases - 2 (d + jitter) - 2)); each has per_site fragments of the lengths
    d + floor(u12 (2 jitter + 1)) - jitter, which start at site - floor(u13 length).  both: every
    fragment [fs, fe) gives a plus read [fs, fs + read_length) and a minus read
    [fe - read_length, fe), all plus reads first; else one of the two, the plus read iff u14 < 0.5."""
    n = int(n_sites) * int(per_site)
    site = d + jitter + np.floor(uniform01(seed, 11, n_sites) * (bases - 2 * (d + jitter) - 2)).astype(np.int64)
    site = np.repeat(site, per_site)
    length = d + np.floor(uniform01(seed, 12, n) * (2 * jitter + 1)).astype(np.int64) - jitter
    fs = site - np.floor(uniform01(seed, 13, n) * length).astype(np.int64)
    fe = fs + length
    if both:
        start = np.concatenate([fs, fe - read_length])
        end = np.concatenate([fs + read_length, fe])
        strand = np.concatenate([np.ones(n, np.int8), -np.ones(n, np.int8)])
    else:
        plus = uniform01(seed, 14, n) < 0.5
        start = np.where(plus, fs, fe - read_length)
        end = np.where(plus, fs + read_length, fe)
        strand = np.where(plus, 1, -1).astype(np.int8)
    return start.astype(np.int32), end.astype(np.int32), strand


def shuffled(seed, *arrays):
    """the arrays in one seeded random order (reads as an unsorted BAM would give them)"""
    order = np.argsort(uniform01(seed, 7, len(arrays[0])), kind="stable")
    return tuple(a[order] for a in arrays)


def duplicated_reads(seed, n, bases, share=0.2, read_length=36):
    """n single-end reads of read_length on [0, bases + read_length) of which floor(share n) are
    duplicates: (chromStart, chromEnd) int32, the strand int8 and the number of duplicates.  uK is
    uniform01(seed, K, .).  The m = n - duplicates originals have distinct starts
    i step + floor(u21 step), step = bases // m, and the strand +1 iff u22 < 0.5, so their keys are
    distinct by fragment and by 5' end alike; duplicate j is a copy of original floor(u23 m), strand
    included; all of them in the order of u24 (stable).  At keep = 1 a removal leaves exactly the m
    originals' units: distinct = kept = m of n reads."""
    n = int(n)
    dup = int(share * n)
    m = n - dup
    step = int(bases) // max(m, 1)
    if m < 1 or step < 1:
        raise ValueError("duplicated_reads: %d originals do not fit %d bases" % (m, bases))
    start = np.arange(m, dtype=np.int64) * step + np.floor(uniform01(seed, 21, m) * step).astype(np.int64)
    strand = np.where(uniform01(seed, 22, m) < 0.5, 1, -1).astype(np.int8)
    source = np.minimum(np.floor(uniform01(seed, 23, dup) * m).astype(np.int64), m - 1)
    start = np.concatenate([start, start[source]])
    strand = np.concatenate([strand, strand[source]])
    order = np.argsort(uniform01(seed, 24, n), kind="stable")
    start, strand = start[order], strand[order]
    if n and start.max() + read_length >= 2 ** 31:
        raise ValueError("synthetic reads exceed int32 coordinates")
    return start.astype(np.int32), (start + read_length).astype(np.int32), strand, dup


def increasing_coverage(n_bins):
    """Worst case of vignettes/Worst_case.Rmd:26-28: count = 1..N, width 1."""
    n_bins = int(n_bins)
    end = np.arange(1, n_bins + 1, dtype=np.int32)
    return (end - 1).astype(np.int32), end, end.copy()


def penalty_grid(n=64, lo=-1.0, hi=5.0):
    """n log-spaced penalties 10^lo..10^hi as strings with 15 significant digits, the way
    R's paste() formats a double."""
    return ["%.15g" % (10.0 ** e) for e in np.linspace(lo, hi, n)]


def write_bedgraph(path, chrom_start, chrom_end, count, chrom="chrSynth"):
    with open(path, "w") as f:
        f.write("".join("%s\t%d\t%d\t%d\n" % (chrom, s, e, c)
                        for s, e, c in zip(chrom_start.tolist(), chrom_end.tolist(),
                                           count.tolist())))


def sha256_of(chrom_start, chrom_end, count):
    h = hashlib.sha256()
    for a in (chrom_start, chrom_end, count):
        h.update(np.ascontiguousarray(a, dtype=np.int32).tobytes())
    return h.hexdigest()
