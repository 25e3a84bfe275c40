"""The yardsticks of the held-out loss (ProblemSet.heldout_loss), written as plain loops from the
definition in include/peaksegdisk_hip.h.

heldout_pair_ref: B_k and Y_k are Python integers (from the set's own segment_columns() and the
dense input), the terms use math.log, the sum is math.fsum.  The tolerance is derived, not measured:
    (n_add + 6) * 2^-52 * sum_k (|x_k B_k| + Y_k (|log x_k| + 1))
n_add is the longest chain of additions a term passes through in the device's fixed order:
ceil(rows / 256) in its thread, six in the tree over the 64 lanes of a wave, three over the four
waves.  The 6 covers the roundings of a * mean, x * B, int64 -> double, the product with the
logarithm and the difference, and psd_log's error of less than one ulp."""
import math

THREADS = 256


def n_add(rows):
    return -(-rows // THREADS) + 6 + 3


def heldout_pair_ref(columns, vector, scale):
    """columns: (chromStart, chromEnd, mean) of a problem as segment_columns() gives them with
    first_chromStart 0; vector: the per-base counts of the contig the model is scored on ->
    {"loss", "rows", "bases", "sum", "zero_mean_rows", "tol"}"""
    start, end, mean = columns
    terms, weight = [], 0.0
    bases = total = zero = 0
    for k in range(len(start)):
        s, e, m = int(start[k]), int(end[k]), float(mean[k])
        b = e - s
        y = 0
        for v in vector[s:e].tolist():
            y += int(v)
        bases += b
        total += y
        x = scale * m
        if y == 0:
            terms.append(x * b)
            weight += abs(x * b)
        elif m > 0.0:
            terms.append(x * b - y * math.log(x))
            weight += abs(x * b) + y * (abs(math.log(x)) + 1.0)
        else:
            zero += 1
    rows = len(start)
    return {"loss": math.fsum(terms) if zero == 0 else math.inf, "rows": rows, "bases": bases,
            "sum": total, "zero_mean_rows": zero,
            "tol": (n_add(rows) + 6) * 2.0 ** -52 * weight}


# ---- the folds: a numpy restatement of the hash with synthetic.splitmix64 ------------------------

BITS = {2: 1, 4: 2, 8: 3}


def contig_seed(seed, i):
    import numpy as np
    with np.errstate(over="ignore"):
        return np.uint64(seed % 2 ** 64) ^ (np.uint64(i + 1) * np.uint64(0xD1B54A32D192ED03))


def dense_folds_ref(vector, i, folds, seed):
    """int64 [folds, bases]: the units of every base of input contig i that fall in each fold"""
    import numpy as np
    from peaksegdisk_amd.synthetic import splitmix64
    bits = BITS[folds]
    per = 64 // bits
    n = len(vector)
    h = splitmix64(contig_seed(seed, i), np.arange(n, dtype=np.uint64))
    shifts = (np.arange(per, dtype=np.uint64) * np.uint64(bits))[None, :]
    t = np.zeros((folds, n), dtype=np.int64)
    for b in range(n):
        count = int(vector[b])
        if count == 0:
            continue
        words = splitmix64(h[b], np.arange(-(-count // per), dtype=np.uint64))
        fields = ((words[:, None] >> shifts) & np.uint64(folds - 1)).reshape(-1)[:count]
        t[:, b] = np.bincount(fields.astype(np.int64), minlength=folds)
    return t


def read_folds_ref(n_reads, i, folds, seed):
    """int64 [n_reads]: the fold of every read of input contig i"""
    import numpy as np
    from peaksegdisk_amd.synthetic import splitmix64
    h = splitmix64(contig_seed(seed, i), np.arange(n_reads, dtype=np.uint64))
    word0 = np.array([splitmix64(x, np.zeros(1, dtype=np.uint64))[0] for x in h], dtype=np.uint64)
    return (word0 >> np.uint64(64 - BITS[folds])).astype(np.int64)


def pileup_ref(start, end, count, lo, hi, bases_counted="each"):
    """int64 [hi - lo]: the coverage of the reads, clipped to the extent; plain loops"""
    import numpy as np
    cov = np.zeros(hi - lo, dtype=np.int64)
    for s, e, k in zip(start.tolist(), end.tolist(), count.tolist()):
        if bases_counted == "end":
            s = e - 1
        s, e = max(s, lo), min(e, hi)
        if s < e:
            cov[s - lo:e - lo] += k
    return cov
