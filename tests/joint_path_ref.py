"""The yardstick of ProblemSet.joint_label_errors: the definitions of include/peaksegdisk_hip.h in
plain Python loops over windows, members and labels, from what joint_peaks() / joint_path() return.

The peaks of problem q in a model: the joint peaks [peakStart, peakEnd) of the windows of q's group
with peakStart >= 0 at which q is up -- every window's, also where two windows' peaks coincide.
  noPeaks    count = peaks with ps < le and ls < pe    false positive: count >= 1
  peaks      count = the same                          false negative: count == 0
  peakStart  count = peaks with ls <= ps < le          fp: count >= 2, fn: count == 0
  peakEnd    count = peaks with ls < pe <= le          fp: count >= 2, fn: count == 0"""
import numpy as np

NO_PEAKS, PEAK_START, PEAK_END, PEAKS = range(4)


def peaks_of(model, n_problems):
    """model: what joint_peaks() returns (a list over groups) -> per problem its list of (ps, pe)"""
    out = [[] for _ in range(n_problems)]
    for entry in model:
        frame = entry["joint"]
        for w in range(len(frame)):
            ps, pe = int(frame["peakStart"][w]), int(frame["peakEnd"][w])
            if ps < 0:
                continue
            for i, q in enumerate(entry["members"].tolist()):
                if int(entry["up"][w, i]) == 1:
                    out[q].append((ps, pe))
    return out


def label_row(peaks, ls, le, a):
    """(count, fp, fn) of one label"""
    n = 0
    for ps, pe in peaks:
        if a == PEAK_START:
            n += ls <= ps < le
        elif a == PEAK_END:
            n += ls < pe <= le
        else:
            n += ps < le and ls < pe
    if a == NO_PEAKS:
        return n, int(n >= 1), 0
    if a == PEAKS:
        return n, 0, int(n == 0)
    return n, int(n >= 2), int(n == 0)


def joint_label_errors_ref(models, labels):
    """models: a list over penalties of what joint_peaks() returns; labels: per problem
    (chromStart, chromEnd, annotation codes) or None -> (model_totals int64 [P, 5], problem_totals
    int32 [P, Q, 5], rows[p][q] = (count, fp, fn) int32 arrays)"""
    n_problems = len(labels)
    model_totals = np.zeros((len(models), 5), np.int64)
    problem_totals = np.zeros((len(models), n_problems, 5), np.int32)
    rows = []
    for p, model in enumerate(models):
        peaks = peaks_of(model, n_problems)
        rows.append([])
        for q, entry in enumerate(labels):
            cols = [[], [], []]
            if entry is not None and len(entry):
                for ls, le, a in zip(*[np.asarray(v).tolist() for v in entry]):
                    n, fp, fn = label_row(peaks[q], ls, le, a)
                    for col, v in zip(cols, (n, fp, fn)):
                        col.append(v)
                    problem_totals[p, q] += [fp + fn, fp, fn, int(a != PEAKS), int(a != NO_PEAKS)]
            rows[-1].append(tuple(np.array(c, np.int32) for c in cols))
        model_totals[p] = problem_totals[p].astype(np.int64).sum(axis=0)
    return model_totals, problem_totals, rows
