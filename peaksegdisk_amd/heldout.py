"""The penalty without labels: K-fold thinning scored by the held-out Poisson loss (DESIGN.md
section 18).  The sampling units of every sample -- the reads, or the unit counts of a base of dense
coverage -- are split at random into K folds on the device (ProblemSet.from_dense_folds /
from_reads_folds); every fold's train contig is solved at every penalty in one solve(); one
ProblemSet.heldout_loss() call scores all models on their folds' test contigs; the tables and the
choice are made here, on the host.

The test fold holds 1/K of the units and the train folds (K - 1)/K, so the expected test mean is the
train mean over K - 1: the pairs' scale.  A penalty lambda on data thinned by eps = (K - 1)/K
penalises as lambda / eps does on all the data (the Poisson loss of the thinned data at the means
eps m is eps times the full loss plus a constant of the model), so the penalty for all the data is
train_penalty K / (K - 1)."""
import math

import numpy as np

RULES = ("min", "1se")


def selection_pairs(n_inputs, folds, n_penalties):
    """the (problem, contig, scale) of the one heldout_loss() call over a fold set: problem
    (i K + f) P + j -- the train contig of input i and fold f at penalties[j] -- on the test contig
    (i K + f) 2 + 1, with the scale 1 / (K - 1)"""
    problem = np.arange(n_inputs * folds * n_penalties, dtype=np.int32)
    contig = ((problem // n_penalties) * 2 + 1).astype(np.int32)
    scale = np.full(len(problem), 1.0 / (folds - 1), dtype=np.float64)
    return problem, contig, scale


class HeldoutSelection:
    """What select_penalty_dense / select_penalty_reads return for one sample.
    table: a data frame with one row per (fold, penalty), fold-major: penalty, fold, peaks,
        segments, heldout_loss, zero_mean_rows.
    summary: a data frame with one row per penalty in the order given: penalty, heldout_loss (the
        sum over the folds), se (the standard error of that sum across the folds: sqrt(K) times
        the folds' standard deviation with K - 1 degrees of freedom; inf where a fold's loss is
        not finite), peaks (the mean over the folds).
    rule, train_penalty, train_index: the choice among the penalties on the thinned data.
        "min": the smallest summed loss; among equal sums the larger penalty; a penalty with a
        +Inf fold never wins unless all have one.  "1se": the largest penalty whose sum is within
        one standard error (the winner's) of the smallest.
    penalty: train_penalty K / (K - 1), the penalty that penalises all the data as train_penalty
        penalised the thinned.
    fit: with refit=True, the PeakSegFPOP_dense / _reads result on all the data at `penalty`."""

    def __init__(self, penalties, folds, peaks, segments, heldout_loss, zero_mean_rows, rule="min"):
        import pandas as pd
        if rule not in RULES:
            raise ValueError('rule is %r, neither "min" nor "1se"' % (rule,))
        pens = np.asarray(penalties, dtype=np.float64).reshape(-1)
        k, p = int(folds), len(pens)
        if k < 2 or p < 1:
            raise ValueError("a selection needs two folds and one penalty at least")
        cols = [np.asarray(a).reshape(k, p) for a in (peaks, segments, heldout_loss, zero_mean_rows)]
        loss = cols[2].astype(np.float64)
        self.folds = k
        self.rule = rule
        self.table = pd.DataFrame({
            "penalty": np.tile(pens, k), "fold": np.repeat(np.arange(k), p),
            "peaks": cols[0].reshape(-1).astype(np.int64),
            "segments": cols[1].reshape(-1).astype(np.int64),
            "heldout_loss": loss.reshape(-1),
            "zero_mean_rows": cols[3].reshape(-1).astype(np.int64)})
        total = np.array([math.fsum(loss[:, j]) if np.isfinite(loss[:, j]).all() else math.inf
                          for j in range(p)])
        with np.errstate(invalid="ignore"):
            se = np.where(np.isfinite(total), np.std(loss, axis=0, ddof=1) * math.sqrt(k), math.inf)
        self.summary = pd.DataFrame({"penalty": pens, "heldout_loss": total, "se": se,
                                     "peaks": cols[0].astype(np.float64).mean(axis=0)})
        self.train_index = self._choose(pens, total, se, rule)
        self.train_penalty = float(pens[self.train_index])
        self.penalty = self.train_penalty * k / (k - 1)
        self.fit = None

    @staticmethod
    def _choose(pens, total, se, rule):
        finite = np.isfinite(total)
        among = np.flatnonzero(finite) if finite.any() else np.arange(len(pens))
        best = min(among, key=lambda j: (total[j], -pens[j]))
        if rule == "1se" and finite.any():
            within = [j for j in among if total[j] <= total[best] + se[best]]
            best = max(within, key=lambda j: (pens[j], -total[j]))
        return int(best)


def select_from_set(pset, rule="min"):
    """The selections of a SOLVED fold set (ProblemSet.from_dense_folds / from_reads_folds), one per
    input contig: one heldout_loss() call over all inputs x folds x penalties, then the tables."""
    n, k, pens = pset.fold_inputs, pset.folds, pset.fold_penalties
    out = pset.heldout_loss(selection_pairs(n, k, len(pens)))
    per = k * len(pens)
    segments = np.array([pset.result(p).n_segments for p in range(n * per)], dtype=np.int64)
    return [HeldoutSelection(pens, k, (segments[i * per:(i + 1) * per] - 1) // 2,
                             segments[i * per:(i + 1) * per], out["loss"][i * per:(i + 1) * per],
                             out["zero_mean_rows"][i * per:(i + 1) * per], rule)
            for i in range(n)]
