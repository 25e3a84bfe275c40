"""Fitting the penalty model: interval regression with an L1 penalty and cross-validation, the
fits on the GPU.  The targets are the intervals of log(penalty) that
targetInterval_dense / targetInterval_reads find, the inputs the coverage features of
problem_features_dense / problem_features_reads, and the result is the dictionary that
penalty_model= and predict_penalties take.

The host prepares one standardised matrix and chooses among the fits; every fit -- a problem per
(fold, regularization) and one per regularization on all rows -- runs in one launch of
peakseg_hip_penalty_fit.  The convention is penaltyLearning::IntervalRegressionCV's (squared
hinge of margin 1, unpenalised intercept, its grid of regularizations and its threshold), with one
stated difference: the features are standardised once over all rows, not per training set, so that
every problem of a call is a subproblem of one matrix."""
import ctypes

import numpy as np
import pandas as pd

from . import _native

DEFAULT_THRESHOLD = 1e-3
MAX_FOLDS = 16
TABLE_COLUMNS = ["regularization", "validation.incorrect", "validation.hinge", "train.incorrect",
                 "nonzero", "iterations", "converged"]


def default_regularizations():
    """penaltyLearning's path: from 0.001 by factors of 1.2"""
    return 0.001 * 1.2 ** np.arange(64)


def default_folds(n, n_folds=5):
    """(F, fold): row i in fold i mod F, F = min(n_folds, n)"""
    if not (isinstance(n_folds, (int, np.integer)) and 1 <= n_folds <= MAX_FOLDS):
        raise ValueError("n_folds: an integer from 1 to %d" % MAX_FOLDS)
    folds = min(int(n_folds), int(n))
    return folds, (np.arange(n) % folds).astype(np.int32)


def target_limits(targets):
    """(n, 2) float64: min_log_lambda, max_log_lambda of a list of TargetInterval or of an array"""
    if isinstance(targets, (list, tuple)) and all(hasattr(t, "min_log_lambda") for t in targets):
        targets = [(t.min_log_lambda, t.max_log_lambda) for t in targets]
    limits = np.asarray(targets, dtype=np.float64)
    if limits.size == 0:
        limits = limits.reshape(0, 2)
    if limits.ndim != 2 or limits.shape[1] != 2:
        raise ValueError("targets: a list of TargetInterval or an (n, 2) array of min_log_lambda, "
                         "max_log_lambda")
    if np.isnan(limits).any():
        raise ValueError("targets: row %d holds a NaN" % int(np.flatnonzero(np.isnan(limits).any(axis=1))[0]))
    bad = np.flatnonzero(limits[:, 0] > limits[:, 1])
    if len(bad):
        raise ValueError("targets: row %d: min_log_lambda exceeds max_log_lambda" % int(bad[0]))
    return limits


class Prepared:
    """What the host makes of a feature table and its targets: rows (the indices kept), dropped_rows,
    names (the columns kept), dropped_features {name: reason}, x (the kept rows and columns,
    standardised), mean, sd, lo, hi."""


def prepare(features, targets, columns=None):
    """Drops the rows whose limits are both infinite, then the columns that are not finite in some
    remaining row ("not finite") or equal in all of them ("constant"), and standardises the rest
    over the remaining rows: (x - mean) / sd, sd with n - 1, in float64."""
    from .grid import FEATURE_NAMES
    if columns is None:
        columns = [name for name in FEATURE_NAMES if name in features.columns]
    columns = list(columns)
    for name in columns:
        if name not in FEATURE_NAMES:
            raise ValueError("fit_penalty_model: unknown feature %r" % (name,))
        if name not in features.columns:
            raise ValueError("fit_penalty_model: the feature table has no column %r" % (name,))
    limits = target_limits(targets)
    if len(limits) != len(features):
        raise ValueError("fit_penalty_model: %d targets for %d rows of features" % (len(limits), len(features)))
    informative = np.isfinite(limits).any(axis=1)
    out = Prepared()
    out.rows = np.flatnonzero(informative)
    out.dropped_rows = np.flatnonzero(~informative).tolist()
    if len(out.rows) < 2:
        raise ValueError("fit_penalty_model: %d rows with a finite limit; at least two are needed"
                         % len(out.rows))
    out.lo = np.ascontiguousarray(limits[out.rows, 0])
    out.hi = np.ascontiguousarray(limits[out.rows, 1])
    raw = features[columns].to_numpy(dtype=np.float64).reshape(len(features), len(columns))[out.rows]
    out.names, out.dropped_features, keep = [], {}, []
    for j, name in enumerate(columns):
        column = raw[:, j]
        if not np.all(np.isfinite(column)):
            out.dropped_features[name] = "not finite"
        elif np.all(column == column[0]):
            out.dropped_features[name] = "constant"
        else:
            out.names.append(name)
            keep.append(j)
    raw = raw[:, keep]
    if len(keep) > _native.lib.peakseg_hip_penalty_fit_max_features():
        raise ValueError("fit_penalty_model: %d features; at most %d" % (
            len(keep), _native.lib.peakseg_hip_penalty_fit_max_features()))
    out.mean = raw.mean(axis=0) if len(keep) else np.zeros(0)
    out.sd = raw.std(axis=0, ddof=1) if len(keep) else np.zeros(0)
    # (a column whose values differ may still have sd 0 in floating point: it says nothing either)
    flat = np.flatnonzero(~(out.sd > 0))
    if len(flat):
        for j in flat:
            out.dropped_features[out.names[j]] = "constant"
        good = np.flatnonzero(out.sd > 0)
        out.names = [out.names[j] for j in good]
        raw, out.mean, out.sd = raw[:, good], out.mean[good], out.sd[good]
    out.x = (raw - out.mean) / out.sd
    return out


def gram_lambda_max(x):
    """The Lipschitz bound's eigenvalue: the largest of [x 1]'[x 1], times 1 + 1e-6 (eigvalsh's own
    error, at the cost of a millionth of the step)."""
    a = np.hstack([np.asarray(x, np.float64), np.ones((len(x), 1))])
    return float(np.linalg.eigvalsh(a.T @ a)[-1]) * (1.0 + 1e-6)


def select_regularization(table):
    """The row of the table that wins, or None: among the regularizations whose fits all converged,
    the fewest validation.incorrect, then the smallest validation.hinge, then the largest
    regularization."""
    best = None
    for k in range(len(table)):
        row = table.iloc[k]
        if not bool(row["converged"]):
            continue
        key = (int(row["validation.incorrect"]), float(row["validation.hinge"]), -float(row["regularization"]))
        if best is None or key < best[0]:
            best = (key, k)
    return None if best is None else best[1]


def back_transform(weights, names, mean, sd):
    """{"intercept", "weights"} in the features' own units from standardised weights (the intercept
    last): weight_j = w_j / sd_j, intercept = b - sum of w_j mean_j / sd_j; zero weights are left out"""
    w = np.asarray(weights, np.float64)
    intercept = float(w[-1])
    out = {}
    for j, name in enumerate(names):
        if w[j] != 0.0:
            out[name] = float(w[j] / sd[j])
            intercept -= float(w[j] * mean[j] / sd[j])
    return {"intercept": intercept, "weights": out}


def fit_problems(x, lo, hi, fold, n_folds, regularizations, lambda_max, threshold, max_iterations,
                 device=0):
    """peakseg_hip_penalty_fit on a standardised matrix x (n, p): -> dict of the raw tables, shaped
    (sets, K, ...) with sets = F + 1 (1 when F = 1), and ms.  RuntimeError with .status for a
    refusal."""
    lib = _native.lib
    x = np.asarray(x, np.float64)
    n, p = x.shape
    x_fm = np.ascontiguousarray(x.T)              # feature-major
    lo = np.ascontiguousarray(lo, dtype=np.float64)
    hi = np.ascontiguousarray(hi, dtype=np.float64)
    fold = np.ascontiguousarray(fold, dtype=np.int32)
    reg = np.ascontiguousarray(regularizations, dtype=np.float64)
    sets = 1 if n_folds == 1 else n_folds + 1
    k = len(reg)
    weights = np.zeros((sets, k, p + 1), np.float64)
    iterations = np.zeros((sets, k), np.int32)
    criterion = np.zeros((sets, k), np.float64)
    converged = np.zeros((sets, k), np.int32)
    incorrect = np.zeros((sets, k), np.int64)
    hinge = np.zeros((sets, k), np.float64)
    st = lib.peakseg_hip_penalty_fit(
        int(device), n, p, x_fm.ctypes.data, lo.ctypes.data, hi.ctypes.data, fold.ctypes.data,
        int(n_folds), k, reg.ctypes.data, float(lambda_max), float(threshold), int(max_iterations),
        weights.ctypes.data, iterations.ctypes.data, criterion.ctypes.data, converged.ctypes.data,
        incorrect.ctypes.data, hinge.ctypes.data)
    if st != 0:
        from .api import PeakSegError
        msg = _native.status_message(st, "<penalty model>", "", "")
        detail = lib.peakseg_hip_last_error().decode(errors="replace")
        raise PeakSegError(st, "%s (%s)" % (msg, detail) if detail else msg)
    ms = ctypes.c_float(0.0)
    lib.peakseg_hip_penalty_fit_last_ms(ctypes.byref(ms))
    return {"weights": weights, "iterations": iterations, "criterion": criterion,
            "converged": converged, "incorrect": incorrect, "hinge": hinge, "ms": float(ms.value)}


class PenaltyModelFit:
    """What fit_penalty_model returns: model ({"intercept", "weights"}: what penalty_model= and
    predict_penalties take), regularization (the chosen one), table (a row per regularization:
    regularization, validation.incorrect and validation.hinge summed over the folds,
    train.incorrect of the all-rows fit, nonzero weights of it, iterations -- the most of its
    problems -- and converged: all of them), weights (sets, K, p + 1: every problem's weights in
    standardised units, the intercept last, the all-rows problems in the last set), iterations,
    criterion, converged, incorrect, hinge (sets, K: the raw tables), feature_names, mean, sd (of
    the columns kept), rows (the rows kept), dropped_rows, dropped_features {name: "not finite" |
    "constant"}, fold (of the rows kept), n_folds, regularizations, ms (the launch)."""

    def __repr__(self):
        return "PenaltyModelFit(regularization=%r, %d weights, %d rows, %d features)" % (
            self.regularization, len(self.model["weights"]), len(self.rows), len(self.feature_names))


def make_table(raw, regularizations, n_folds):
    """the row per regularization of PenaltyModelFit.table from the raw tables of fit_problems"""
    folds = raw["incorrect"][:-1] if n_folds > 1 else raw["incorrect"][:0]
    fold_hinge = raw["hinge"][:-1] if n_folds > 1 else raw["hinge"][:0]
    return pd.DataFrame({
        "regularization": np.asarray(regularizations, np.float64),
        "validation.incorrect": folds.sum(axis=0).astype(np.int64),
        "validation.hinge": fold_hinge.sum(axis=0),
        "train.incorrect": raw["incorrect"][-1].astype(np.int64),
        "nonzero": np.count_nonzero(raw["weights"][-1][:, :-1], axis=1).astype(np.int64),
        "iterations": raw["iterations"].max(axis=0).astype(np.int64),
        "converged": raw["converged"].min(axis=0).astype(bool),
    }, columns=TABLE_COLUMNS)


def fit_penalty_model(features, targets, columns=None, regularizations=None, n_folds=5, fold=None,
                      threshold=DEFAULT_THRESHOLD, max_iterations=100000, device=0):
    """Fits the penalty model on the GPU.  features: the data frame of coverage_features /
    problem_features_* (one row per contig); targets: a list of target.TargetInterval, or an (n, 2)
    array of min_log_lambda, max_log_lambda (+-inf allowed); columns: the features to use (None:
    every column of grid.FEATURE_NAMES that is present; another name: ValueError);
    regularizations: increasing, at most 256 (None: 0.001 x 1.2**arange(64)); fold: an integer per
    row in [0, F) (None: row i in fold i mod F with F = min(n_folds, rows kept)), given for all rows
    of `features`; F = 1: no validation, one regularization.  Rows whose limits are both infinite and
    columns that are not finite or constant are dropped and reported.  Every (fold, regularization)
    and every all-rows problem is fitted in one launch (peakseg_hip_penalty_fit); the regularization
    is chosen among those whose fits all converged: fewest incorrect validation intervals summed
    over the folds, then the smaller validation hinge, then the larger regularization.  Returns a
    PenaltyModelFit; PeakSegError with status ERROR_FIT_ARGUMENTS when no regularization has all
    its fits converged."""
    prepared = prepare(features, targets, columns)
    n = len(prepared.rows)
    if fold is None:
        folds, fold_kept = default_folds(n, n_folds)
    else:
        fold_all = np.asarray(fold)
        if fold_all.shape != (len(features),) or not np.issubdtype(fold_all.dtype, np.integer):
            raise ValueError("fold: one integer per row of the features")
        fold_kept = fold_all[prepared.rows].astype(np.int32)
        if fold_kept.min() < 0:
            raise ValueError("fold: a negative fold")
        folds = int(fold_kept.max()) + 1
        if folds > MAX_FOLDS:
            raise ValueError("fold: %d folds; at most %d" % (folds, MAX_FOLDS))
    if regularizations is None:
        if folds == 1:
            raise ValueError("regularizations: without validation (one fold) give the one to use")
        regularizations = default_regularizations()
    reg = np.atleast_1d(np.asarray(regularizations, dtype=np.float64))
    if reg.ndim != 1 or not 1 <= len(reg) <= 256:
        raise ValueError("regularizations: 1 to 256 values")
    if folds == 1 and len(reg) != 1:
        raise ValueError("regularizations: without validation (one fold) there is one")
    raw = fit_problems(prepared.x, prepared.lo, prepared.hi, fold_kept, folds, reg,
                       gram_lambda_max(prepared.x), threshold, max_iterations, device)
    out = PenaltyModelFit()
    out.table = make_table(raw, reg, folds)
    for name in ("weights", "iterations", "criterion", "converged", "incorrect", "hinge", "ms"):
        setattr(out, name, raw[name])
    out.feature_names, out.mean, out.sd = prepared.names, prepared.mean, prepared.sd
    out.rows, out.dropped_rows = prepared.rows, prepared.dropped_rows
    out.dropped_features = prepared.dropped_features
    out.fold, out.n_folds, out.regularizations = fold_kept, folds, reg
    out.x, out.lo, out.hi = prepared.x, prepared.lo, prepared.hi
    chosen = select_regularization(out.table)
    if chosen is None:
        from .api import PeakSegError
        raise PeakSegError(_native.ERROR_FIT_ARGUMENTS, "%s (fit_penalty_model: no regularization has all "
                           "its fits converged within max_iterations = %d at threshold %g)" % (
                               _native.status_message(_native.ERROR_FIT_ARGUMENTS, "<penalty model>", "", ""),
                               int(max_iterations), float(threshold)))
    out.chosen = chosen
    out.regularization = float(reg[chosen])
    out.model = back_transform(raw["weights"][-1, chosen], prepared.names, prepared.mean, prepared.sd)
    return out


_FIT_KEYS = ("columns", "regularizations", "n_folds", "fold", "threshold", "max_iterations")


def _learn(target_call, feature_call, data, labels, target_keys, feature_keys, device, kwargs):
    unknown = set(kwargs) - set(_FIT_KEYS) - set(target_keys) - set(feature_keys)
    if unknown:
        raise TypeError("unexpected keyword arguments: %s" % ", ".join(sorted(unknown)))
    pick = lambda keys: {k: kwargs[k] for k in keys if k in kwargs}  # noqa: E731
    targets = target_call(data, labels, device=device, **pick(target_keys))
    features = feature_call(data, device=device, **pick(feature_keys))
    if not isinstance(targets, list):
        targets = [targets]
    out = fit_penalty_model(features, targets, device=device, **pick(_FIT_KEYS))
    out.targets, out.features = targets, features
    return out


def learn_penalty_model_dense(count_vecs, labels, device=0, **kwargs):
    """Labelled dense coverage in, a fitted penalty model out: targetInterval_dense (keywords width,
    max_rounds, chrom_starts), problem_features_dense and fit_penalty_model (its keywords) in one
    process.  Returns the PenaltyModelFit with .targets (the TargetIntervals) and .features (the
    feature table) attached."""
    from . import api
    return _learn(api.targetInterval_dense, api.problem_features_dense, count_vecs, labels,
                  ("width", "max_rounds", "chrom_starts"), (), device, kwargs)


def learn_penalty_model_reads(reads, labels, device=0, **kwargs):
    """learn_penalty_model_dense with the pile-up in front of it: reads as PeakSegFPOP_reads, the
    keywords extents and bases_counted go to both targetInterval_reads and problem_features_reads."""
    from . import api
    return _learn(api.targetInterval_reads, api.problem_features_reads, reads, labels,
                  ("width", "max_rounds", "extents", "bases_counted"), ("extents", "bases_counted"),
                  device, kwargs)
