"""fit_penalty_model / learn_penalty_model_dense and peakseg_hip_penalty_fit: the interval
regression with an L1 penalty that turns target intervals and coverage features into a
penalty_model, every fit of the regularisation path and of the folds in one launch (DESIGN.md
section 14).

The scenario functions are shared with the emulator rehearsal (tests/test_penalty_fit_emu.py), which
runs them without a GPU; the tests marked gpu run them on the MI355X.

The yardstick never comes from the library: tests/penalty_fit_ref.py recomputes objective, gradient,
criterion and the validation figures in numpy float64 from the weights a call returns.  The
objective is convex, so a subgradient of sup-norm <= threshold at the returned weights certifies them
without comparing against another solver's path.  Inputs come from synthetic.uniform01 (Box-Muller
where normals are wanted): the same on every machine."""
import contextlib
import math

import numpy as np
import pandas as pd
import pytest

import penalty_fit_ref as ref

GPU = pytest.mark.gpu
THRESHOLD = 1e-3


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


def names(p):
    """the package's 36 feature names, and beyond them names of this file's own"""
    from peaksegdisk_amd.grid import FEATURE_NAMES
    return list(FEATURE_NAMES[:p]) + ["wide.%d" % k for k in range(len(FEATURE_NAMES), p)]


@contextlib.contextmanager
def known_names(p):
    """The Python layer takes no column it does not know, and it knows 36; the kernel takes 64.  For
    the fits that are as wide as the kernel, grid.FEATURE_NAMES holds names(p) while they are made,
    so that they go through fit_penalty_model like every other."""
    from peaksegdisk_amd import grid
    kept = grid.FEATURE_NAMES
    grid.FEATURE_NAMES = tuple(names(max(p, len(kept))))
    try:
        yield
    finally:
        grid.FEATURE_NAMES = kept


# ---- inputs -----------------------------------------------------------------------------------

def normals(seed, stream, n):
    from peaksegdisk_amd import synthetic
    u, v = synthetic.uniform01(seed, stream, n), synthetic.uniform01(seed, stream + 1000, n)
    return np.sqrt(-2.0 * np.log(u)) * np.cos(2.0 * math.pi * v)


def raw_features(n, p, seed):
    """a feature table of p columns: for p = 36 the 36 features made as coverage_features makes them
    from nine positive base columns (the logs are collinear, and log(log(v)) is not finite where
    v <= 1: such columns are dropped), else independent columns of different scales"""
    if p == 36:
        base = np.stack([np.exp(1.0 + 0.8 * normals(seed, 10 + k, n)) for k in range(9)], axis=1)
        with np.errstate(all="ignore"):
            table = np.hstack([base, np.log(base + 1), np.log(base), np.log(np.log(base))])
    else:
        table = np.stack([(1.0 + k) * normals(seed, 10 + k, n) + 3.0 * k for k in range(p)], axis=1)
    return pd.DataFrame(table, columns=names(p))


def targets_for(frame, seed):
    """intervals around a linear function of the first two columns plus noise: a third of the rows
    without lower limit, a third without upper limit, the rest with both"""
    from peaksegdisk_amd import synthetic
    n = len(frame)
    z = frame.iloc[:, 0].to_numpy()
    z = (z - z.mean()) / z.std(ddof=1)
    centre = 1.0 + 0.8 * z + 0.5 * normals(seed, 50, n)
    if frame.shape[1] > 1:
        z1 = frame.iloc[:, 1].to_numpy()
        centre = centre - 0.5 * (z1 - z1.mean()) / z1.std(ddof=1)
    below = 0.2 + 1.3 * synthetic.uniform01(seed, 51, n)
    above = 0.2 + 1.3 * synthetic.uniform01(seed, 52, n)
    lo, hi = centre - below, centre + above
    lo[np.arange(n) % 3 == 0] = -np.inf
    hi[np.arange(n) % 3 == 1] = np.inf
    return np.stack([lo, hi], axis=1)


SHAPES = {                       # (n, p, F, regularizations)
    "2x1": (2, 1, 2, [0.05]),
    "63x3": (63, 3, 5, [0.01, 0.05, 0.2, 5.0]),
    "65x36": (65, 36, 5, [0.02, 0.05, 0.2, 5.0]),
    "257x5": (257, 5, 3, [0.01, 0.05, 0.2, 5.0]),
    "1000x12": (1000, 12, 16, [0.01, 0.1, 1.0]),
    # as wide as the kernel: every lane of wave 0 has a weight, the intercept is slot 64; one less
    "300x64": (300, 64, 5, [0.02, 0.05, 0.2, 5.0]),
    "301x63": (301, 63, 5, [0.02, 0.05, 0.2, 5.0]),
}
_FITS = {}


def fitted(psd, key):
    """the fit of a shape, made once per library (the emulator's and the device's)"""
    at = (id(_lib()), key)
    if at not in _FITS:
        n, p, folds, reg = SHAPES[key]
        frame = raw_features(n, p, 100 + n)
        targets = targets_for(frame, 200 + n)
        with known_names(p):
            fit = psd.fit_penalty_model(frame, targets, regularizations=reg, n_folds=folds,
                                        threshold=THRESHOLD)
        _FITS[at] = (frame, targets, fit)
    return _FITS[at]


def standardised(frame, fit):
    """the standardised matrix of the columns and rows the fit kept, computed here"""
    raw = frame[fit.feature_names].to_numpy(dtype=np.float64)[fit.rows]
    mean, sd = raw.mean(axis=0), raw.std(axis=0, ddof=1)
    assert np.allclose(mean, fit.mean, rtol=1e-12, atol=1e-12) and np.allclose(sd, fit.sd, rtol=1e-12)
    return (raw - mean) / sd


def train_mask(fit, s):
    sets = fit.weights.shape[0]
    return np.ones(len(fit.fold), bool) if s == sets - 1 else fit.fold != s


def check_certificate(frame, targets, fit, what):
    """every problem converged, and the criterion recomputed from its weights is <= threshold (+1e-9:
    the reordering of sums of at most 13000 terms of size about 10 in float64: below 1e-10) and equals the
    reported one within 1e-9"""
    x = standardised(frame, fit)
    lo, hi = targets[fit.rows, 0], targets[fit.rows, 1]
    sets, k, width = fit.weights.shape
    assert sets == (fit.n_folds + 1 if fit.n_folds > 1 else 1) and width == x.shape[1] + 1
    assert k == len(fit.regularizations)
    for s in range(sets):
        mask = train_mask(fit, s)
        for j in range(k):
            w, b = fit.weights[s, j, :-1], fit.weights[s, j, -1]
            c = ref.criterion(x, lo, hi, mask, w, b, fit.regularizations[j])
            print(what, s, j, "criterion", c, "reported", fit.criterion[s, j], "iterations",
                  fit.iterations[s, j])
            assert fit.converged[s, j] == 1, (what, s, j)
            assert c <= THRESHOLD + 1e-9, (what, s, j, c)
            assert abs(c - fit.criterion[s, j]) <= 1e-9, (what, s, j, c, fit.criterion[s, j])
            assert 0 <= fit.iterations[s, j] <= 100000
    return x, lo, hi


def raw_fit(x, lo, hi, fold, folds, reg, lambda_max, threshold=THRESHOLD, max_iterations=1000):
    """peakseg_hip_penalty_fit as it is: x (n, p) standardised -> (status, weights, converged)"""
    x = np.asarray(x, np.float64)
    n, p = x.shape
    x_fm = np.ascontiguousarray(x.T)
    lo, hi = np.ascontiguousarray(lo, np.float64), np.ascontiguousarray(hi, np.float64)
    fold = np.ascontiguousarray(fold, np.int32)
    reg = np.ascontiguousarray(reg, np.float64)
    sets = 1 if folds == 1 else max(folds, 0) + 1
    weights = np.zeros((sets, max(len(reg), 1), p + 1))
    converged = np.zeros((sets, max(len(reg), 1)), np.int32)
    st = _lib().peakseg_hip_penalty_fit(
        0, n, p, x_fm.ctypes.data, lo.ctypes.data, hi.ctypes.data, fold.ctypes.data, folds, len(reg),
        reg.ctypes.data, lambda_max, threshold, max_iterations, weights.ctypes.data, None, None,
        converged.ctypes.data, None, None)
    return st, weights, converged


# ---- scenario 1: closed form, intercept only --------------------------------------------------

def scenario_intercept_only(psd):
    """rows (-inf, 0] and [2, +inf) and a constant column: the loss is ((b + 1)^2 + (b - 3)^2) / 2,
    least at b = 1 with derivative 2 b - 2, so a criterion <= threshold puts b within threshold / 2"""
    frame = pd.DataFrame({names(1)[0]: [4.0, 4.0]})
    targets = np.array([[-np.inf, 0.0], [2.0, np.inf]])
    fit = psd.fit_penalty_model(frame, targets, regularizations=[0.1], n_folds=1, threshold=THRESHOLD)
    assert fit.dropped_features == {names(1)[0]: "constant"} and fit.feature_names == []
    assert fit.weights.shape == (1, 1, 1) and fit.converged[0, 0] == 1
    b = fit.weights[0, 0, 0]
    print("intercept", b, "iterations", fit.iterations[0, 0])
    assert abs(b - 1.0) <= THRESHOLD / 2
    assert fit.model == {"intercept": b, "weights": {}} and fit.regularization == 0.1
    assert psd.predict_penalties(frame, fit.model).tolist() == [float(psd.paste(math.exp(b)))] * 2
    assert fit.ms >= 0.0 and fit.dropped_rows == []


# ---- scenario 2: closed form, lasso -----------------------------------------------------------

def scenario_lasso_closed_form(psd):
    """Four rows, the orthogonal columns x1 = [1, 1, -1, -1] and x2 = [1, -1, 1, -1], point targets
    lo = hi = y = 5 + 0.5 x1 + 0.1 x2.  Both columns have mean 0 and sd^2 = 4 / 3, so the
    standardised columns x~_j = x_j sqrt(3) / 2 are orthogonal to each other and to the ones, with
    x~_j . x~_j = n - 1 = 3.  Where every residual |f_i - y_i| < 1 both hinges of a row are active:
    phi(f - y) + phi(y - f) = (f - y - 1)^2 + (y - f - 1)^2 = 2 (f - y)^2 + 2, and the objective is
    (2 / n) |f - y|^2 + 2 + reg |w|_1.  By orthogonality it separates: in b it is 2 (b - mean y)^2 +
    const, least at b = mean(y) with curvature 4; in w_j it is (2 (n - 1) / n) (w_j - a_j)^2 +
    reg |w_j| + const with a_j = x~_j . y / (n - 1), curvature 4 (n - 1) / n, least at
    w_j = S(a_j, reg n / (4 (n - 1))), S(a, k) = sign(a) max(|a| - k, 0).  A subgradient of size c
    in a coordinate of curvature h puts it within c / h of the minimiser: |w_j - w*_j| <=
    threshold n / (4 (n - 1)) and |b - b*| <= threshold / 4; where the formula gives zero the
    returned weight is zero exactly (the prox step sets it, and the criterion accepts it).
    Here a = (0.5774, 0.1155) and the threshold of S is reg / 3: both weights are zero at reg = 5 and
    none at 0.01 and at 0.3 (0.1155 > 0.1: the second weight is 0.0155 there, small but not zero);
    reg = 0.4 is added for the mixed case, the second weight zero and the first not."""
    n = 4
    x1, x2 = np.array([1.0, 1, -1, -1]), np.array([1.0, -1, 1, -1])
    y = 5.0 + 0.5 * x1 + 0.1 * x2
    frame = pd.DataFrame({names(2)[0]: x1, names(2)[1]: x2})
    targets = np.stack([y, y], axis=1)
    xs = np.stack([x1, x2], axis=1) * math.sqrt(3.0) / 2.0
    a = xs.T @ y / (n - 1)
    for reg in (0.01, 0.3, 0.4, 5.0):
        fit = psd.fit_penalty_model(frame, targets, regularizations=[reg], n_folds=1, threshold=THRESHOLD)
        assert fit.weights.shape == (1, 1, 3) and fit.converged[0, 0] == 1
        w, b = fit.weights[0, 0, :2], fit.weights[0, 0, 2]
        want = ref.soft(a, reg * n / (4.0 * (n - 1)))
        print("reg", reg, "w", w, "want", want, "b", b, "iterations", fit.iterations[0, 0])
        assert np.all(np.abs(ref.predict(xs, w, b) - y) < 1.0)
        assert np.all(np.abs(w - want) <= THRESHOLD * n / (4.0 * (n - 1)))
        assert abs(b - y.mean()) <= THRESHOLD / 4
        assert np.array_equal(w == 0.0, want == 0.0)
        assert (want == 0.0).tolist() == {0.01: [False, False], 0.3: [False, False], 0.4: [False, True],
                                            5.0: [True, True]}[reg]
        assert sorted(fit.model["weights"]) == sorted(np.array(names(2))[want != 0.0].tolist())


# ---- scenario 3: the certificate on every problem of a path -----------------------------------

def scenario_certificate(psd):
    for key in SHAPES:
        frame, targets, fit = fitted(psd, key)
        n, p, folds, reg = SHAPES[key]
        assert fit.n_folds == folds and len(fit.rows) == n and fit.dropped_rows == []
        if p == 36:       # log(log(v)) of a v <= 1
            assert set(fit.dropped_features.values()) == {"not finite"}
            assert 20 <= len(fit.feature_names) < 36
        else:       # the width reaches the kernel
            assert fit.feature_names == names(p) and fit.dropped_features == {}
            assert len(fit.feature_names) == p and fit.weights.shape[2] == p + 1
        lo, hi = targets[:, 0], targets[:, 1]
        assert np.all(np.isinf(lo[0::3])) and np.all(np.isinf(hi[1::3])) and np.all(np.isfinite(targets[2::3]))
        check_certificate(frame, targets, fit, key)
        assert np.all(np.isfinite(fit.weights)) and np.all(np.isfinite(fit.hinge))


# ---- scenario 4: the objective against the host solver ----------------------------------------

def scenario_objective(psd):
    """F_dev - F_ref <= threshold (|w_dev - w_ref|_1 + |b_dev - b_ref|) + 1e-9: the first-order bound
    of a convex function whose subgradient at w_dev has sup-norm at most threshold"""
    for key in ("63x3", "257x5", "300x64"):
        frame, targets, fit = fitted(psd, key)
        x = standardised(frame, fit)
        assert x.shape[1] == SHAPES[key][1]
        lo, hi = targets[fit.rows, 0], targets[fit.rows, 1]
        lam = ref.gram_lambda_max(x)
        for s in range(fit.weights.shape[0]):
            mask = train_mask(fit, s)
            for j, reg in enumerate(fit.regularizations):
                w, b = fit.weights[s, j, :-1], fit.weights[s, j, -1]
                rw, rb, its, c = ref.fista(x, lo, hi, mask, reg, lam, 1e-9)
                assert c <= 1e-9, (key, s, j, its, c)
                gap = ref.objective(x, lo, hi, mask, w, b, reg) - ref.objective(x, lo, hi, mask, rw, rb, reg)
                bound = THRESHOLD * (float(np.sum(np.abs(w - rw))) + abs(b - rb)) + 1e-9
                print(key, s, j, "gap", gap, "bound", bound)
                assert gap <= bound, (key, s, j, gap, bound)


# ---- scenario 5: validation counts and the selection ------------------------------------------

def expected_choice(table):
    """the rule of DESIGN.md section 14 on the table: converged only; fewest validation.incorrect,
    then the smaller validation.hinge, then the larger regularization"""
    rows = [(int(r["validation.incorrect"]), float(r["validation.hinge"]), -float(r["regularization"]), k)
            for k, (_, r) in enumerate(table.iterrows()) if bool(r["converged"])]
    return min(rows)[3]


def scenario_validation_and_selection(psd):
    for key in ("63x3", "257x5", "1000x12"):
        frame, targets, fit = fitted(psd, key)
        x = standardised(frame, fit)
        lo, hi = targets[fit.rows, 0], targets[fit.rows, 1]
        sets, k, _ = fit.weights.shape
        for s in range(sets):
            for j in range(k):     # no prediction within 1e-9 of a limit: the counts are unambiguous
                assert ref.limit_distance(x, lo, hi, fit.weights[s, j, :-1], fit.weights[s, j, -1]) > 1e-9
        for s in range(sets):
            rows = np.ones(len(lo), bool) if s == sets - 1 else fit.fold == s
            for j in range(k):
                w, b = fit.weights[s, j, :-1], fit.weights[s, j, -1]
                assert fit.incorrect[s, j] == ref.incorrect(x, lo, hi, rows, w, b), (key, s, j)
                want = ref.hinge(x, lo, hi, rows, w, b)
                assert abs(fit.hinge[s, j] - want) <= 1e-9 * max(1.0, want), (key, s, j)
        table = fit.table
        assert list(table.columns) == ["regularization", "validation.incorrect", "validation.hinge",
                                       "train.incorrect", "nonzero", "iterations", "converged"]
        assert table["regularization"].tolist() == list(fit.regularizations)
        assert table["validation.incorrect"].tolist() == fit.incorrect[:-1].sum(axis=0).tolist()
        assert table["train.incorrect"].tolist() == fit.incorrect[-1].tolist()
        assert table["nonzero"].tolist() == np.count_nonzero(fit.weights[-1][:, :-1], axis=1).tolist()
        assert table["iterations"].tolist() == fit.iterations.max(axis=0).tolist()
        assert table["converged"].tolist() == [True] * k
        chosen = expected_choice(table)
        assert fit.regularization == fit.regularizations[chosen] and fit.chosen == chosen
        w, b = fit.weights[-1, chosen, :-1], fit.weights[-1, chosen, -1]
        weights = {name: w[j] / fit.sd[j] for j, name in enumerate(fit.feature_names) if w[j] != 0.0}
        intercept = b - sum(w[j] * fit.mean[j] / fit.sd[j] for j in range(len(w)) if w[j] != 0.0)
        assert fit.model["weights"] == weights and len(weights) == table["nonzero"].iloc[chosen]
        assert abs(fit.model["intercept"] - intercept) <= 1e-12 * max(1.0, abs(intercept))
        psd.predict_penalties(frame, fit.model)
        if key != "1000x12":
            # the largest regularization leaves no weight and makes strictly more validation errors
            # than the chosen one: a selection that did not read the table would not pass
            assert table["nonzero"].iloc[-1] == 0 and chosen != k - 1
            assert table["validation.incorrect"].iloc[-1] > table["validation.incorrect"].iloc[chosen]


# ---- scenario 6: reproducibility --------------------------------------------------------------

def scenario_reproducible(psd):
    frame, targets, first = fitted(psd, "1000x12")
    n, p, folds, reg = SHAPES["1000x12"]
    again = psd.fit_penalty_model(frame, targets, regularizations=reg, n_folds=folds, threshold=THRESHOLD)
    for name in ("weights", "iterations", "criterion", "converged", "incorrect", "hinge"):
        assert getattr(first, name).tobytes() == getattr(again, name).tobytes(), name
    assert first.model == again.model


# ---- scenario 7: the caller's folds -----------------------------------------------------------

def scenario_own_folds(psd):
    n, p = 65, 3
    frame = raw_features(n, p, 7)
    targets = targets_for(frame, 8)
    fold = np.array([0] * 40 + [1] * 24 + [2], dtype=np.int64)       # unequal, one of a single row
    fit = psd.fit_penalty_model(frame, targets, regularizations=[0.02, 0.3], fold=fold, threshold=THRESHOLD)
    assert fit.n_folds == 3 and fit.fold.tolist() == fold.tolist() and fit.weights.shape == (4, 2, 4)
    x, lo, hi = check_certificate(frame, targets, fit, "own folds")
    # the masks matter: the weights of a fold are no certificate for another training set
    c = ref.criterion(x, lo, hi, fit.fold != 1, fit.weights[0, 0, :-1], fit.weights[0, 0, -1], 0.02)
    assert c > THRESHOLD + 1e-9
    assert fit.incorrect[2, 0] in (0, 1)          # the fold of a single row


# ---- scenario 8: not converged ----------------------------------------------------------------

def scenario_not_converged(psd):
    n, p, folds, reg = SHAPES["63x3"]
    frame = raw_features(n, p, 100 + n)
    targets = targets_for(frame, 200 + n)
    from peaksegdisk_amd import fit as fit_module
    prepared = fit_module.prepare(frame, targets)
    raw = fit_module.fit_problems(prepared.x, prepared.lo, prepared.hi, fit_module.default_folds(n, folds)[1],
                                  folds, reg, fit_module.gram_lambda_max(prepared.x), THRESHOLD, 3)
    assert not raw["converged"].any() and (raw["iterations"] == 3).all()
    assert np.all(np.isfinite(raw["criterion"])) and np.all(raw["criterion"] > THRESHOLD)
    for s in range(folds + 1):      # the criterion is that of the weights returned
        mask = np.ones(n, bool) if s == folds else fit_module.default_folds(n, folds)[1] != s
        for j in range(len(reg)):
            c = ref.criterion(prepared.x, prepared.lo, prepared.hi, mask, raw["weights"][s, j, :-1],
                              raw["weights"][s, j, -1], reg[j])
            assert abs(c - raw["criterion"][s, j]) <= 1e-9
    with pytest.raises(psd.PeakSegError) as ei:
        psd.fit_penalty_model(frame, targets, regularizations=reg, n_folds=folds, max_iterations=3)
    assert ei.value.status == 21 and "converged" in str(ei.value)


# ---- scenario 9: arguments --------------------------------------------------------------------

def scenario_arguments(psd):
    from peaksegdisk_amd import _native
    assert _native.ERROR_FIT_ARGUMENTS == 21
    text = _native.status_message(21, "f", "1", "d")
    assert text.startswith("error code 21") and "penalty model" in text
    assert _lib().peakseg_hip_penalty_fit_max_features() == 64
    n = 12
    x = np.stack([normals(3, 1, n), normals(3, 2, n)], axis=1)
    x = (x - x.mean(axis=0)) / x.std(axis=0, ddof=1)
    lo, hi = x[:, 0] - 0.5, x[:, 0] + 0.5
    lo[0], hi[1] = -np.inf, np.inf
    fold = (np.arange(n) % 3).astype(np.int32)
    lam = ref.gram_lambda_max(x)
    good = dict(x=x, lo=lo, hi=hi, fold=fold, folds=3, reg=[0.1, 0.2], lambda_max=lam)

    def call(**change):
        args = dict(good)
        args.update(change)
        st = raw_fit(**args)[0]
        return st, _lib().peakseg_hip_last_error().decode()

    def spoiled(array, at, value):
        out = np.array(array, dtype=np.float64 if array.dtype != np.int32 else np.int32)
        out[at] = value
        return out

    refusals = [
        (dict(x=x[:1], lo=lo[:1], hi=hi[:1], fold=fold[:1]), "n = 1"),
        (dict(x=np.zeros((n, 65))), "p = 65"),
        (dict(folds=0), "n_folds = 0"),
        (dict(folds=17), "n_folds = 17"),
        (dict(reg=[]), "n_reg = 0"),
        (dict(reg=np.arange(1, 258) * 0.01), "n_reg = 257"),
        (dict(folds=1, fold=np.zeros(n, np.int32)), "n_folds = 1"),
        (dict(x=spoiled(x, (5, 1), np.inf)), "row 5"),
        (dict(x=spoiled(x, (7, 0), np.nan)), "row 7"),
        (dict(lo=spoiled(lo, 3, np.nan)), "row 3"),
        (dict(hi=spoiled(hi, 4, np.nan)), "row 4"),
        (dict(lo=spoiled(lo, 6, 2.0)), "row 6"),
        (dict(hi=spoiled(hi, 0, np.inf)), "row 0"),
        (dict(fold=spoiled(fold, 9, 3)), "row 9"),
        (dict(fold=spoiled(fold, 2, -1)), "row 2"),
        (dict(fold=np.ones(n, np.int32)), "fold 1"),
        (dict(reg=[0.2, 0.2]), "reg[1]"),
        (dict(reg=[0.2, 0.1]), "reg[1]"),
        (dict(reg=[-0.1, 0.1]), "reg[0]"),
        (dict(reg=[0.1, np.nan]), "reg[1]"),
        (dict(lambda_max=0.0), "gram_lambda_max"),
        (dict(lambda_max=-1.0), "gram_lambda_max"),
        (dict(threshold=0.0), "threshold"),
        (dict(max_iterations=0), "max_iterations"),
    ]
    for change, needle in refusals:
        st, text = call(**change)
        assert st == 21 and needle in text, (needle, st, text)
    st, weights, converged = raw_fit(**good)
    assert st == 0 and converged.all() and weights.shape == (4, 2, 3)
    # the Python layer's own checks
    frame = raw_features(n, 2, 5)
    targets = np.stack([lo, hi], axis=1)
    with pytest.raises(ValueError, match="unknown feature"):
        psd.fit_penalty_model(frame, targets, columns=["no.such.feature"])
    with pytest.raises(ValueError, match="targets"):
        psd.fit_penalty_model(frame, targets[:-1])
    silent = np.full((n, 2), [-np.inf, np.inf])
    silent[4] = [0.0, 1.0]
    with pytest.raises(ValueError, match="at least two"):
        psd.fit_penalty_model(frame, silent)
    with pytest.raises(ValueError):
        psd.fit_penalty_model(frame, targets, regularizations=[0.1, 0.2], n_folds=1)
    with pytest.raises(ValueError):
        psd.fit_penalty_model(frame, targets, n_folds=17)
    with known_names(65):           # one column more than the kernel takes
        with pytest.raises(ValueError, match="65 features; at most 64"):
            psd.fit_penalty_model(raw_features(n, 65, 5), targets)
    # rows that say nothing and columns that are not finite or constant: dropped and reported
    wide = raw_features(n, 4, 5)
    wide.iloc[3, 2] = np.nan
    wide.iloc[:, 3] = 2.5
    some = targets.copy()
    some[5] = [-np.inf, np.inf]
    some[10] = [-np.inf, np.inf]
    wide.iloc[10, 1] = np.inf        # (in a dropped row: the column stays)
    fit = psd.fit_penalty_model(wide, some, regularizations=[0.05, 0.5], n_folds=3, threshold=THRESHOLD)
    assert fit.dropped_rows == [5, 10] and fit.rows.tolist() == [i for i in range(n) if i not in (5, 10)]
    assert fit.dropped_features == {names(4)[2]: "not finite", names(4)[3]: "constant"}
    assert fit.feature_names == names(2) and fit.fold.tolist() == [i % 3 for i in range(n - 2)]
    check_certificate(wide, some, fit, "dropped")


# ---- scenario 10: more rows than a chunk ------------------------------------------------------

def scenario_chunks(psd):
    """The kernel goes over the rows in chunks (6144): one row more than a chunk, and more than two
    chunks.  The certificate, the counts and the hinge of every problem."""
    for n in (6145, 13000):
        frame = raw_features(n, 3, 300 + n)
        targets = targets_for(frame, 400 + n)
        fit = psd.fit_penalty_model(frame, targets, regularizations=[0.02, 0.3], n_folds=2,
                                    threshold=THRESHOLD)
        assert fit.weights.shape == (3, 2, 4) and len(fit.rows) == n
        x, lo, hi = check_certificate(frame, targets, fit, "chunks %d" % n)
        for s in range(3):
            rows = np.ones(n, bool) if s == 2 else fit.fold == s
            for j in range(2):
                w, b = fit.weights[s, j, :-1], fit.weights[s, j, -1]
                assert np.any(w != 0.0)
                assert ref.limit_distance(x, lo, hi, w, b) > 1e-9
                assert fit.incorrect[s, j] == ref.incorrect(x, lo, hi, rows, w, b), (n, s, j)
                want = ref.hinge(x, lo, hi, rows, w, b)
                assert abs(fit.hinge[s, j] - want) <= 1e-9 * max(1.0, want), (n, s, j)


SCENARIOS = [scenario_intercept_only, scenario_lasso_closed_form, scenario_certificate,
             scenario_objective, scenario_validation_and_selection, scenario_reproducible,
             scenario_own_folds, scenario_not_converged, scenario_arguments, scenario_chunks]


# ---- scenario 11: end to end (MI355X only: the emulator cannot afford the searches) -----------

def generating_segments(n, seed):
    """the segments poisson_coverage(n, seed) draws its rates from: (start, end, is_peak) in bases.
    This repeats the first lines of synthetic.poisson_coverage (n_seg, the lengths from stream 1 with
    means 200 and 2000, odd segments peaks) and must follow them if they change; scenario_end_to_end
    checks that the labels it leads to still separate peak from background coverage."""
    from peaksegdisk_amd import synthetic
    n_seg = max(16, int(n / 1100.0 * 1.5) + 16)
    u_len = synthetic.uniform01(seed, 1, n_seg)
    is_peak = (np.arange(n_seg) % 2) == 1
    q = 1.0 / np.where(is_peak, 200.0, 2000.0)
    length = 1 + np.floor(np.log(u_len) / np.log1p(-q)).astype(np.int64)
    assert int(length.sum()) >= n
    end = np.cumsum(length)
    return [(int(e - ln), int(min(e, n)), bool(pk)) for e, ln, pk in zip(end, length, is_peak) if e - ln < n]


def labels_for(n, seed):
    """two to four labels on the generating segments: noPeaks inside a background segment, peaks
    around a peak segment that lies inside the contig"""
    start, end, kind = [], [], []
    for s, e, is_peak in generating_segments(n, seed):
        if len(start) == 4:
            break
        if is_peak and e - s >= 20 and s >= 10 and e + 10 <= n:
            start, end, kind = start + [s - 5], end + [e + 5], kind + ["peaks"]
        elif not is_peak and e - s >= 80:
            quarter = (e - s) // 4
            start, end, kind = start + [s + quarter], end + [e - quarter], kind + ["noPeaks"]
    if len(start) == 1:          # one long background segment: two labels on it
        middle = (start[0] + end[0]) // 2
        start, end, kind = [start[0], middle + 1], [middle, end[0]], [kind[0]] * 2
    assert 2 <= len(start) <= 4
    return (np.array(start, np.int32), np.array(end, np.int32), kind)


def scenario_end_to_end(psd):
    from peaksegdisk_amd import synthetic
    sizes = [2000, 2300, 2600, 2900, 3200, 3500, 3800, 4000]
    vectors = [synthetic.poisson_coverage(n, seed=60 + k)[2].astype(np.int32) for k, n in enumerate(sizes)]
    labels = [labels_for(n, 60 + k) for k, n in enumerate(sizes)]
    inside = {"peaks": [], "noPeaks": []}       # the generator still puts its peaks where the labels say
    for v, (start, end, kind) in zip(vectors, labels):
        for s, e, a in zip(start.tolist(), end.tolist(), kind):
            inside[a].append(float(v[s + (5 if a == "peaks" else 0):e - (5 if a == "peaks" else 0)].mean()))
    assert inside["peaks"] and min(inside["peaks"]) > 2.0 > max(inside["noPeaks"])
    fit = psd.learn_penalty_model_dense(vectors, labels, n_folds=4,
                                        regularizations=0.001 * 1.2 ** np.arange(0, 64, 4))
    assert len(fit.targets) == 8 and len(fit.features) == 8
    predicted = psd.predict_penalties(fit.features, fit.model)
    assert len(predicted) == 8 and np.all(np.isfinite(predicted)) and np.all(predicted > 0)
    outside = sum(1 for t, p in zip(fit.targets, predicted)
                  if not (t.min_log_lambda <= math.log(p) <= t.max_log_lambda))
    assert outside == int(fit.table["train.incorrect"].iloc[fit.chosen])
    results = psd.PeakSegFPOP_dense(vectors, penalty_model=fit.model, labels=labels)
    assert len(results) == 8
    for c, result in enumerate(results):
        assert len(result) == 1 and len(result[0].segments) >= 1
        assert len(result[0].label_errors) == len(labels[c][0])
        assert float(result[0].loss["penalty"].iloc[0]) == predicted[c]


# ---- MI355X -----------------------------------------------------------------------------------

@GPU
@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__[len("scenario_"):])
def test_gpu_penalty_fit(psd, scenario):
    scenario(psd)


@GPU
def test_gpu_penalty_fit_end_to_end(psd):
    scenario_end_to_end(psd)
