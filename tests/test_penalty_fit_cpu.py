"""The host side of the penalty-model fits, without a GPU and without the emulator: the
preprocessing and the selection of peaksegdisk_amd/fit.py, the yardstick's own gradient
(tests/penalty_fit_ref.py) against central differences, and the new names of the C ABI."""
import ctypes
import math

import numpy as np
import pandas as pd
import pytest

import penalty_fit_ref as ref


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as entry
    entry.build_hip()
    from peaksegdisk_amd import _native
    return _native


def names(p):
    from peaksegdisk_amd.grid import FEATURE_NAMES
    return list(FEATURE_NAMES[:p])


def uniforms(stream, n):
    from peaksegdisk_amd import synthetic
    return synthetic.uniform01(11, stream, n)


def test_names_and_status(native):
    import peaksegdisk_amd
    assert native.ERROR_FIT_ARGUMENTS == 21
    for name in ("fit_penalty_model", "learn_penalty_model_dense", "learn_penalty_model_reads",
                 "PenaltyModelFit"):
        assert name in peaksegdisk_amd.__all__ and hasattr(peaksegdisk_amd, name)
    for name in ("peakseg_hip_penalty_fit", "peakseg_hip_penalty_fit_last_ms",
                 "peakseg_hip_penalty_fit_max_features"):
        assert hasattr(native.lib, name) and name in native.EXPORTED_SYMBOLS
    assert native.lib.peakseg_hip_penalty_fit_max_features() == 64
    text = native.status_message(21, "f", "1", "d")
    assert text.startswith("error code 21") and "penalty model" in text and "converged" in text


def test_refusals_come_before_the_device(native):
    """the argument checks are the host's: status 21 whether or not a GPU is visible"""
    x = np.ascontiguousarray(np.array([[-1.0, 0.0, 1.0, 0.5]]))
    lo, hi = np.array([0.0, -np.inf, 1.0, 2.0]), np.array([1.0, 2.0, np.inf, 3.0])
    fold = np.array([0, 1, 0, 1], np.int32)
    reg = np.array([0.1, 0.2])

    def call(lo=lo, hi=hi, folds=2, lam=5.0):
        st = native.lib.peakseg_hip_penalty_fit(
            0, 4, 1, x.ctypes.data, lo.ctypes.data, hi.ctypes.data, fold.ctypes.data, folds, 2,
            reg.ctypes.data, lam, 1e-3, 10, None, None, None, None, None, None)
        return st, native.lib.peakseg_hip_last_error().decode()
    st, text = call(lo=np.array([0.0, -np.inf, 1.0, 4.0]))
    assert st == 21 and "row 3" in text and "exceeds" in text
    st, text = call(hi=np.array([1.0, np.inf, np.inf, 3.0]))
    assert st == 21 and "row 1" in text and "infinite" in text
    st, text = call(folds=1)
    assert st == 21 and "n_folds = 1" in text
    st, text = call(lam=0.0)
    assert st == 21 and "gram_lambda_max" in text
    st, _ = call()
    assert st == (0 if native.lib.peakseg_hip_device_count() >= 1 else native.ERROR_NO_HIP_DEVICE)
    ms = ctypes.c_float(-1.0)
    assert native.lib.peakseg_hip_penalty_fit_last_ms(ctypes.byref(ms)) == 0 and ms.value >= 0.0


def test_prepare_drops_standardises_and_reports(native):
    from peaksegdisk_amd import fit
    n = 9
    frame = pd.DataFrame({name: 10.0 * (k + 1) * uniforms(k, n) + k for k, name in enumerate(names(5))})
    frame.iloc[2, 1] = -np.inf          # not finite in a kept row
    frame.iloc[:, 3] = 7.0              # constant
    frame.iloc[6, 4] = np.nan           # not finite, but only in a row that is dropped
    targets = np.array([[0.0, 1.0]] * n)
    targets[0] = [-np.inf, 2.0]
    targets[6] = [-np.inf, np.inf]
    p = fit.prepare(frame, targets)
    assert p.rows.tolist() == [0, 1, 2, 3, 4, 5, 7, 8] and p.dropped_rows == [6]
    assert p.dropped_features == {names(5)[1]: "not finite", names(5)[3]: "constant"}
    assert p.names == [names(5)[0], names(5)[2], names(5)[4]]
    raw = frame[p.names].to_numpy()[p.rows]
    # (numpy's sums take their order from the memory layout: the last bits may differ)
    assert np.allclose(p.mean, raw.mean(axis=0), rtol=1e-14, atol=0)
    assert np.allclose(p.sd, raw.std(axis=0, ddof=1), rtol=1e-14, atol=0)
    assert np.array_equal(p.x, (raw - p.mean) / p.sd)
    assert np.allclose(p.x.mean(axis=0), 0.0, atol=1e-14) and np.allclose(p.x.std(axis=0, ddof=1), 1.0)
    assert p.lo.tolist() == targets[p.rows, 0].tolist() and p.hi.tolist() == targets[p.rows, 1].tolist()
    # columns: a subset in the caller's order; names outside FEATURE_NAMES are refused
    q = fit.prepare(frame, targets, columns=[names(5)[2], names(5)[0]])
    assert q.names == [names(5)[2], names(5)[0]] and np.array_equal(q.x, p.x[:, [1, 0]])
    with pytest.raises(ValueError, match="unknown feature"):
        fit.prepare(frame.assign(extra=1.0), targets, columns=["extra"])
    with pytest.raises(ValueError, match="targets"):
        fit.prepare(frame, targets[:-1])
    with pytest.raises(ValueError, match="at least two"):
        fit.prepare(frame, np.array([[0.0, 1.0]] + [[-np.inf, np.inf]] * (n - 1)))
    with pytest.raises(ValueError, match="exceeds"):
        fit.prepare(frame, np.array([[2.0, 1.0]] * n))
    # every column dropped: an intercept-only model is legal
    r = fit.prepare(frame[[names(5)[3]]], targets)
    assert r.names == [] and r.x.shape == (8, 0)
    # a list of TargetInterval
    from peaksegdisk_amd.target import TargetInterval
    intervals = [TargetInterval(lo, hi, True, True, 0, 1, None) for lo, hi in targets.tolist()]
    assert np.array_equal(fit.target_limits(intervals), targets)


def test_default_folds_and_grid(native):
    from peaksegdisk_amd import fit
    folds, fold = fit.default_folds(12)
    assert folds == 5 and fold.dtype == np.int32 and fold.tolist() == [i % 5 for i in range(12)]
    assert fit.default_folds(3)[0] == 3 and fit.default_folds(3)[1].tolist() == [0, 1, 2]
    assert fit.default_folds(40, 16)[0] == 16
    for bad in (0, 17, 2.5):
        with pytest.raises(ValueError):
            fit.default_folds(10, bad)
    grid = fit.default_regularizations()
    assert len(grid) == 64 and grid[0] == 0.001 and np.all(np.diff(grid) > 0)
    assert np.allclose(grid[1:] / grid[:-1], 1.2) and abs(grid[-1] - 0.001 * 1.2 ** 63) < 1e-9


def test_selection_rule_on_a_table(native):
    from peaksegdisk_amd import fit

    def table(rows):
        return pd.DataFrame(rows, columns=["regularization", "validation.incorrect", "validation.hinge",
                                           "converged"])
    # fewest incorrect wins over a smaller hinge
    assert fit.select_regularization(table([[0.1, 3, 0.5, True], [0.2, 2, 9.0, True], [0.3, 4, 0.1, True]])) == 1
    # ties: the smaller hinge
    assert fit.select_regularization(table([[0.1, 2, 0.5, True], [0.2, 2, 0.4, True], [0.3, 2, 0.6, True]])) == 1
    # ties again: the larger regularization
    assert fit.select_regularization(table([[0.1, 2, 0.5, True], [0.2, 2, 0.5, True], [0.3, 3, 0.5, True]])) == 1
    # a regularization whose fits did not all converge takes no part
    assert fit.select_regularization(table([[0.1, 0, 0.0, False], [0.2, 5, 1.0, True]])) == 1
    assert fit.select_regularization(table([[0.1, 0, 0.0, False], [0.2, 5, 1.0, False]])) is None


def test_make_table(native):
    from peaksegdisk_amd import fit
    raw = {"incorrect": np.array([[1, 2], [3, 4], [5, 6]]), "hinge": np.array([[.5, 1.], [.25, 2.], [9., 9.]]),
           "weights": np.array([[[0, 0, 1.], [0, 0, 1.]], [[0, 0, 1.], [0, 0, 1.]], [[2., 0, 1.], [0, 0, 0.]]]),
           "iterations": np.array([[8, 16], [24, 8], [8, 8]]), "converged": np.array([[1, 1], [1, 0], [1, 1]])}
    t = fit.make_table(raw, [0.1, 0.2], 2)
    assert list(t.columns) == fit.TABLE_COLUMNS
    assert t["validation.incorrect"].tolist() == [4, 6] and t["validation.hinge"].tolist() == [0.75, 3.0]
    assert t["train.incorrect"].tolist() == [5, 6] and t["nonzero"].tolist() == [1, 0]
    assert t["iterations"].tolist() == [24, 16] and t["converged"].tolist() == [True, False]
    one = {k: v[-1:] for k, v in raw.items()}          # F = 1: the all-rows fits alone
    t = fit.make_table(one, [0.1, 0.2], 1)
    assert t["validation.incorrect"].tolist() == [0, 0] and t["train.incorrect"].tolist() == [5, 6]


def test_back_transform(native):
    from peaksegdisk_amd import fit, predict_penalties
    n = 7
    frame = pd.DataFrame({name: 5.0 * uniforms(20 + k, n) + 2.0 * k for k, name in enumerate(names(3))})
    p = fit.prepare(frame, np.array([[0.0, 1.0]] * n))
    w = np.array([0.7, 0.0, -0.3, 1.25])
    model = fit.back_transform(w, p.names, p.mean, p.sd)
    assert sorted(model["weights"]) == sorted([names(3)[0], names(3)[2]])
    assert model["weights"][names(3)[0]] == 0.7 / p.sd[0]
    # the model predicts in raw units what the standardised weights predict
    want = ref.predict(p.x, w[:-1], w[-1])
    got = np.log(predict_penalties(frame, model))
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert fit.back_transform([0.0, 0.0, 0.0, 2.0], p.names, p.mean, p.sd) == {"intercept": 2.0, "weights": {}}


def test_gram_lambda_max_against_power_iteration(native):
    from peaksegdisk_amd import fit
    n, p = 40, 6
    x = np.stack([uniforms(30 + k, n) for k in range(p)], axis=1)
    x[:, 5] = x[:, 0] + 1e-3 * x[:, 1]          # nearly collinear
    x = (x - x.mean(axis=0)) / x.std(axis=0, ddof=1)
    a = np.hstack([x, np.ones((n, 1))])
    gram = a.T @ a
    v = np.ones(p + 1)
    for _ in range(20000):
        v = gram @ v
        v /= np.linalg.norm(v)
    brute = float(v @ gram @ v)
    got = fit.gram_lambda_max(x)
    assert got >= brute and abs(got / brute - (1.0 + 1e-6)) < 1e-9
    assert got == ref.gram_lambda_max(x)
    assert fit.gram_lambda_max(np.zeros((5, 0))) == pytest.approx(5.0 * (1.0 + 1e-6))


def test_yardstick_gradient_against_central_differences():
    n, p = 11, 3
    x = np.stack([uniforms(40 + k, n) - 0.5 for k in range(p)], axis=1) * 2.0
    centre = 0.5 * x[:, 0] - x[:, 2]
    lo, hi = centre - 0.3, centre + 0.4
    lo[::3], hi[1::3] = -np.inf, np.inf
    train = np.arange(n) % 4 != 1
    w, b = np.array([0.3, -0.2, 0.9]), 0.15
    g, gb = ref.gradient(x, lo, hi, train, w, b)
    h = 1e-6          # the objective is piecewise quadratic: central differences err by O(h) at a kink only
    for j in range(p):
        e = np.zeros(p)
        e[j] = h
        d = (ref.smooth(x, lo, hi, train, w + e, b) - ref.smooth(x, lo, hi, train, w - e, b)) / (2 * h)
        assert abs(d - g[j]) < 1e-7, (j, d, g[j])
    d = (ref.smooth(x, lo, hi, train, w, b + h) - ref.smooth(x, lo, hi, train, w, b - h)) / (2 * h)
    assert abs(d - gb) < 1e-7
    # the rows outside the mask play no part, and infinite limits never give a NaN
    lo2 = lo.copy()
    lo2[~train] = -50.0
    assert np.array_equal(ref.gradient(x, lo2, hi, train, w, b)[0], g)
    assert math.isfinite(ref.objective(x, lo, hi, train, w, b, 0.1))
    # the yardstick's own solver ends on its own certificate
    rw, rb, its, c = ref.fista(x, lo, hi, train, 0.05, ref.gram_lambda_max(x), 1e-9)
    assert c <= 1e-9 and ref.criterion(x, lo, hi, train, rw, rb, 0.05) == c
    assert ref.objective(x, lo, hi, train, rw, rb, 0.05) <= ref.objective(x, lo, hi, train, w, b, 0.05)
