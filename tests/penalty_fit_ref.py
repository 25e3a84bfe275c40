"""The yardstick of the penalty-model fits (numpy only, float64): objective, gradient and stopping
criterion of the interval regression of DESIGN.md section 14, the validation figures, and a plain
FISTA that the tests use only where they say so.  Nothing here comes from the library.

Rows: x (n, p) standardised features, lo / hi the limits in log(penalty) (-inf / +inf allowed),
train a boolean mask of the rows that take part.  With phi(z) = (z - 1)^2 for z < 1, else 0,
    F(w, b) = (1/|S|) sum over S of  phi(f_i - lo_i) + phi(hi_i - f_i)  +  reg |w|_1,   f = b + x w."""
import numpy as np


def phi(z):
    z = np.asarray(z, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(z < 1.0, (np.where(np.isfinite(z), z, 0.0) - 1.0) ** 2, 0.0)


def dphi(z):
    z = np.asarray(z, np.float64)
    return np.where(z < 1.0, 2.0 * (np.where(np.isfinite(z), z, 0.0) - 1.0), 0.0)


def predict(x, w, b):
    return b + np.asarray(x, np.float64) @ np.asarray(w, np.float64)


def smooth(x, lo, hi, train, w, b):
    """the smooth part of the objective: the mean squared hinge of the training rows"""
    f = predict(x, w, b)[train]
    return float(np.sum(phi(f - lo[train]) + phi(hi[train] - f)) / np.count_nonzero(train))


def objective(x, lo, hi, train, w, b, reg):
    return smooth(x, lo, hi, train, w, b) + reg * float(np.sum(np.abs(w)))


def gradient(x, lo, hi, train, w, b):
    """(gradient by w, derivative by b) of the smooth part"""
    f = predict(x, w, b)[train]
    r = (dphi(f - lo[train]) - dphi(hi[train] - f)) / np.count_nonzero(train)
    return x[train].T @ r, float(np.sum(r))


def criterion(x, lo, hi, train, w, b, reg):
    """the distance of the subgradient of F at (w, b) from zero in the sup norm"""
    g, gb = gradient(x, lo, hi, train, w, b)
    w = np.asarray(w, np.float64)
    c = np.where(w != 0.0, np.abs(g + reg * np.sign(w)), np.maximum(0.0, np.abs(g) - reg))
    return max(abs(gb), float(c.max()) if len(c) else 0.0)


def incorrect(x, lo, hi, rows, w, b):
    """the rows of the mask `rows` whose prediction lies outside their interval"""
    f = predict(x, w, b)[rows]
    return int(np.count_nonzero((f < lo[rows]) | (f > hi[rows])))


def hinge(x, lo, hi, rows, w, b):
    f = predict(x, w, b)[rows]
    return float(np.sum(phi(f - lo[rows]) + phi(hi[rows] - f)))


def limit_distance(x, lo, hi, w, b):
    """how close a prediction comes to a finite limit of its row"""
    f = predict(x, w, b)
    d = np.concatenate([np.abs(f - lo)[np.isfinite(lo)], np.abs(f - hi)[np.isfinite(hi)]])
    return float(d.min()) if len(d) else np.inf


def gram_lambda_max(x):
    """the largest eigenvalue of [x 1]'[x 1] with the margin the library's caller adds"""
    a = np.hstack([np.asarray(x, np.float64), np.ones((len(x), 1))])
    return float(np.linalg.eigvalsh(a.T @ a)[-1]) * (1.0 + 1e-6)


def soft(a, k):
    return np.sign(a) * np.maximum(np.abs(a) - k, 0.0)


def fista(x, lo, hi, train, reg, lambda_max, threshold, max_iterations=1000000):
    """(w, b, iterations, criterion): accelerated proximal gradient from zero, constant step
    |S| / (4 lambda_max), gradient restart, the criterion looked at every iteration"""
    n, p = x.shape
    rows = np.count_nonzero(train)
    step = rows / (4.0 * lambda_max)
    w, b = np.zeros(p), 0.0
    yw, yb, t = w.copy(), 0.0, 1.0
    for it in range(max_iterations + 1):
        c = criterion(x, lo, hi, train, w, b, reg)
        if c <= threshold or it == max_iterations:
            return w, b, it, c
        g, gb = gradient(x, lo, hi, train, yw, yb)
        nw, nb = soft(yw - step * g, step * reg), yb - step * gb
        if float(np.dot(yw - nw, nw - w)) + (yb - nb) * (nb - b) > 0.0:
            t, keep = 1.0, 0.0
        else:
            nt = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
            keep, t = (t - 1.0) / nt, nt
        yw, yb = nw + keep * (nw - w), nb + keep * (nb - b)
        w, b = nw, nb
