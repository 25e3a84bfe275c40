#!/usr/bin/env python3
"""Timing of the penalty-model fits on one MI355X.

The feature table is that of section 9's set (b): --contigs (6144) contigs of 10 k bins of
synthetic coverage, expanded on the device, their 36 features computed there
(problem_features_dense); the columns that are finite and not constant take part.  The targets are
intervals around a linear function of two of the standardised columns plus noise, a third of them
without lower limit and a third without upper limit.  Two shapes: all rows, and the first 512;
F = 5 folds, the default 64 regularizations: 384 problems per call.

Per shape one JSON line for the device and one for the host: median (min-max) of peakseg_hip_penalty_fit_last_ms over --reps warmed
repetitions, the wall time of a whole fit_penalty_model call, the wall time of the numpy FISTA of
tests/penalty_fit_ref.py over the same problems on this host (once; --skip-host leaves it out),
and the largest iteration count.  Before any time is printed the certificate of the tests is
checked on the timed result: every problem converged and the criterion recomputed in numpy from
its weights is <= threshold + 1e-9 and equals the reported one within 1e-9."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402
import peaksegdisk_amd as psd  # noqa: E402
from peaksegdisk_amd import fit as fit_module, synthetic  # noqa: E402
import penalty_fit_ref as ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--contigs", type=int, default=6144)
ap.add_argument("--small", type=int, default=512)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--folds", type=int, default=5)
ap.add_argument("--skip-host", action="store_true")
args = ap.parse_args()
THRESHOLD = 1e-3


def mmm(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v)}


def normals(seed, stream, n):
    u, v = synthetic.uniform01(seed, stream, n), synthetic.uniform01(seed, stream + 1000, n)
    return np.sqrt(-2.0 * np.log(u)) * np.cos(2.0 * math.pi * v)


def feature_table(contigs):
    tensors = []
    for k in range(contigs):
        cs, ce, cnt = synthetic.poisson_coverage(10000, seed=k)
        tensors.append(torch.repeat_interleave(torch.from_numpy(cnt).to("cuda:0"),
                                               torch.from_numpy((ce - cs).astype(np.int64)).to("cuda:0")))
    frame = psd.problem_features_dense(tensors)
    del tensors
    torch.cuda.empty_cache()
    return frame


def targets_for(frame):
    n = len(frame)
    finite = [c for c in frame.columns if np.all(np.isfinite(frame[c].to_numpy()))
              and frame[c].nunique() > 1]
    pick = [c for c in ("log+1.mean", "log.bases") if c in finite] or finite[:2]
    centre = 2.0 + 0.5 * normals(5, 50, n)
    for sign, name in zip((1.0, -0.5), pick):
        z = frame[name].to_numpy()
        centre = centre + sign * (z - z.mean()) / z.std(ddof=1)
    lo = centre - (0.2 + 1.3 * synthetic.uniform01(5, 51, n))
    hi = centre + (0.2 + 1.3 * synthetic.uniform01(5, 52, n))
    lo[np.arange(n) % 3 == 0] = -np.inf
    hi[np.arange(n) % 3 == 1] = np.inf
    return np.stack([lo, hi], axis=1), pick


def certificate(fit):
    sets, k, _ = fit.weights.shape
    worst = 0.0
    for s in range(sets):
        mask = np.ones(len(fit.fold), bool) if s == sets - 1 else fit.fold != s
        for j in range(k):
            c = ref.criterion(fit.x, fit.lo, fit.hi, mask, fit.weights[s, j, :-1], fit.weights[s, j, -1],
                              fit.regularizations[j])
            assert fit.converged[s, j] == 1, (s, j)
            assert c <= THRESHOLD + 1e-9 and abs(c - fit.criterion[s, j]) <= 1e-9, (s, j, c, fit.criterion[s, j])
            worst = max(worst, c)
    return worst


def shape(part, frame, targets, pick):
    laps, walls = [], []
    for rep in range(args.reps + 3):
        t0 = time.time()
        fit = psd.fit_penalty_model(frame, targets, n_folds=args.folds, threshold=THRESHOLD)
        wall = time.time() - t0
        if rep >= 3:  # warmed
            laps.append(fit.ms)
            walls.append(wall)
    worst = certificate(fit)
    out = {"part": part, "rows": len(fit.rows), "features": len(fit.feature_names),
           "dropped_features": len(fit.dropped_features), "target_columns": pick, "folds": fit.n_folds,
           "regularizations": len(fit.regularizations), "problems": int(fit.converged.size),
           "reps": args.reps, "certificate": True, "largest_criterion": worst,
           "penalty_fit_ms": mmm(laps), "fit_penalty_model_call_ms": mmm([w * 1e3 for w in walls]),
           "largest_iterations": int(fit.iterations.max()), "median_iterations": float(np.median(fit.iterations)),
           "chosen_regularization": fit.regularization,
           "matrix_bytes": 8 * len(fit.rows) * len(fit.feature_names)}
    # two passes over the matrix per gradient, 9 gradients per 8 iterations
    gradients = float((fit.iterations.astype(np.float64) * 9.0 / 8.0 + 1.0).sum())
    out["l2_bytes_per_s_median"] = 2.0 * out["matrix_bytes"] * gradients / (out["penalty_fit_ms"]["median"] * 1e-3)
    print(json.dumps(out), flush=True)
    if not args.skip_host:
        out = {"part": part + "_host_numpy", "penalty_fit_ms": out["penalty_fit_ms"],
               "fit_penalty_model_call_ms": out["fit_penalty_model_call_ms"]}
        lam = ref.gram_lambda_max(fit.x)
        t0 = time.time()
        iterations = 0
        sets, k, _ = fit.weights.shape
        for s in range(sets):
            mask = np.ones(len(fit.fold), bool) if s == sets - 1 else fit.fold != s
            for j in range(k):
                iterations = max(iterations, ref.fista(fit.x, fit.lo, fit.hi, mask, fit.regularizations[j],
                                                       lam, THRESHOLD, 100000)[2])
        out["host_numpy_fista_s"] = time.time() - t0
        out["host_numpy_largest_iterations"] = iterations
        out["host_numpy_over_penalty_fit"] = out["host_numpy_fista_s"] * 1e3 / out["penalty_fit_ms"]["median"]
        out["host_numpy_over_call"] = out["host_numpy_fista_s"] * 1e3 / out["fit_penalty_model_call_ms"]["median"]
        print(json.dumps(out), flush=True)


t0 = time.time()
table = feature_table(args.contigs)
print(json.dumps({"part": "feature_table", "contigs": args.contigs, "seconds": time.time() - t0}), flush=True)
limits, picked = targets_for(table)
shape("fit_all_rows", table, limits, picked)
small_limits, small_picked = targets_for(table.iloc[:args.small])
shape("fit_first_%d_rows" % args.small, table.iloc[:args.small].reset_index(drop=True), small_limits,
      small_picked)
