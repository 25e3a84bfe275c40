"""Timing of ProblemSet.joint_path on the MI355X against the loop it
replaces: one ProblemSet.joint_peaks per penalty, in the same session on the same resident set.

The set is (ii) of sections 15 and 16: `--samples` samples x `--regions` genomic regions of 10 k
bins from the generator with a seed per (sample, region), solved at one penalty.  The windows are
the clusters, downloaded once and given to both sides as device arrays, so neither side runs the
cluster step.  The penalties are log-spaced over the range of the positive gains at penalty 0.

For 1, 8 and 16 penalties: peakseg_hip_joint_path_last_ms of one call against the sum of
peakseg_hip_joint_peaks_last_ms over the same penalties, one call each -- HIP events from the first
launch to the last, warmed, `--reps` repetitions: median (min-max).  Before any time is printed the
path's columns are compared with the loop's for equality, byte for byte.  Then
ProblemSet.joint_label_errors with `--labels` labels per problem on the 16-penalty path, and the
search of joint_target.joint_target_interval on the resident set -- what learn_joint_penalty_dense
runs after its single-sample solve -- with its number of rounds.  There is no pass mark.

usage: python tools/joint_path_timing.py [--samples 64] [--regions 96] [--reps 20] [--labels 32]
       [--penalty 1550.5]
One JSON line on stdout."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402
from peaksegdisk_amd import ProblemSet, _native, joint_target_interval, synthetic  # noqa: E402
from joint_ref import cluster_window  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=64)
ap.add_argument("--regions", type=int, default=96)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--labels", type=int, default=32)
ap.add_argument("--penalty", type=float, default=1550.5)
args = ap.parse_args()
lib = _native.lib
WARM = 3


def mmm(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v)}


def contig(seed):
    """the dense coverage of the generator's 10 k bins, on the device"""
    cs, ce, cnt = synthetic.poisson_coverage(10000, seed=seed)
    return torch.repeat_interleave(torch.from_numpy(cnt.astype(np.int32)).to("cuda:0"),
                                   torch.from_numpy((ce - cs).astype(np.int64)).to("cuda:0"))


def last_ms(name):
    ms = ctypes.c_float()
    getattr(lib, name)(ctypes.byref(ms))
    return ms.value


def columns(model):
    return [(e["joint"].to_numpy().tobytes(), e["gain"].tobytes(), e["up"].tobytes(),
             e["sum"].tobytes(), e["bases"].tobytes()) for e in model]


n = args.samples * args.regions
tensors = [contig(1000003 * (k % args.regions) + k // args.regions) for k in range(n)]
lengths = [int(t.numel()) for t in tensors]
groups = np.array([k % args.regions for k in range(n)], np.int32)
s = ProblemSet.from_dense(tensors, [(k, args.penalty) for k in range(n)])
del tensors
try:
    s.solve()
    clusters = s.peak_clusters(groups)
    windows = []
    for entry in clusters:
        table = entry["clusters"][["clusterStart", "clusterEnd"]].to_numpy().tolist()
        pairs = [cluster_window(cs, ce) for cs, ce in table]
        windows.append((torch.tensor([a for a, _ in pairs], dtype=torch.int32, device="cuda:0"),
                        torch.tensor([b for _, b in pairs], dtype=torch.int32, device="cuda:0"))
                       if pairs else None)
    at_zero = s.joint_peaks(groups, penalty=0.0, windows=windows)
    gains = np.concatenate([e["gain"].ravel() for e in at_zero])
    gains = gains[gains > 0]
    out = {"part": "joint_path", "samples": args.samples, "groups": args.regions, "problems": n,
           "penalty": args.penalty, "windows": int(sum(len(e["joint"]) for e in at_zero)),
           "matrix_entries": int(sum(e["gain"].size for e in at_zero)), "reps": args.reps,
           "gain_range": [float(gains.min()), float(gains.max())]}
    for count in (1, 8, 16):
        pens = np.exp(np.linspace(np.log(gains.min()), np.log(gains.max()), count + 2)[1:-1]).tolist()
        path = s.joint_path(groups, pens, windows=windows)
        for p, penalty in enumerate(pens):           # equality before any time
            assert columns(path[p]) == columns(s.joint_peaks(groups, penalty=penalty, windows=windows)), penalty
        path_ms, loop_ms, path_wall, loop_wall = [], [], [], []
        for rep in range(args.reps + WARM):
            t0 = time.time()
            s.joint_path(groups, pens, windows=windows, torch_device="cuda:0")
            wall = time.time() - t0
            one = last_ms("peakseg_hip_joint_path_last_ms")
            t0 = time.time()
            total = 0.0
            for penalty in pens:
                s.joint_peaks(groups, penalty=penalty, windows=windows, torch_device="cuda:0")
                total += last_ms("peakseg_hip_joint_peaks_last_ms")
            if rep >= WARM:
                path_ms.append(one)
                loop_ms.append(total)
                path_wall.append(wall * 1e3)
                loop_wall.append((time.time() - t0) * 1e3)
        out["penalties_%d" % count] = {
            "penalties": pens, "columns_equal": True, "path_ms": mmm(path_ms), "loop_ms": mmm(loop_ms),
            "path_call_wall_ms": mmm(path_wall), "loop_calls_wall_ms": mmm(loop_wall),
            "loop_over_path": statistics.median(loop_ms) / statistics.median(path_ms),
            "windows_with_a_joint_peak": [int(sum((e["joint"]["peakStart"] >= 0).sum() for e in m))
                                          for m in path]}
    # the label errors of the 16 models: `--labels` labels per problem, on the device
    rng = np.random.default_rng(3)
    labels = []
    for k in range(n):
        start = np.sort(rng.integers(0, lengths[k] - 2000, args.labels)).astype(np.int32)
        end = (start + rng.integers(1, 2000, args.labels)).astype(np.int32)
        labels.append(tuple(torch.from_numpy(a).to("cuda:0") for a in
                            (start, end, rng.integers(0, 4, args.labels).astype(np.int32))))
    laps = []
    for rep in range(args.reps + WARM):
        model = s.joint_label_errors(labels, torch_device="cuda:0")[5]
        if rep >= WARM:
            laps.append(last_ms("peakseg_hip_joint_label_errors_last_ms"))
    out["joint_label_errors"] = {"labels_per_problem": args.labels, "penalties": 16, "ms": mmm(laps),
                                 "errors_per_model": model.cpu().numpy()[:, 0].tolist()}
    host_labels = [tuple(a.cpu().numpy() for a in e) for e in labels]
    t0 = time.time()
    found = joint_target_interval(s, groups, host_labels, windows=windows)
    out["joint_target_interval"] = {
        "seconds": time.time() - t0, "rounds": found.rounds, "models": len(found.models),
        "min_errors": found.min_errors, "min_log_lambda": found.min_log_lambda,
        "max_log_lambda": found.max_log_lambda, "penalty": found.penalty}
    print(json.dumps(out), flush=True)
finally:
    s.close()
