"""Timing of ProblemSet.joint_peaks on the MI355X against the host path it
replaces: the coverage of every member downloaded, then the numpy yardstick of the tests
(tests/joint_ref.py, with float64 in place of longdouble and without its margin assertions), on the
same host and in the same call.

The set is (ii) of section 15: `--samples` samples x `--regions` genomic regions of 10 k bins from
the generator with a seed per (sample, region), solved at one penalty: samples x regions problems in
`--regions` groups.  The windows are the clusters (windows=None), so a call runs the cluster step
first; peakseg_hip_joint_peaks_last_ms covers the joint step alone.

Device times are HIP events from the first launch to the last, warmed, `--reps` repetitions: median
(min-max); the wall time of the Python call (cluster step included) is given next to them.  The host
path is a Python loop per window: it is timed on the first `--host-groups` groups only, its peaks
are compared for equality with the device's there before any time is printed, and the ratio is
formed per group.  There is no pass mark on the ratio: it compares a kernel with a Python loop.

usage: python tools/joint_timing.py [--samples 64] [--regions 96] [--reps 20] [--host-groups 2]
       [--penalty 1550.5] [--joint-penalty 0]
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
from peaksegdisk_amd import ProblemSet, _native, synthetic  # noqa: E402
from joint_ref import cluster_window, joint_peaks_ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=64)
ap.add_argument("--regions", type=int, default=96)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--host-groups", type=int, default=2)
ap.add_argument("--penalty", type=float, default=1550.5)
ap.add_argument("--joint-penalty", type=float, default=0.0)
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


n = args.samples * args.regions
tensors = [contig(1000003 * (k % args.regions) + k // args.regions) for k in range(n)]
groups = np.array([k % args.regions for k in range(n)], np.int32)
s = ProblemSet.from_dense(tensors, [(k, args.penalty) for k in range(n)])
kept = {k: tensors[k] for k in range(n) if k % args.regions < args.host_groups}
del tensors
try:
    forward_ms = s.solve()[0]
    laps, walls = [], []
    for rep in range(args.reps + WARM):
        t0 = time.time()
        out = s.joint_peaks(groups, penalty=args.joint_penalty, torch_device="cuda:0")
        wall = time.time() - t0
        ms = ctypes.c_float()
        lib.peakseg_hip_joint_peaks_last_ms(ctypes.byref(ms))
        if rep >= WARM:
            laps.append(ms.value)
            walls.append(wall * 1e3)
    w_off, e_off = out[0], out[1]
    levels = out[8].cpu().numpy()
    t0 = time.time()
    result = s.joint_peaks(groups, penalty=args.joint_penalty)
    frames_s = time.time() - t0
    clusters = s.peak_clusters(groups)
    # the host path on the first groups: the coverage downloaded, then the yardstick per window
    hg = min(args.host_groups, args.regions)
    torch.cuda.synchronize()
    host_s, host_windows = 0.0, 0
    for g in range(hg):
        members = np.flatnonzero(groups == g)
        table = clusters[g]["clusters"][["clusterStart", "clusterEnd"]].to_numpy().tolist()
        t1 = time.time()
        vectors = [kept[int(p)].cpu().numpy() for p in members]          # the coverage downloaded
        refs = [joint_peaks_ref(vectors, [0] * len(vectors), cluster_window(cs, ce), args.joint_penalty,
                                real=np.float64, check_margin=False) for cs, ce in table]
        host_s += time.time() - t1
        host_windows += len(table)
        frame = result[g]["joint"]
        for k, ref in enumerate(refs):
            got = (int(frame["peakStart"][k]), int(frame["peakEnd"][k]), int(frame["samples_up"][k]))
            assert got == (ref["peakStart"], ref["peakEnd"], ref["samples_up"]), (g, k, got, ref["trace"])
            assert np.array_equal(result[g]["sum"][k], ref["sum"]), (g, k)
    med = statistics.median(laps)
    print(json.dumps({
        "part": "joint_peaks", "samples": args.samples, "groups": args.regions, "problems": n,
        "penalty": args.penalty, "joint_penalty": args.joint_penalty, "windows": int(w_off[-1]),
        "matrix_entries": int(e_off[-1]), "levels_max": int(levels.max()) if len(levels) else 0,
        "windows_with_a_joint_peak": int((out[4].cpu().numpy() >= 0).sum()),
        "reps": args.reps, "joint_peaks_ms": mmm(laps), "joint_peaks_call_wall_ms": mmm(walls),
        "joint_peaks_frames_call_s": frames_s, "forward_kernel_ms": forward_ms,
        "kernel_build": s.kernel_build, "host_groups": hg, "host_windows": host_windows,
        "host_download_and_yardstick_s": host_s, "peaks_equal_on_host_groups": True,
        "host_per_group_over_device_per_group": (host_s / hg) / (med * 1e-3 / args.regions),
        "host_per_group_over_call_wall_per_group":
            (host_s / hg) / (statistics.median(walls) * 1e-3 / args.regions)}), flush=True)
finally:
    s.close()
