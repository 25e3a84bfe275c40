"""Timing of the held-out loss, the fold kernels and select_penalty_dense on the MI355X (DESIGN.md
section 18).

Part "heldout_loss": the set (ii) of section 15 -- `--samples` x `--regions` problems of 10 k bins
from the generator, solved at one penalty -- and one pair per problem (its own contig, scale 1).
peakseg_hip_heldout_loss_last_ms, warmed, `--reps` repetitions: median (min-max), with the wall time
of the Python call next to it.  Next to it the only way the parent commit has to the same losses,
timed as wall time on the same host: segment_columns() downloaded, region_stats() with the segments
as regions, numpy for the terms.  The two are compared (relative 1e-9 on the loss, equality on the
sums) before any time is printed.  There is no pass mark on the ratio.

Part "folds": ProblemSet.from_dense_folds and from_reads_folds of `--samples` samples: the fold
kernel's milliseconds (peakseg_hip_fold_units_last_ms) next to the encoder's three launches and the
pile-up's.

Part "select": select_penalty_dense's steps for `--samples` samples x `--folds` folds x
`--penalties` penalties, as wall times: the fold set, the solve, the scoring call, the host tables.

usage: python tools/heldout_timing.py [--samples 64] [--regions 96] [--reps 20] [--penalty 1550.5]
       [--folds 4] [--penalties 16]
One JSON line per part on stdout."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch  # noqa: E402
from peaksegdisk_amd import ProblemSet, _native, synthetic  # noqa: E402
from peaksegdisk_amd.heldout import HeldoutSelection, selection_pairs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=64)
ap.add_argument("--regions", type=int, default=96)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--penalty", type=float, default=1550.5)
ap.add_argument("--folds", type=int, default=4)
ap.add_argument("--penalties", type=int, default=16)
args = ap.parse_args()
lib = _native.lib
WARM = 3


def mmm(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v)}


def last_ms(fn, n=1):
    out = [ctypes.c_float() for _ in range(n)]
    fn(*[ctypes.byref(x) for x in out])
    return [x.value for x in out]


def contig(seed):
    """the dense coverage of the generator's 10 k bins, on the device"""
    cs, ce, cnt = synthetic.poisson_coverage(10000, seed=seed)
    return torch.repeat_interleave(torch.from_numpy(cnt.astype(np.int32)).to("cuda:0"),
                                   torch.from_numpy((ce - cs).astype(np.int64)).to("cuda:0"))


# ---- the held-out loss of one pair per problem, and the host path -------------------------------
n = args.samples * args.regions
tensors = [contig(1000003 * (k % args.regions) + k // args.regions) for k in range(n)]
s = ProblemSet.from_dense(tensors, [(k, args.penalty) for k in range(n)])
samples = tensors[:args.samples]
del tensors
try:
    forward_ms = s.solve()[0]
    pairs = tuple(torch.from_numpy(a).to("cuda:0") for a in (
        np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, dtype=np.float64)))
    laps, walls = [], []
    for rep in range(args.reps + WARM):
        t0 = time.time()
        dev = s.heldout_loss(pairs, torch_device="cuda:0")
        wall = time.time() - t0
        if rep >= WARM:
            laps.append(last_ms(lib.peakseg_hip_heldout_loss_last_ms)[0])
            walls.append(wall * 1e3)
    got = {k: v.cpu().numpy() for k, v in dev.items()}
    host = []
    for rep in range(3):
        t0 = time.time()
        cols = s.segment_columns()
        t1 = time.time()
        stats = s.region_stats([(c[0], c[1]) for c in cols])
        t2 = time.time()
        loss = np.empty(n)
        for p in range(n):
            mean, y = cols[p][2], stats[p]["sum"].astype(np.float64)
            b = stats[p]["bases"].astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                term = np.where(y > 0, mean * b - y * np.log(mean), mean * b)
            loss[p] = term.sum()
        t3 = time.time()
        host.append((t3 - t0, t1 - t0, t2 - t1, t3 - t2))
    assert np.allclose(got["loss"], loss, rtol=1e-9, atol=0.0), "device and host losses differ"
    assert np.array_equal(got["sum"], np.array([int(st["sum"].sum()) for st in stats]))
    best = min(host)
    print(json.dumps({
        "part": "heldout_loss", "problems": n, "pairs": n, "rows": int(got["rows"].sum()),
        "penalty": args.penalty, "reps": args.reps, "heldout_loss_ms": mmm(laps),
        "heldout_loss_call_wall_ms": mmm(walls), "forward_kernel_ms": forward_ms,
        "kernel_build": s.kernel_build,
        "host_path_s": {"total": best[0], "segment_columns": best[1], "region_stats": best[2],
                        "numpy_terms": best[3], "runs": len(host)},
        "losses_equal_rel_1e-9": True,
        "host_path_over_device_ms": best[0] * 1e3 / statistics.median(laps),
        "host_path_over_call_wall": best[0] * 1e3 / statistics.median(walls)}), flush=True)
finally:
    s.close()

# ---- the fold kernels next to the encoder and the pile-up ---------------------------------------
fold_ms, enc_ms = [], []
for rep in range(WARM + 5):
    f = ProblemSet.from_dense_folds(samples, [float("inf")], folds=args.folds, seed=1)
    f.close()
    if rep >= WARM:
        fold_ms.append(last_ms(lib.peakseg_hip_fold_units_last_ms)[0])
        enc_ms.append(last_ms(lib.peakseg_hip_dense_last_encode_ms, 3))
reads = []
for k in range(args.samples):
    start, end, extent = synthetic.poisson_reads(10000, seed=k + 1)
    reads.append((torch.from_numpy(start).to("cuda:0"), torch.from_numpy(end).to("cuda:0"), extent))
rfold_ms, pile_ms = [], []
for rep in range(WARM + 5):
    f = ProblemSet.from_reads_folds([r[:2] for r in reads], [float("inf")], folds=args.folds, seed=1,
                                    extents=[r[2] for r in reads])
    f.close()
    if rep >= WARM:
        rfold_ms.append(last_ms(lib.peakseg_hip_fold_units_last_ms)[0])
        pile_ms.append(last_ms(lib.peakseg_hip_reads_last_pileup_ms, 2))
print(json.dumps({
    "part": "folds", "samples": args.samples, "folds": args.folds,
    "bases": int(sum(t.shape[0] for t in samples)), "reads": int(sum(r[0].shape[0] for r in reads)),
    "dense_fold_kernel_ms": mmm(fold_ms),
    "encoder_count_scan_scatter_ms_of_the_folds": [statistics.median(x[j] for x in enc_ms) for j in range(3)],
    "reads_fold_kernel_ms": mmm(rfold_ms),
    "pileup_scatter_scan_ms_of_the_folds": [statistics.median(x[j] for x in pile_ms) for j in range(2)],
}), flush=True)
del reads

# ---- select_penalty_dense, step by step ---------------------------------------------------------
pens = [float("%.15g" % x) for x in np.logspace(1.0, 5.0, args.penalties)]
steps = []
for rep in range(3):
    torch.cuda.synchronize()
    t0 = time.time()
    f = ProblemSet.from_dense_folds(samples, pens, folds=args.folds, seed=1)
    try:
        t1 = time.time()
        fwd = f.solve()[0]
        t2 = time.time()
        out = f.heldout_loss(selection_pairs(args.samples, args.folds, len(pens)))
        score_ms = last_ms(lib.peakseg_hip_heldout_loss_last_ms)[0]
        t3 = time.time()
        per = args.folds * len(pens)
        seg = np.array([f.result(p).n_segments for p in range(args.samples * per)], dtype=np.int64)
        chosen = [HeldoutSelection(pens, args.folds, (seg[i * per:(i + 1) * per] - 1) // 2,
                                   seg[i * per:(i + 1) * per], out["loss"][i * per:(i + 1) * per],
                                   out["zero_mean_rows"][i * per:(i + 1) * per])
                  for i in range(args.samples)]
        t4 = time.time()
    finally:
        f.close()
    steps.append({"total_s": t4 - t0, "fold_set_s": t1 - t0, "solve_s": t2 - t1,
                  "forward_kernel_ms": fwd, "scoring_call_s": t3 - t2, "scoring_kernels_ms": score_ms,
                  "host_tables_s": t4 - t3})
print(json.dumps({
    "part": "select", "samples": args.samples, "folds": args.folds, "penalties": len(pens),
    "problems": args.samples * args.folds * len(pens), "runs": steps,
    "chosen_train_penalties": sorted({c.train_penalty for c in chosen}),
    "mean_peaks_at_the_choice": float(np.mean([c.summary["peaks"][c.train_index] for c in chosen])),
}), flush=True)
