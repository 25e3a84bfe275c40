#!/usr/bin/env python3
"""Timing of the dense in-memory path on the MI355X.

(a) the encoder alone on one contig of 2.5e8 bases (synthetic.poisson_coverage(10**7) expanded on
    the device), (b) the same on many contigs of 10 k bins (about 2.5e5 bases each): HIP events of
    the three launches, warmed, --reps repetitions, minimum / median / maximum, achieved bytes/s by
    the encoder's algorithmic traffic 8 B + 12 R (B bases read twice, R runs x three int32 written)
    and its share of the 6.29 TB/s a plain copy reaches on this chip.
(c) end to end for set (b) with one penalty per contig, alternating in one process:
      dense_api      PeakSegFPOP_dense on device tensors (data frames out)
      dense_arrays   ProblemSet.from_dense + solve + segment_columns + loss on device tensors
      dense_host     the same from host numpy arrays (upload included)
      files          PeakSegFPOP_disk_batch on bedGraph files written beforehand (file to file)
      host_encoded   numpy run-length encoding of the host vectors + ProblemSet + solve + a
                     segments call per problem
    The legs' results are compared for equality before any time is printed.
(s) the segment statistics launch (peakseg_hip_problem_set_pack_segment_stats: zeroing, tile
    kernel, finish kernel between two HIP events) on solved sets: the +Inf model of (a) once and
    64 times in one set, the first 2.5e7 bases of (a) at four penalties, and set (b) with one
    penalty per contig.  Warmed, --reps repetitions, minimum / median / maximum, next to the bytes
    the launch must move (12 R per problem + 24 per row), that figure's share of the copy rate,
    and the forward kernel's time for the same set.

(r) --reads: the path from aligned reads and nothing else.  Synthetic reads
    (synthetic.poisson_reads: lengths 20-115, placed by the piecewise Poisson rate) for the extent
    of (a) and for the contigs of (b), each once sorted by chromStart and once shuffled:
      r_pileup  HIP events of the pile-up (zeroing + scatter; the three scan launches), warmed,
                --reps repetitions, minimum / median / maximum
      r_legs    three ways to a solved set, alternating in one process, results compared for
                equality before any time is printed: from_reads on cuda tensors, from_reads on
                numpy arrays, and numpy add.at + cumsum per contig followed by from_dense.  Each leg
                is timed up to the finished set (creation), then solved; the forward kernel's time
                is the solve's.  For the one-contig set the legs run on its first
                --reads-solve-bases bases (the whole contig's solve takes minutes).

(l) --labels: the label errors and nothing else.  Set (b) with one penalty
    per contig and 32 random labels per contig, and the first 2.5e7 bases of (a) at four penalties
    with 10^4 labels, labels in cuda tensors: HIP events of peakseg_hip_problem_set_pack_label_errors
    (zeroing, translate kernel, count kernel), warmed, --reps repetitions, minimum / median /
    maximum, next to the segment statistics launch and the forward kernel of the same set in the
    same run; the first problems' totals are compared with a brute-force count before any time is
    printed.  Then the target-interval search of Mono27ac with its golden labels at widths 1, 4 and
    8: rounds, models and seconds.

(f) --features: the coverage statistics and nothing else, on the two sets of
    --labels: HIP events of peakseg_hip_problem_set_pack_coverage_stats with the ten ranks of the
    quartiles (zeroing, the moments launch, two launches per digit pass), warmed, --reps
    repetitions, minimum / median / maximum, next to the segment statistics launch and the forward
    kernel of the same set in the same run, the wall time of ProblemSet.coverage_features(), and
    the host path it replaces: the coverage downloaded, then numpy quantile + mean + std per
    contig.  The quartiles of the two paths are compared for equality (mean and sd within 1e-9)
    before any time is printed.

usage: python tools/dense_timing.py [--contigs 6144] [--reps 20] [--e2e-reps 2] [--skip-long]
       [--skip-e2e] [--skip-stats] [--labels] [--features] [--reads [--reads-bins 10000000] [--reads-solve-bases 2500000]]
One JSON line per part on stdout."""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import peaksegdisk_amd as psd  # noqa: E402
from peaksegdisk_amd import ProblemSet, _native, synthetic  # noqa: E402

COPY_BW = 6.29e12  # bytes/s of a plain copy on the MI355X (measured; the specification says 8e12)

ap = argparse.ArgumentParser()
ap.add_argument("--contigs", type=int, default=6144)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--e2e-reps", type=int, default=2)
ap.add_argument("--skip-long", action="store_true")
ap.add_argument("--skip-e2e", action="store_true")
ap.add_argument("--skip-stats", action="store_true")
ap.add_argument("--reads", action="store_true")
ap.add_argument("--labels", action="store_true")
ap.add_argument("--features", action="store_true")
ap.add_argument("--reads-bins", type=int, default=10 ** 7)
ap.add_argument("--reads-solve-bases", type=int, default=2500000)
args = ap.parse_args()
lib = _native.lib


def mmm(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v)}


def expand(cnt, width):
    return torch.repeat_interleave(torch.from_numpy(cnt).to("cuda:0"),
                                   torch.from_numpy(width).to("cuda:0"))


def encoder_laps(tensors, reps):
    nc = len(tensors)
    nb = (ctypes.c_longlong * nc)(*[len(t) for t in tensors])
    ptr = (ctypes.c_void_p * nc)(*[t.data_ptr() for t in tensors])
    runs = np.zeros(nc, np.int64)
    laps = []
    torch.cuda.synchronize()
    for k in range(reps + 3):
        st = lib.peakseg_hip_dense_encode_probe(0, nc, nb, ptr, 1, runs.ctypes.data, None, None,
                                                None, None, None, None)
        assert st == 0, _native.last_error()
        ms = [ctypes.c_float() for _ in range(3)]
        lib.peakseg_hip_dense_last_encode_ms(*[ctypes.byref(m) for m in ms])
        if k >= 3:  # warmed
            laps.append([m.value for m in ms])
    bases = sum(len(t) for t in tensors)
    total = [sum(l) for l in laps]
    traffic = 8.0 * bases + 12.0 * float(runs.sum())
    med = statistics.median(total)
    return {"contigs": nc, "bases": bases, "runs": int(runs.sum()), "reps": reps,
            "traffic_bytes": traffic,
            "count_ms": mmm([l[0] for l in laps]), "scan_ms": mmm([l[1] for l in laps]),
            "scatter_ms": mmm([l[2] for l in laps]), "total_ms": mmm(total),
            "bytes_per_s_median": traffic / (med * 1e-3),
            "share_of_copy_bandwidth": traffic / (med * 1e-3) / COPY_BW,
            "bytes_per_s_best": traffic / (min(total) * 1e-3)}


def stats_laps(part, tensors_, problems_, reps):
    """one JSON line: the statistics launch on the solved set of `problems_`"""
    s = ProblemSet.from_dense(tensors_, problems_)
    try:
        forward_ms = s.solve()[0]
        k = len(problems_)
        rows = np.zeros(k, np.int64)
        ptr = [ctypes.c_void_p() for _ in range(4)]
        laps = []
        for rep in range(reps + 3):
            total = lib.peakseg_hip_problem_set_pack_segment_stats(
                s._h, None, rows.ctypes.data, *[ctypes.byref(q) for q in ptr])
            assert total >= 0, _native.last_error()
            ms = ctypes.c_float()
            lib.peakseg_hip_segment_stats_last_ms(ctypes.byref(ms))
            if rep >= 3:  # warmed
                laps.append(ms.value)
        runs = sum(int(s.loss(p)[4]) for p in range(k))
        # the columns' sums against the contigs': the launch did its work
        got = s.segment_stats()
        sums = {}
        for p, (c, _) in enumerate(problems_):
            sums.setdefault(c, int(tensors_[c].sum(dtype=torch.int64)))
            assert int(got[p][0].sum()) == sums[c], p
        build = s.kernel_build
    finally:
        s.close()
    med = statistics.median(laps)
    must = 12.0 * runs + 24.0 * total
    moved = 8.0 * runs + 64.0 * total
    out = {"part": part, "problems": k, "runs_read": runs, "rows": int(total), "reps": reps,
           "stats_ms": {"min": min(laps), "median": med, "max": max(laps)},
           "bytes_12R_plus_24rows": must, "bytes_per_s_median": must / (med * 1e-3),
           "share_of_copy_bandwidth": must / (med * 1e-3) / COPY_BW,
           "bytes_8R_plus_64rows_the_launches_move": moved,
           "forward_kernel_ms": forward_ms, "kernel_build": build,
           "stats_share_of_forward": med / forward_ms if forward_ms > 0 else None}
    print(json.dumps(out), flush=True)


def pileup_laps(contigs, extents, reps):
    """HIP events of the pile-up alone (no encoding) on device tensors"""
    from peaksegdisk_amd.grid import reads_arguments
    r_args, keep, _ = reads_arguments(contigs, extents, "each", 0, "dense_timing")
    laps = []
    torch.cuda.synchronize()
    for k in range(reps + 3):
        st = lib.peakseg_hip_reads_pileup_probe(0, *r_args, None, None, None, None, None)
        assert st == 0, _native.last_error()
        ms = [ctypes.c_float(), ctypes.c_float()]
        lib.peakseg_hip_reads_last_pileup_ms(ctypes.byref(ms[0]), ctypes.byref(ms[1]))
        if k >= 3:  # warmed
            laps.append([m.value for m in ms])
    n = sum(len(c[0]) for c in contigs)
    bases = sum(hi - lo for lo, hi in extents)
    return {"contigs": len(contigs), "reads": n, "bases": bases, "reps": reps,
            "traffic_bytes_8n_plus_16B": 8.0 * n + 16.0 * bases,
            "scatter_ms": mmm([l[0] for l in laps]), "scan_ms": mmm([l[1] for l in laps]),
            "total_ms": mmm([sum(l) for l in laps])}


def numpy_pileup(start, end, lo, hi):
    """what a user does today: add.at on a difference array, cumsum (reads clipped to [lo, hi))"""
    s = start.astype(np.int64)
    e = end.astype(np.int64)
    inside = (e > lo) & (s < hi)
    diff = np.zeros(hi - lo + 1, np.int32)
    np.add.at(diff, np.maximum(s[inside], lo) - lo, 1)
    np.add.at(diff, np.minimum(e[inside], hi) - lo, -1)
    return np.cumsum(diff[:-1], dtype=np.int32)


def reads_legs(part, host, extents, problems_, reps):
    """one JSON line: the three legs on the reads `host` (numpy), creation timed, then solved"""
    device = [tuple(torch.from_numpy(v).to("cuda:0") for v in c) for c in host]

    def solved(make):
        torch.cuda.synchronize()
        t0 = time.time()
        s = make()
        t_create = time.time() - t0
        try:
            k_ms = s.solve()[0]
            return t_create, k_ms, s.kernel_build, s.segment_columns(), \
                [s.loss(p) for p in range(len(problems_))]
        finally:
            s.close()

    legs = [("from_reads_cuda", lambda: ProblemSet.from_reads(device, problems_, extents=extents)),
            ("from_reads_numpy", lambda: ProblemSet.from_reads(host, problems_, extents=extents)),
            ("numpy_pileup_from_dense", lambda: ProblemSet.from_dense(
                [numpy_pileup(c[0], c[1], lo, hi) for c, (lo, hi) in zip(host, extents)], problems_))]
    times = {name: [] for name, _ in legs}
    last = {}
    for rep in range(reps + 1):  # (the first round warms every leg and is not counted)
        for name, make in legs:
            last[name] = solved(make)
            if rep > 0:
                times[name].append(last[name][0])
    ref = last["numpy_pileup_from_dense"]
    for name in ("from_reads_cuda", "from_reads_numpy"):
        for p in range(len(problems_)):
            assert all(np.array_equal(x, y) for x, y in zip(last[name][3][p], ref[3][p])), (name, p)
            assert np.array_equal(last[name][4][p], ref[4][p]), (name, p)
    laps = pileup_laps(device, extents, args.reps)
    forward_ms = last["from_reads_cuda"][1]
    out = {"part": part, "legs_equal": True, "problems": len(problems_),
           "data_points": int(sum(ref[4][p][4] for p in range(len(problems_)))),
           "forward_kernel_ms": forward_ms, "kernel_build": last["from_reads_cuda"][2],
           "pileup": laps,
           "pileup_share_of_forward": laps["total_ms"]["median"] / forward_ms if forward_ms else None}
    for name, _ in legs:
        out[name + "_create_s"] = mmm(times[name])
    out["numpy_leg_over_from_reads_cuda"] = statistics.median(times["numpy_pileup_from_dense"]) / \
        statistics.median(times["from_reads_cuda"])
    print(json.dumps(out), flush=True)


def reads_mode():
    grid_ = synthetic.penalty_grid()
    # the extent of (a)
    if not args.skip_long:
        s, e, ext = synthetic.poisson_reads(args.reads_bins, seed=1)
        for order, (rs, re_) in (("sorted", (s, e)), ("shuffled", synthetic.shuffled(1, s, e))):
            dev = [(torch.from_numpy(rs).to("cuda:0"), torch.from_numpy(re_).to("cuda:0"))]
            print(json.dumps(dict(part="r_pileup_one_contig_" + order,
                                  **pileup_laps(dev, [ext], args.reps))), flush=True)
            del dev
            if not args.skip_e2e:
                head = (0, min(args.reads_solve_bases, ext[1]))
                keep = rs < head[1]
                reads_legs("r_legs_one_contig_first_bases_" + order, [(rs[keep], re_[keep])], [head],
                           [(0, 1550.5)], args.e2e_reps)
        torch.cuda.empty_cache()
    # the contigs of (b)
    sets = {"sorted": [], "shuffled": []}
    extents = []
    for k in range(args.contigs):
        s, e, ext = synthetic.poisson_reads(10000, seed=k)
        sets["sorted"].append((s, e))
        sets["shuffled"].append(synthetic.shuffled(k, s, e))
        extents.append(ext)
    problems_ = [(k, float(grid_[k % 64])) for k in range(args.contigs)]
    for order in ("sorted", "shuffled"):
        if args.skip_e2e:
            dev = [tuple(torch.from_numpy(v).to("cuda:0") for v in c) for c in sets[order]]
            print(json.dumps(dict(part="r_pileup_many_contigs_" + order,
                                  **pileup_laps(dev, extents, args.reps))), flush=True)
            del dev
        else:
            reads_legs("r_legs_many_contigs_" + order, sets[order], extents, problems_, args.e2e_reps)


def brute_totals(columns, labels):
    """[errors, fp, fn] of one model by looking at every (peak, label) pair"""
    ps, pe = columns[0][1::2].astype(np.int64), columns[1][1::2].astype(np.int64)
    fp = fn = 0
    for ls, le, a in zip(*[x.tolist() for x in labels]):
        over = int(np.sum((ps < le) & (ls < pe)))
        n = over if a in (0, 3) else int(np.sum((ls <= ps) & (ps < le))) if a == 1 else \
            int(np.sum((ls < pe) & (pe <= le)))
        fp += int(a != 3 and n >= (1 if a == 0 else 2))
        fn += int(a != 0 and n == 0)
    return [fp + fn, fp, fn]


def labels_laps(part, tensors_, problems_, labels_host, reps):
    """one JSON line: the label errors, the statistics launch and the forward kernel of one set"""
    labels_dev = [tuple(torch.from_numpy(a).to("cuda:0") for a in e) for e in labels_host]
    s = ProblemSet.from_dense(tensors_, problems_)
    try:
        forward_ms = s.solve()[0]
        k = len(problems_)
        ptr = [ctypes.c_void_p() for _ in range(4)]
        stats = []
        for rep in range(reps + 3):
            assert lib.peakseg_hip_problem_set_pack_segment_stats(
                s._h, None, None, *[ctypes.byref(q) for q in ptr]) >= 0, _native.last_error()
            ms = ctypes.c_float()
            lib.peakseg_hip_segment_stats_last_ms(ctypes.byref(ms))
            if rep >= 3:  # warmed
                stats.append(ms.value)
        laps = []
        for rep in range(reps + 3):
            offs = s.label_errors(labels_dev, torch_device="cuda:0")[0]
            ms = ctypes.c_float()
            lib.peakseg_hip_label_errors_last_ms(ctypes.byref(ms))
            if rep >= 3:
                laps.append(ms.value)
        totals, _ = s.label_errors(labels_dev)
        columns = s.segment_columns()
        for p in range(min(k, 4)):
            assert totals[p][:3].tolist() == brute_totals(columns[p], labels_host[problems_[p][0]]), p
        segments = sum(len(c[0]) for c in columns)
        build = s.kernel_build
    finally:
        s.close()
    med = statistics.median(laps)
    print(json.dumps({
        "part": part, "problems": k, "labels": int(sum(len(e[0]) for e in labels_host)),
        "label_rows": int(offs[-1]), "segments": segments, "reps": reps, "label_errors_ms": mmm(laps),
        "segment_stats_ms": mmm(stats), "forward_kernel_ms": forward_ms, "kernel_build": build,
        "label_errors_share_of_forward": med / forward_ms if forward_ms > 0 else None,
        "label_errors_over_segment_stats": med / statistics.median(stats)}), flush=True)


def labels_mode():
    rng = np.random.default_rng(1)

    def random_labels(n, bases):
        ls = rng.integers(0, bases, n)
        return (ls.astype(np.int32), (ls + rng.integers(1, 5001, n)).astype(np.int32),
                rng.integers(0, 4, n).astype(np.int32))
    grid_ = synthetic.penalty_grid()
    tensors_ = []
    for k in range(args.contigs):
        cs, ce, cnt = synthetic.poisson_coverage(10000, seed=k)
        tensors_.append(expand(cnt, (ce - cs).astype(np.int64)))
    labels_laps("l_b_many_contigs_one_penalty_each_32_labels", tensors_,
                [(k, float(grid_[k % 64])) for k in range(args.contigs)],
                [random_labels(32, len(t)) for t in tensors_], args.reps)
    del tensors_
    torch.cuda.empty_cache()
    if not args.skip_long:
        cs, ce, cnt = synthetic.poisson_coverage(10 ** 6, seed=1)
        long_t = expand(cnt, (ce - cs).astype(np.int64))[:25 * 10 ** 6]
        labels_laps("l_a_first_2.5e7_bases_4_penalties_1e4_labels", [long_t],
                    [(0, 0.72), (0, 37.3), (0, 1550.5), (0, 51795.0)],
                    [random_labels(10 ** 4, len(long_t))], args.reps)
        del long_t
        torch.cuda.empty_cache()
    golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    cols = np.loadtxt(os.path.join(golden, "Mono27ac.bedGraph"), usecols=(1, 2, 3), dtype=np.int64)
    dense = np.repeat(cols[:, 2], cols[:, 1] - cols[:, 0]).astype(np.int32)
    mono_labels, _ = psd.read_labels_bed(os.path.join(golden, "Mono27ac.labels.bed"))
    psd.targetInterval_dense(dense, mono_labels, width=8, chrom_starts=[int(cols[0, 0])])  # warms
    for width in (1, 4, 8):
        t0 = time.time()
        res = psd.targetInterval_dense(dense, mono_labels, width=width, chrom_starts=[int(cols[0, 0])])
        print(json.dumps({"part": "l_target_interval_mono27ac", "width": width, "rounds": res.rounds,
                          "models": len(res.models), "seconds": time.time() - t0,
                          "min_log_lambda": res.min_log_lambda, "max_log_lambda": res.max_log_lambda,
                          "exact": [res.lower_exact, res.upper_exact],
                          "min_errors": res.min_errors}), flush=True)


def features_laps(part, tensors_, problems_, reps):
    """one JSON line: the coverage statistics, the statistics launch and the forward kernel of one
    set, and the host path: download + numpy"""
    from peaksegdisk_amd.grid import quartile_ranks
    s = ProblemSet.from_dense(tensors_, problems_)
    try:
        forward_ms = s.solve()[0]
        ptr = [ctypes.c_void_p() for _ in range(4)]
        stats = []
        for rep in range(reps + 3):
            assert lib.peakseg_hip_problem_set_pack_segment_stats(
                s._h, None, None, *[ctypes.byref(q) for q in ptr]) >= 0, _native.last_error()
            ms = ctypes.c_float()
            lib.peakseg_hip_segment_stats_last_ms(ctypes.byref(ms))
            if rep >= 3:  # warmed
                stats.append(ms.value)
        ranks = np.array([sum(quartile_ranks(len(t))[:2], []) for t in tensors_], dtype=np.int64)
        laps, walls = [], []
        passes = ctypes.c_int()
        for rep in range(reps + 3):
            torch.cuda.synchronize()
            t0 = time.time()
            s._coverage_stats(ranks)
            wall = time.time() - t0
            ms = ctypes.c_float()
            lib.peakseg_hip_coverage_stats_last_ms(ctypes.byref(ms))
            lib.peakseg_hip_coverage_stats_last_passes(ctypes.byref(passes))
            if rep >= 3:
                laps.append(ms.value)
                walls.append(wall)
        t0 = time.time()
        frame = s.coverage_features()
        frame_s = time.time() - t0
        moments = s.coverage_moments()
        runs = int(moments["runs"].sum())
        build = s.kernel_build
    finally:
        s.close()
    # the host path this replaces
    torch.cuda.synchronize()
    t0 = time.time()
    host = [t.cpu().numpy() for t in tensors_]
    t1 = time.time()
    quart = np.array([np.quantile(v, [0, .25, .5, .75, 1]) for v in host])
    mean = np.array([v.mean() for v in host])
    sd = np.array([v.std(ddof=1) for v in host])
    t2 = time.time()
    names = ["quartile.0%", "quartile.25%", "quartile.50%", "quartile.75%", "quartile.100%"]
    assert np.array_equal(frame[names].to_numpy(), quart), part
    assert np.allclose(frame["mean"].to_numpy(), mean, rtol=1e-9, atol=0), part
    assert np.allclose(frame["sd"].to_numpy(), sd, rtol=1e-9, atol=0), part
    assert frame["bases"].tolist() == [float(len(v)) for v in host], part
    med = statistics.median(laps)
    model = 8.0 * runs * (1 + passes.value)
    print(json.dumps({
        "part": part, "contigs": len(tensors_), "problems": len(problems_), "runs": runs,
        "bases": int(sum(len(v) for v in host)), "ranks_per_contig": 10,
        "digit_passes": passes.value, "reps": reps, "results_equal": True,
        "coverage_stats_ms": mmm(laps), "coverage_stats_call_wall_ms": mmm([w * 1e3 for w in walls]),
        "coverage_features_call_s": frame_s,
        "segment_stats_ms": mmm(stats), "forward_kernel_ms": forward_ms, "kernel_build": build,
        "bytes_8R_per_reading_launch": model, "bytes_per_s_median": model / (med * 1e-3),
        "coverage_stats_over_segment_stats": med / statistics.median(stats),
        "coverage_stats_share_of_forward": med / forward_ms if forward_ms > 0 else None,
        "host_download_s": t1 - t0, "host_numpy_s": t2 - t1,
        "host_path_over_coverage_features_call": (t2 - t0) / frame_s}), flush=True)


def features_mode():
    grid_ = synthetic.penalty_grid()
    tensors_ = []
    for k in range(args.contigs):
        cs, ce, cnt = synthetic.poisson_coverage(10000, seed=k)
        tensors_.append(expand(cnt, (ce - cs).astype(np.int64)))
    features_laps("f_b_many_contigs_one_penalty_each", tensors_,
                  [(k, float(grid_[k % 64])) for k in range(args.contigs)], args.reps)
    del tensors_
    torch.cuda.empty_cache()
    if not args.skip_long:
        cs, ce, cnt = synthetic.poisson_coverage(10 ** 6, seed=1)
        long_t = expand(cnt, (ce - cs).astype(np.int64))[:25 * 10 ** 6]
        features_laps("f_a_first_2.5e7_bases_4_penalties", [long_t],
                      [(0, 0.72), (0, 37.3), (0, 1550.5), (0, 51795.0)], args.reps)


if args.reads:
    reads_mode()
    sys.exit(0)
if args.features:
    features_mode()
    sys.exit(0)
if args.labels:
    labels_mode()
    sys.exit(0)


if not args.skip_long:
    cs, ce, cnt = synthetic.poisson_coverage(10 ** 7, seed=1)
    long_t = expand(cnt, (ce - cs).astype(np.int64))
    print(json.dumps(dict(part="a_encoder_one_contig", **encoder_laps([long_t], args.reps))),
          flush=True)
    if not args.skip_stats:
        inf = float("inf")
        stats_laps("s_a_one_contig_inf_model", [long_t], [(0, inf)], args.reps)
        stats_laps("s_a_one_contig_64_inf_models", [long_t], [(0, inf)] * 64, args.reps)
        stats_laps("s_a_first_2.5e7_bases_4_penalties", [long_t[:25 * 10 ** 6]],
                   [(0, 0.72), (0, 37.3), (0, 1550.5), (0, 51795.0)], args.reps)
    del long_t
    torch.cuda.empty_cache()

# set (b)
grid = synthetic.penalty_grid()
bins, tensors = [], []
for k in range(args.contigs):
    cs, ce, cnt = synthetic.poisson_coverage(10000, seed=k)
    width = (ce - cs).astype(np.int64)
    bins.append((cnt, width))
    tensors.append(expand(cnt, width))
print(json.dumps(dict(part="b_encoder_many_contigs", **encoder_laps(tensors, args.reps))),
      flush=True)
pens = [grid[k % 64] for k in range(args.contigs)]
problems = [(k, float(pens[k])) for k in range(args.contigs)]
if not args.skip_stats:
    stats_laps("s_b_many_contigs_one_penalty_each", tensors, problems, args.reps)
if args.skip_e2e:
    sys.exit(0)

host_vectors = [np.repeat(c, w).astype(np.int32) for c, w in bins]


def rle(x):
    change = np.flatnonzero(np.diff(x) != 0)
    ends = np.concatenate([change + 1, [len(x)]]).astype(np.int64)
    starts = np.concatenate([[0], ends[:-1]]).astype(np.int64)
    return x[starts], (ends - starts).astype(np.int32), ends.astype(np.int32)


work = tempfile.mkdtemp(prefix="psd_dense_timing_")
try:
    files = []
    t0 = time.time()
    for k, v in enumerate(host_vectors):
        count, weight, ends = rle(v)
        d = os.path.join(work, "p%05d" % k)
        os.mkdir(d)
        files.append(os.path.join(d, "coverage.bedGraph"))
        synthetic.write_bedgraph(files[-1], ends - weight, ends, count, chrom="chrT")
    t_files = time.time() - t0
    n = args.contigs
    c_files = (ctypes.c_char_p * n)(*[os.fsencode(f) for f in files])
    c_pens = (ctypes.c_char_p * n)(*[p.encode() for p in pens])
    c_dbs = (ctypes.c_char_p * n)(*[os.fsencode(f + ".db") for f in files])
    status = (ctypes.c_int * n)()

    def leg_dense_api():
        return psd.PeakSegFPOP_dense(tensors, [[float(p)] for p in pens], chrom="chrT")

    def leg_dense_arrays(source=tensors):
        s = ProblemSet.from_dense(source, problems)
        try:
            k_ms = s.solve()[0]
            cols = s.segment_columns()
            loss = [s.loss(p) for p in range(n)]
            build = s.kernel_build
        finally:
            s.close()
        return cols, loss, k_ms, build

    def leg_dense_host():
        return leg_dense_arrays(host_vectors)

    def leg_files():
        rc = lib.PeakSegFPOP_disk_batch(n, c_files, c_pens, c_dbs, status)
        assert rc == 0, rc
        return None

    def leg_host_encoded():
        enc = [rle(v) for v in host_vectors]
        s = ProblemSet([(c, w) for c, w, _ in enc], problems)
        try:
            k_ms = s.solve()[0]
            tables = [s.segments(p) for p in range(n)]
        finally:
            s.close()
        return enc, tables, k_ms

    legs = [("dense_api", leg_dense_api), ("dense_arrays", leg_dense_arrays),
            ("dense_host", leg_dense_host), ("files", leg_files),
            ("host_encoded", leg_host_encoded)]
    times = {name: [] for name, _ in legs}
    last = {}
    for rep in range(args.e2e_reps + 1):  # (the first round warms every leg and is not counted)
        for name, fn in legs:
            t0 = time.time()
            last[name] = fn()
            if rep > 0:
                times[name].append(time.time() - t0)
    # equality of the legs' results, before any time is printed
    cols, loss, k_ms_dense, build = last["dense_arrays"]
    cols_h, loss_h, _, _ = last["dense_host"]
    enc, tables, k_ms_host = last["host_encoded"]
    api = last["dense_api"]
    for p in range(n):
        start, end, mean = cols[p]
        assert all(np.array_equal(x, y) for x, y in zip(cols[p], cols_h[p])), p
        assert np.array_equal(loss[p], loss_h[p]), p
        idx, t_mean = tables[p]
        ends = enc[p][2]
        assert np.array_equal(np.where(idx < 0, 0, ends[np.maximum(idx, 0)]), start), p
        assert np.array_equal(t_mean, mean), p
        text = open("%s_penalty=%s_segments.bed" % (files[p], pens[p])).read()
        want = "".join("chrT\t%d\t%d\t%s\t%g\n" % (a, b, "background" if r % 2 == 0 else "peak", m)
                       for r, (a, b, m) in enumerate(zip(start.tolist(), end.tolist(),
                                                         mean.tolist())))
        assert text == want, p
        row = open("%s_penalty=%s_loss.tsv" % (files[p], pens[p])).read().split("\t")
        assert [float(x) for x in row] == loss[p].tolist(), p
        seg = api[p][0].segments
        assert seg["chromStart"].tolist() == start.tolist() and \
            seg["mean"].tolist() == [float("%g" % m) for m in mean.tolist()], p
    out = {"part": "c_end_to_end", "contigs": n, "data_points": int(sum(len(e[0]) for e in enc)),
           "bases": int(sum(len(v) for v in host_vectors)), "kernel_build": build,
           "solve_kernel_s_dense": k_ms_dense / 1e3, "solve_kernel_s_host_encoded": k_ms_host / 1e3,
           "writing_the_bedGraph_files_s_not_in_any_leg": t_files,
           "legs_equal": True, "reps": args.e2e_reps}
    for name, _ in legs:
        out[name + "_s"] = {"min": min(times[name]), "median": statistics.median(times[name]),
                            "max": max(times[name])}
    print(json.dumps(out), flush=True)
    # where the dense path's time goes: the library's own laps, on stderr
    os.environ["PEAKSEG_HIP_TIMING"] = "1"
    t0 = time.time()
    s = ProblemSet.from_dense(tensors, problems)
    t1 = time.time()
    s.solve()
    t2 = time.time()
    s.segment_columns()
    t3 = time.time()
    for p in range(n):
        s.loss(p)
    t4 = time.time()
    s.close()
    print(json.dumps({"part": "c_dense_arrays_phases", "from_dense_s": t1 - t0,
                      "solve_s": t2 - t1, "segment_columns_s": t3 - t2, "loss_rows_s": t4 - t3}),
          flush=True)
finally:
    shutil.rmtree(work, ignore_errors=True)
