"""Timing of ProblemSet.region_stats and ProblemSet.peak_clusters on the MI355X
against the host path each replaces: segment_columns() and the coverage downloaded, then the numpy
yardsticks of the tests (tests/consensus_ref.py), on the same host and in the same call.

(i)  region_stats on set (b) of section 10 -- `--contigs` contigs of 10 k bins, not solved -- in
     three shapes: one region over each whole contig; 32 random regions per contig; one region per
     run (the run-sized windows).  The regions are cuda tensors, read in place.
(ii) peak_clusters on `--samples` samples x `--regions` genomic regions from the same generator with
     a seed per (sample, region) and one penalty: samples x regions problems in `--regions` groups.

Device times are HIP events around the launches (peakseg_hip_*_last_ms), warmed, `--reps`
repetitions: median (min-max); the wall time of the Python call is given next to them.  The host
path is a Python loop per region: it is timed on the first `--host-contigs` contigs (`--host-groups`
groups) only, its results are compared with the device's there, and the ratio is formed per contig
(per group).  There is no pass mark on a ratio.

usage: python tools/consensus_timing.py [--contigs 6144] [--samples 64] [--regions 96] [--reps 20]
       [--host-contigs 8] [--host-groups 2] [--penalty 1550.5] [--skip-regions] [--skip-clusters]
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402
from peaksegdisk_amd import ProblemSet, _native, synthetic  # noqa: E402
from consensus_ref import cluster_ref, region_ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--contigs", type=int, default=6144)
ap.add_argument("--samples", type=int, default=64)
ap.add_argument("--regions", type=int, default=96)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--host-contigs", type=int, default=8)
ap.add_argument("--host-groups", type=int, default=2)
ap.add_argument("--penalty", type=float, default=1550.5)
ap.add_argument("--skip-regions", action="store_true")
ap.add_argument("--skip-clusters", action="store_true")
args = ap.parse_args()
lib = _native.lib
WARM = 3


def mmm(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v)}


def contig(seed):
    """(count, width) of the generator's 10 k bins"""
    cs, ce, cnt = synthetic.poisson_coverage(10000, seed=seed)
    return cnt.astype(np.int32), (ce - cs).astype(np.int64)


def expand(cnt, width):
    return torch.repeat_interleave(torch.from_numpy(cnt).to("cuda:0"), torch.from_numpy(width).to("cuda:0"))


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to("cuda:0")


def region_laps(part, s, bins, kept, regions_host):
    """one JSON line: region_stats with these regions (a list over contigs of (start, end)); kept:
    the dense coverage of the first contigs, on the device"""
    nc = len(bins)
    regions = [(cuda(a), cuda(b)) for a, b in regions_host]
    torch.cuda.synchronize()
    laps, walls = [], []
    for rep in range(args.reps + WARM):
        t0 = time.time()
        offs, bases, total, largest = s.region_stats(regions, torch_device="cuda:0")
        wall = time.time() - t0
        ms = ctypes.c_float()
        lib.peakseg_hip_region_stats_last_ms(ctypes.byref(ms))
        if rep >= WARM:
            laps.append(ms.value)
            walls.append(wall * 1e3)
    got = [t.cpu().numpy() for t in (bases, total, largest)]
    # the host path on the first contigs: the coverage downloaded, then the yardstick
    hc = min(args.host_contigs, nc)
    torch.cuda.synchronize()
    t0 = time.time()
    vectors = [kept[c].cpu().numpy() for c in range(hc)]   # the coverage downloaded
    t1 = time.time()
    want = [region_ref(vectors[c], 0, *regions_host[c]) for c in range(hc)]
    t2 = time.time()
    for c in range(hc):
        rows = slice(int(offs[c]), int(offs[c + 1]))
        assert all(np.array_equal(g[rows], w) for g, w in zip(got, want[c])), (part, c)
    med = statistics.median(laps)
    host_per_contig = (t2 - t0) / hc
    print(json.dumps({
        "part": part, "contigs": nc, "regions": int(offs[-1]), "bins": int(sum(len(b[0]) for b in bins)),
        "runs": int(s.coverage_moments()["runs"].sum()),
        "reps": args.reps, "region_stats_ms": mmm(laps), "region_stats_call_wall_ms": mmm(walls),
        "host_contigs": hc, "host_download_s": t1 - t0, "host_numpy_s": t2 - t1,
        "results_equal_on_host_contigs": True,
        "host_per_contig_over_device_per_contig": host_per_contig / (med * 1e-3 / nc),
        "host_per_contig_over_call_wall_per_contig":
            host_per_contig / (statistics.median(walls) * 1e-3 / nc)}), flush=True)


def regions_mode():
    bins = [contig(k) for k in range(args.contigs)]
    tensors = [expand(*b) for b in bins]
    s = ProblemSet.from_dense(tensors, [(0, float("inf"))])    # (never solved: region_stats needs no solve)
    kept = tensors[:args.host_contigs]
    del tensors
    rng = np.random.default_rng(17)
    try:
        whole = [(np.zeros(1, np.int32), np.array([w.sum()], np.int32)) for _, w in bins]
        region_laps("i_one_whole_contig_region_each", s, bins, kept, whole)
        rand = []
        for _, w in bins:
            b = int(w.sum())
            a = rng.integers(-b // 20, b, 32)
            rand.append((a, a + rng.integers(1, b, 32)))
        region_laps("i_32_random_regions_each", s, bins, kept, rand)
        windows = []
        for _, w in bins:
            end = np.cumsum(w)
            windows.append((end - w, end))
        region_laps("i_one_region_per_run", s, bins, kept, windows)
    finally:
        s.close()


def clusters_mode():
    n = args.samples * args.regions
    bins = [contig(1000003 * (k % args.regions) + k // args.regions) for k in range(n)]
    tensors = [expand(*b) for b in bins]
    groups = np.array([k % args.regions for k in range(n)], np.int32)
    s = ProblemSet.from_dense(tensors, [(k, args.penalty) for k in range(n)])
    kept = {k: tensors[k] for k in range(n) if k % args.regions < args.host_groups}
    del tensors
    try:
        forward_ms = s.solve()[0]
        laps, walls = [], []
        for rep in range(args.reps + WARM):
            t0 = time.time()
            out = s.peak_clusters(groups, torch_device="cuda:0")
            wall = time.time() - t0
            ms = ctypes.c_float()
            lib.peakseg_hip_peak_clusters_last_ms(ctypes.byref(ms))
            if rep >= WARM:
                laps.append(ms.value)
                walls.append(wall * 1e3)
        c_off, e_off = out[0], out[1]
        t0 = time.time()
        result = s.peak_clusters(groups)
        frames_s = time.time() - t0
        peaks = sum(int((s.loss(p)[2])) for p in range(n))
        # the host path on the first groups: every table and the coverage downloaded, then the sweep
        # and the yardstick of the regions
        hg = min(args.host_groups, args.regions)
        torch.cuda.synchronize()
        t0 = time.time()
        columns = s.segment_columns()
        t1 = time.time()
        host_s = 0.0
        for g in range(hg):
            members = np.flatnonzero(groups == g)
            t2 = time.time()
            vectors = [kept[int(p)].cpu().numpy() for p in members]      # the coverage downloaded
            table, m_peaks = cluster_ref([(columns[p][0][1::2][::-1], columns[p][1][1::2][::-1])
                                          for p in members])
            cols = [region_ref(v, 0, table[:, 0], table[:, 1]) for v in vectors]
            host_s += time.time() - t2
            assert np.array_equal(result[g]["clusters"].to_numpy(), table), g
            assert np.array_equal(result[g]["peaks"], m_peaks), g
            for j in range(len(members)):
                for name, w in zip(("bases", "sum", "max"), cols[j]):
                    assert np.array_equal(result[g][name][:, j], w), (g, j, name)
        med = statistics.median(laps)
        host_per_group = (t1 - t0) / args.regions + host_s / hg
        print(json.dumps({
            "part": "ii_peak_clusters", "samples": args.samples, "groups": args.regions, "problems": n,
            "penalty": args.penalty, "peaks": peaks, "clusters": int(c_off[-1]),
            "matrix_entries": int(e_off[-1]), "reps": args.reps, "peak_clusters_ms": mmm(laps),
            "peak_clusters_call_wall_ms": mmm(walls), "peak_clusters_frames_call_s": frames_s,
            "forward_kernel_ms": forward_ms, "kernel_build": s.kernel_build,
            "host_groups": hg, "host_segment_columns_s": t1 - t0, "host_download_sweep_and_regions_s": host_s,
            "results_equal_on_host_groups": True,
            "host_per_group_over_device_per_group": host_per_group / (med * 1e-3 / args.regions),
            "host_per_group_over_call_wall_per_group":
                host_per_group / (statistics.median(walls) * 1e-3 / args.regions)}), flush=True)
    finally:
        s.close()


if not args.skip_regions:
    regions_mode()
    torch.cuda.empty_cache()
if not args.skip_clusters:
    clusters_mode()
