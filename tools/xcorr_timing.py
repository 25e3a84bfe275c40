"""Timing of the strand cross-correlation on the MI355X, next to the pile-up
of the same reads.

The two sets of section 11: (a) the reads of synthetic.poisson_reads(`--reads-bins` bins) as one
contig -- 1.6e7 reads on 2.5e8 bases at the default -- and (b) `--contigs` contigs of 10 k bins.
Strands by hash (+1 iff splitmix64(1, index) is even), reads and strands as cuda tensors, sorted and
shuffled.  Per set: peakseg_hip_reads_last_xcorr_ms (zeroing and tags_kernel; xcorr_kernel and
edges_kernel) at `--max-shift`, warmed, `--reps` repetitions: median (min-max), with the wall time
of the call, and peakseg_hip_reads_last_pileup_ms of the pile-up alone measured the same way (what
tools/dense_timing.py --reads --skip-e2e measures).  Two calls are compared for equal bytes before
any time is printed.  xcorr_kernel and edges_kernel are also timed at the widths of `--also` (5
repetitions): max_shift 0 leaves the reading and the staging, 1023 has all four shifts of a thread
and 1024 table atomics per tile.  There is no pass mark on the ratio.

usage: python tools/xcorr_timing.py [--contigs 6144] [--reps 20] [--max-shift 400]
       [--reads-bins 10000000] [--skip-long] [--also 0,1023]
One JSON line per set and order on stdout."""
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
from peaksegdisk_amd import _native, strand, synthetic  # noqa: E402
from peaksegdisk_amd.grid import reads_arguments  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--contigs", type=int, default=6144)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--max-shift", type=int, default=400)
ap.add_argument("--reads-bins", type=int, default=10 ** 7)
ap.add_argument("--skip-long", action="store_true")
ap.add_argument("--also", type=lambda v: [int(x) for x in v.split(",") if x], default=[0, 1023])
args = ap.parse_args()
lib = _native.lib
WARM = 3


def mmm(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v)}


def last_ms(fn):
    out = [ctypes.c_float(), ctypes.c_float()]
    fn(ctypes.byref(out[0]), ctypes.byref(out[1]))
    return [x.value for x in out]


def hash_strands(n):
    even = (synthetic.splitmix64(1, np.arange(n, dtype=np.uint64)) & np.uint64(1)) == 0
    return np.where(even, 1, -1).astype(np.int8)


def laps(part, host, extents):
    """one JSON line: the cross-correlation and the pile-up of the reads `host` (numpy, per contig
    (chromStart, chromEnd, strand)) on device tensors"""
    reads = [tuple(torch.from_numpy(v).to("cuda:0") for v in c[:2]) for c in host]
    strands = [torch.from_numpy(c[2]).to("cuda:0") for c in host]
    torch.cuda.synchronize()
    tags, cross, walls, tables = [], [], [], []
    for rep in range(args.reps + WARM):
        t0 = time.time()
        table, _ = strand.xcorr_tables(reads, strands, args.max_shift, extents, 0, lib, "xcorr_timing")
        wall = time.time() - t0
        if rep >= WARM:
            ms = last_ms(lib.peakseg_hip_reads_last_xcorr_ms)
            tags.append(ms[0])
            cross.append(ms[1])
            walls.append(wall * 1e3)
        if rep < 2:
            tables.append(np.stack(table).tobytes())
    assert tables[0] == tables[1], "two calls gave different tables"
    other = {}
    for shifts in args.also:   # where the time goes: the same reads at other widths, 5 repetitions
        ms = []
        for rep in range(5 + WARM):
            strand.xcorr_tables(reads, strands, shifts, extents, 0, lib, "xcorr_timing")
            if rep >= WARM:
                ms.append(last_ms(lib.peakseg_hip_reads_last_xcorr_ms)[1])
        other[str(shifts)] = statistics.median(ms)
    rows = strand.pooled(table)
    shift = strand.choose_shift(rows)
    r_args, keep, _ = reads_arguments(reads, extents, "each", 0, "xcorr_timing")
    scatter, scan = [], []
    for rep in range(args.reps + WARM):
        st = lib.peakseg_hip_reads_pileup_probe(0, *r_args, None, None, None, None, None)
        assert st == 0, _native.last_error()
        if rep >= WARM:
            ms = last_ms(lib.peakseg_hip_reads_last_pileup_ms)
            scatter.append(ms[0])
            scan.append(ms[1])
    n = sum(len(c[0]) for c in host)
    bases = sum(hi - lo for lo, hi in extents)
    total = [a + b for a, b in zip(tags, cross)]
    pile = [a + b for a, b in zip(scatter, scan)]
    print(json.dumps({
        "part": part, "contigs": len(host), "reads": n, "bases": bases, "max_shift": args.max_shift,
        "reps": args.reps, "plus_tags": int(rows[0][1]), "minus_tags": int(rows[0][3]),
        "tags_ms": mmm(tags), "xcorr_ms": mmm(cross), "total_ms": mmm(total),
        "xcorr_ms_median_at_other_max_shift": other,
        "call_wall_ms": mmm(walls), "pileup_scatter_ms": mmm(scatter), "pileup_scan_ms": mmm(scan),
        "pileup_total_ms": mmm(pile),
        "xcorr_over_pileup": statistics.median(total) / statistics.median(pile),
        "pooled_shift_of_largest_r": shift, "pooled_largest_r": strand.correlation(rows[shift]),
        "tables_equal_between_calls": True}), flush=True)


if not args.skip_long:
    s, e, ext = synthetic.poisson_reads(args.reads_bins, seed=1)
    d = hash_strands(len(s))
    for order, part in (("sorted", (s, e, d)), ("shuffled", synthetic.shuffled(1, s, e, d))):
        laps("x_one_contig_" + order, [part], [ext])
        torch.cuda.empty_cache()
    del s, e, d
sets = {"sorted": [], "shuffled": []}
extents = []
for k in range(args.contigs):
    s, e, ext = synthetic.poisson_reads(10000, seed=k)
    d = hash_strands(len(s))
    sets["sorted"].append((s, e, d))
    sets["shuffled"].append(synthetic.shuffled(k, s, e, d))
    extents.append(ext)
for order in ("sorted", "shuffled"):
    laps("x_many_contigs_" + order, sets[order], extents)
