"""Timing of duplicate removal on the MI355X, next to the pile-up of the same
reads and to the host route.

The two sets of section 11: (a) the reads of synthetic.poisson_reads(`--reads-bins` bins) as one
contig -- 1.6e7 reads at the default -- and (b) `--contigs` contigs of 10 k bins, each sorted and
shuffled, with duplicates added by hash: a quarter as many copies of reads chosen by
uniform01(seed, 31, .), strands included, so that a fifth of the rows are duplicates.  Strands by
hash (+1 iff splitmix64(1, index) is even); reads and strands as cuda tensors.  Per set and order:
peakseg_hip_reads_last_dedup_ms (keys, sort, runs) of the marking by 5' end at keep 1, warmed,
`--reps` repetitions: median (min-max), with the wall time of the call, the number of passes the keys'
mask chose and the summary; peakseg_hip_reads_last_pileup_ms of the pile-up of the same reads measured
the same way in the same process; and the host route -- download, a removal by np.lexsort, upload of
the survivors -- by the wall clock, `--host-reps` repetitions.  Two calls are compared for equal
bytes, and the marks with the host route's, before any time is printed.  There is no pass mark on
either ratio.

usage: python tools/dedup_timing.py [--contigs 6144] [--reps 20] [--host-reps 3]
       [--reads-bins 10000000] [--skip-long]
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
from peaksegdisk_amd import _native, dedup, synthetic  # noqa: E402
from peaksegdisk_amd.grid import reads_arguments  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--contigs", type=int, default=6144)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--reads-bins", type=int, default=10 ** 7)
ap.add_argument("--skip-long", action="store_true")
args = ap.parse_args()
lib = _native.lib
WARM = 3


def mmm(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v)}


def last_ms(fn, n):
    out = [ctypes.c_float() for _ in range(n)]
    fn(*[ctypes.byref(x) for x in out])
    return [x.value for x in out]


def with_duplicates(seed, s, e):
    """(chromStart, chromEnd, strand): the reads, strands by hash, and a quarter as many copies"""
    n = len(s)
    even = (synthetic.splitmix64(1, np.arange(n, dtype=np.uint64)) & np.uint64(1)) == 0
    d = np.where(even, 1, -1).astype(np.int8)
    source = np.minimum(np.floor(synthetic.uniform01(seed, 31, n // 4) * n).astype(np.int64), n - 1)
    return np.concatenate([s, s[source]]), np.concatenate([e, e[source]]), np.concatenate([d, d[source]])


def host_route(reads, strands):
    """download, keep the first read of every (5' base, strand) by a stable lexsort, upload"""
    out = []
    for (s, e), d in zip(reads, strands):
        hs, he, hd = s.cpu().numpy(), e.cpu().numpy(), d.cpu().numpy()
        five = np.where(hd > 0, hs, he - 1)
        order = np.lexsort((five, hd))
        head = np.ones(len(order), bool)
        head[1:] = (five[order][1:] != five[order][:-1]) | (hd[order][1:] != hd[order][:-1])
        keep = np.zeros(len(order), bool)
        keep[order[head]] = True
        out.append((tuple(torch.from_numpy(v[keep]).to("cuda:0") for v in (hs, he, hd)), keep))
    torch.cuda.synchronize()
    return out


def laps(part, host, extents):
    reads = [tuple(torch.from_numpy(v).to("cuda:0") for v in c[:2]) for c in host]
    strands = [torch.from_numpy(c[2]).to("cuda:0") for c in host]
    torch.cuda.synchronize()
    keys, sort, runs, walls, seen = [], [], [], [], []
    for rep in range(args.reps + WARM):
        t0 = time.time()
        out, summary = dedup.mark(reads, strands, 1, "five_prime", 0, lib, "dedup_timing")
        wall = time.time() - t0
        if rep >= WARM:
            ms = last_ms(lib.peakseg_hip_reads_last_dedup_ms, 3)
            keys.append(ms[0])
            sort.append(ms[1])
            runs.append(ms[2])
            walls.append(wall * 1e3)
        if rep < 2:
            seen.append(b"".join(o.cpu().numpy().tobytes() for o in out) + summary.tobytes())
    assert seen[0] == seen[1], "two calls gave different bytes"
    n_passes = lib.peakseg_hip_reads_last_dedup_passes()
    host_ms = []
    for rep in range(args.host_reps):
        t0 = time.time()
        routed = host_route(reads, strands)
        host_ms.append((time.time() - t0) * 1e3)
    for o, (_, keep) in zip(out, routed):
        assert np.array_equal(o.cpu().numpy() > 0, keep), "the marks differ from the host route's"
    del routed
    r_args, alive, _ = reads_arguments(reads, extents, "each", 0, "dedup_timing")
    scatter, scan = [], []
    for rep in range(args.reps + WARM):
        st = lib.peakseg_hip_reads_pileup_probe(0, *r_args, None, None, None, None, None)
        assert st == 0, _native.last_error()
        if rep >= WARM:
            ms = last_ms(lib.peakseg_hip_reads_last_pileup_ms, 2)
            scatter.append(ms[0])
            scan.append(ms[1])
    total = [a + b + c for a, b, c in zip(keys, sort, runs)]
    pile = [a + b for a, b in zip(scatter, scan)]
    print(json.dumps({
        "part": part, "contigs": len(host), "rows": int(summary[:, 0].sum()), "by": "five_prime",
        "keep": 1, "kept": int(summary[:, 1].sum()), "distinct": int(summary[:, 3].sum()),
        "passes": n_passes, "reps": args.reps, "keys_ms": mmm(keys), "sort_ms": mmm(sort),
        "runs_ms": mmm(runs), "total_ms": mmm(total), "call_wall_ms": mmm(walls),
        "pileup_total_ms": mmm(pile), "dedup_over_pileup": statistics.median(total) / statistics.median(pile),
        "host_route_wall_ms": mmm(host_ms), "host_reps": args.host_reps,
        "host_route_over_call_wall": statistics.median(host_ms) / statistics.median(walls),
        "bytes_equal_between_calls": True, "marks_equal_host_route": True}), flush=True)


if not args.skip_long:
    s, e, ext = synthetic.poisson_reads(args.reads_bins, seed=1)
    part = with_duplicates(1, s, e)
    for order, rows in (("sorted", tuple(a[np.argsort(part[0], kind="stable")] for a in part)),
                        ("shuffled", synthetic.shuffled(1, *part))):
        laps("d_one_contig_" + order, [rows], [ext])
        torch.cuda.empty_cache()
    del s, e, part, rows
sets = {"sorted": [], "shuffled": []}
extents = []
for k in range(args.contigs):
    s, e, ext = synthetic.poisson_reads(10000, seed=k)
    part = with_duplicates(k, s, e)
    sets["sorted"].append(tuple(a[np.argsort(part[0], kind="stable")] for a in part))
    sets["shuffled"].append(synthetic.shuffled(k, *part))
    extents.append(ext)
for order in ("sorted", "shuffled"):
    laps("d_many_contigs_" + order, sets[order], extents)
