#!/usr/bin/env python3
"""bench.py -- coverage bins/sec of the PeakSegFPOP hot path on a 64-penalty grid.

A "step" is one pass of the hot path (forward functional-pruning DP + decoding) over one
batch of synthetic input that is already resident in HBM when the timed region starts.

  --mode weak (default)  BASELINE.json configs[1] per GPU: a seeded synthetic Poisson-coverage
                         contig of --bins data points x --penalties log-spaced penalties.  At N
                         GPUs every rank solves its own contig x penalty grid (independent
                         problems, weak scaling); the segment tables are gathered to rank 0
                         over RCCL inside the timed region.
  --mode grid            BASELINE.json configs[3]: 24 contigs, lengths log-uniform in
                         [1e5, 1e7] x --grid-scale, x --penalties penalties, dealt longest-first
                         to the ranks (peaksegdisk_amd.parallel.solve_grid; strong scaling:
                         the work is fixed, upload and gather are inside the timed region).

`python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment starts the N ranks
itself (python -m torch.distributed.run, one process per GPU, rendezvous on 127.0.0.1)
before anything touches the GPU, and exits with their return code; under torchrun it is a
rank.  Every rank checks that the world size equals --gpus.

Prints ONE JSON line (rank 0): metric/value/unit per BASELINE.json, ms_per_step (wall time of
one timed step) and the workload.  A plain run does only what that line needs: set up, warm up,
time --steps steps.  --full adds, after the timed steps,
  checks       -- structural parity gate on every segment table of the last step
  upload       -- value_incl_upload, upload_alloc_s, runtime_init_s (weak mode)
  roofline     -- the kernel (forward pass with the decoding fused in): algorithmic HBM bytes
                  (24 B per (bin,penalty) + 20 B per stored piece; decoding: per
                  segment 12 B written, 8 B + 28 B per piece of the function read) / HIP-event
                  kernel time (events on the stream the kernel runs on), against 8 TB/s
  cpu_baseline -- the CPU oracle (libm build, disk-backed store like the reference) timed on
                  a bounded sample of the same workload on this host: one core, and all cores
                  with a process pool (N=1 only; not with --no-cpu).

--dump-outputs DIR writes the segment tables the last timed step returned as float64 .npy files
(dump_outputs); the inputs are seeded, so two builds can be compared file by file.
"""
import argparse
import json
import os
import shutil
import socket
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s spec


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mode", choices=["weak", "grid"], default="weak")
    ap.add_argument("--bins", type=int, default=1000000)
    ap.add_argument("--penalties", type=int, default=64)
    ap.add_argument("--grid-contigs", type=int, default=24)
    ap.add_argument("--grid-scale", type=float, default=1.0,
                    help="grid mode: contig lengths are log-uniform in [1e5, 1e7] x this")
    ap.add_argument("--cpu-bins", type=int, default=40000,
                    help="CPU baseline, one core: first this many bins x every penalty")
    ap.add_argument("--cpu-bins-all", type=int, default=1000000,
                    help="CPU baseline, all cores: first this many bins x every penalty")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also the parity gate, upload timing, roofline and CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last step's segment tables to DIR/<name>.npy")
    return ap.parse_args(argv)


# --dump-outputs: at most this many table rows (x 3 float64 files = 48 MiB); a longer
# concatenation is written as a seeded sample of its rows
DUMP_MAX_ROWS = 2 ** 21
DUMP_SEED = 20261016


def dump_outputs(out_dir, tables, summary=None, max_rows=DUMP_MAX_ROWS):
    """tables: list of (seg_start, seg_mean) in problem order, as the step returned them.
    Writes float64 arrays: seg_rows (rows per table), seg_row_index (which rows of the
    concatenated tables follow: all of them, or a sorted seeded sample of max_rows when there
    are more), seg_start and seg_mean (those rows), and summary when given."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    rows = np.array([len(s) for s, _ in tables], dtype=np.float64)
    start = np.concatenate([np.asarray(s, dtype=np.float64) for s, _ in tables] or [np.zeros(0)])
    mean = np.concatenate([np.asarray(m, dtype=np.float64) for _, m in tables] or [np.zeros(0)])
    if len(start) > max_rows:
        index = np.sort(np.random.default_rng(DUMP_SEED).choice(len(start), max_rows,
                                                                replace=False))
    else:
        index = np.arange(len(start))
    arrays = {"seg_rows": rows, "seg_row_index": index.astype(np.float64),
              "seg_start": start[index], "seg_mean": mean[index]}
    if summary is not None:
        arrays["summary"] = np.asarray(summary, dtype=np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def cpu_model_name():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def host_cores():
    """Cores this process may actually use: the affinity mask, cut by the cgroup CPU quota
    (a GPU box hands each GPU's container a share of a large host)."""
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                parts = f.read().split()
            if path.endswith("cpu.max"):
                if parts[0] != "max":
                    cores = min(cores, max(1, int(round(int(parts[0]) / int(parts[1])))))
            else:
                quota = int(parts[0])
                with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                    period = int(f.read())
                if quota > 0:
                    cores = min(cores, max(1, int(round(quota / period))))
            break
        except (OSError, ValueError, IndexError):
            continue
    return cores


def cpu_baseline(chrom_start, chrom_end, count, penalties, bins_one, bins_all):
    """Time oracle_cli_libm -- one process per (contig, penalty), cost-function database on
    local scratch, as the reference runs -- on the bench workload:
      (i)  one process at a time on one core: the first `bins_one` bins of the contig at EVERY
           penalty of the grid (a bounded sample: the CPU needs ~10 min for the whole grid);
      (ii) a pool with one worker per usable host core: the first `bins_all` bins (default:
           the whole contig) at every penalty.  Besides the all-cores rate this gives the CPU
           seconds (user + system, from wait4) of every process, i.e. what one core needs for
           the grid at the bench's own contig length -- per-bin cost grows with the length, so
           the short sample of (i) flatters the CPU.
    kind = "port": the reference's own solver sources include R.h, which this image lacks, so
    they cannot be built here; the oracle is the C restatement pinned by
    the reference's fixtures."""
    from concurrent.futures import ThreadPoolExecutor
    from peaksegdisk_amd import synthetic
    cli = os.path.join(ROOT, "oracle", "_build", "oracle_cli_libm")
    if not os.path.exists(cli):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    cores = host_cores()
    work = tempfile.mkdtemp(prefix="psd_cpu_")

    def run_one(bg, pen, k):
        """returns the child's user + system CPU seconds"""
        proc = subprocess.Popen([cli, bg, pen, os.path.join(work, "db%d" % k)],
                                stdout=subprocess.DEVNULL)
        _, status, ru = os.wait4(proc.pid, 0)
        proc.returncode = os.waitstatus_to_exitcode(status)
        if proc.returncode != 0:
            raise RuntimeError("oracle_cli_libm status %d" % proc.returncode)
        return ru.ru_utime + ru.ru_stime

    try:
        n1 = min(bins_one, len(count))
        bg1 = os.path.join(work, "one", "coverage.bedGraph")
        os.makedirs(os.path.dirname(bg1))
        synthetic.write_bedgraph(bg1, chrom_start[:n1], chrom_end[:n1], count[:n1])
        t0 = time.time()
        for k, pen in enumerate(penalties):
            run_one(bg1, pen, k)
        wall1 = time.time() - t0
        n2 = min(bins_all, len(count))
        bg2 = os.path.join(work, "all", "coverage.bedGraph")
        os.makedirs(os.path.dirname(bg2))
        synthetic.write_bedgraph(bg2, chrom_start[:n2], chrom_end[:n2], count[:n2])
        t0 = time.time()
        with ThreadPoolExecutor(max_workers=cores) as pool:  # each task is one child process
            cpu_s = list(pool.map(lambda kp: run_one(bg2, kp[1], 1000 + kp[0]),
                                  enumerate(penalties)))
        wall2 = time.time() - t0
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return {
        "value": n1 * len(penalties) / wall1, "unit": "bins/s", "cores": 1, "kind": "port",
        "sample": "first %d bins of the contig x all %d penalties, oracle_cli_libm (C "
                  "restatement, glibc exp/log, disk-backed store), one process per problem, "
                  "one at a time, %.1f s wall" % (n1, len(penalties), wall1),
        "all_cores": {
            "value": n2 * len(penalties) / wall2, "unit": "bins/s", "cores": cores,
            "sample": "first %d bins x all %d penalties, pool of %d processes, %.1f s wall"
                      % (n2, len(penalties), cores, wall2),
        },
        "one_core_at_length": {
            "value": n2 * len(penalties) / sum(cpu_s), "unit": "bins/s", "cores": 1,
            "sample": "the same %d processes: %d bins x %d penalties / their summed user+system "
                      "CPU time (%.1f s)" % (len(penalties), n2, len(penalties), sum(cpu_s)),
        },
        "cpu_model": cpu_model_name(),
        "why_port": "the reference's solver sources include R.h (absent here): unbuildable, "
                    "see DESIGN.md section 2",
    }


def grid_contig_lengths(n_contigs, scale):
    """configs[3]: contig lengths log-uniform in [1e5, 1e7] (x scale), seeded."""
    from peaksegdisk_amd import synthetic
    u = synthetic.uniform01(20241001, 9, n_contigs)
    return [max(64, int(round(scale * 10.0 ** (5.0 + 2.0 * x)))) for x in u]


def headline(args, world, units_per_step, elapsed, lengths):
    """The fields of the result line that a plain run prints (lengths: grid mode's contigs)."""
    if args.mode == "weak":
        workload = ("%d-bin synthetic Poisson coverage x %d-penalty grid per GPU "
                    "(BASELINE.json configs[1])" % (args.bins, args.penalties))
        cfg = {"workload": workload, "bins": args.bins, "penalties": args.penalties,
               "penalty_grid": "10^seq(-1,5), 15 significant digits", "seed": "1+rank",
               "sharding": "independent (contig x penalty) problems per rank; RCCL gather "
                           "of segment tables to rank 0"}
    else:
        workload = ("%d synthetic contigs of %d..%d bins (log-uniform) x %d penalties "
                    "dealt longest-first to %d rank(s) (BASELINE.json configs[3])"
                    % (len(lengths), min(lengths), max(lengths), args.penalties, world))
        cfg = {"workload": workload, "contigs": len(lengths), "total_bins": sum(lengths),
               "penalties": args.penalties, "grid_scale": args.grid_scale,
               "sharding": "LPT dealing of (contig x penalty) problems; one RCCL gather of "
                           "segment tables + summaries to rank 0; upload inside the timed "
                           "region"}
    return {
        "metric": "coverage bins/sec across 64-penalty grid",
        "value": units_per_step * args.steps / elapsed,
        "unit": "bins/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak" if args.mode == "weak" else "strong",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": cfg,
    }


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(args):
    """--gpus N without a torchrun environment: build once, then start N ranks as children
    (never by replacing this process) and return their exit code."""
    import __graft_entry__ as entry
    if not os.environ.get("PSD_BENCH_TEST_LIB"):
        entry.build_hip()
    entry.build_oracle()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def main():
    args = parse_args()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args))

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    # RCCL ("nccl") on GPUs; tests rehearse the N>1 plumbing on CPU with PSD_BENCH_BACKEND=gloo
    # and the kernels under the SIMT emulator (PSD_BENCH_TEST_LIB, honoured only with gloo)
    backend = os.environ.get("PSD_BENCH_BACKEND", "nccl")
    on_gpu = backend == "nccl"
    import numpy as np
    import __graft_entry__ as entry
    if world == 1 and not os.environ.get("PSD_BENCH_TEST_LIB"):
        entry.build_hip()  # N > 1: the launcher (or the driver's build step) has built it
    import torch
    dist = None
    if world > 1:
        import torch.distributed as dist
        if on_gpu:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
        assert dist.get_world_size() == args.gpus
        if not os.environ.get("PSD_BENCH_TEST_LIB"):
            # under the driver's torchrun the library is normally built already (build());
            # if it is not, one rank builds it and the others wait
            if rank == 0 and not os.path.exists(entry.LIB):
                entry.build_hip()
            dist.barrier()
    device = local_rank if (world > 1 and on_gpu) else 0
    from peaksegdisk_amd import _native
    if not on_gpu and os.environ.get("PSD_BENCH_TEST_LIB"):
        import ctypes
        _native.lib = _native.declare(ctypes.CDLL(os.environ["PSD_BENCH_TEST_LIB"]))
    from peaksegdisk_amd import ProblemSet, synthetic
    from peaksegdisk_amd.parallel import gather_problem_set, solve_grid

    pen_str = synthetic.penalty_grid(args.penalties)
    penalties = [float(p) for p in pen_str]

    def sync():
        if on_gpu:
            torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()

    def finish():
        if args.mode == "weak":
            pset.close()
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()

    extra = {}
    lengths = None
    if args.mode == "weak":
        # every rank: its own contig (seed 1 + rank), the same penalty grid
        cs, ce, cnt = synthetic.poisson_coverage(args.bins, seed=1 + rank)
        weight = (ce - cs).astype(np.int32)
        problems = [(0, p) for p in penalties]
        # The first HIP call of a process creates the device context (0.2-0.4 s, once per
        # process, whatever is solved afterwards): a one-bin set pays it here, so that create_s
        # is what SURVEY.md 8(d) counts -- upload and allocation of THIS set
        # (profiles/r04/create_timing.log: 0.45 s for the first set of a process, 0.02 s for
        # the second and third).  --full only: a plain run reports no upload figures.
        if args.full:
            t_c = time.time()
            ProblemSet([(cnt[:2], weight[:2])], [(0, 1.0)], device=device).close()
            runtime_init_s = time.time() - t_c
        t_c = time.time()
        pset = ProblemSet([(cnt, weight)], problems, device=device)
        create_s = time.time() - t_c

        def one_step():
            f_ms, _ = pset.solve()
            # every segment table leaves the device inside the timed region: packed in HBM,
            # then one download (N = 1) or the RCCL gather to rank 0 (N > 1)
            gathered = gather_problem_set(pset, dist, device)
            return f_ms, gathered

        units_per_step = args.bins * args.penalties * world
    else:
        lengths = grid_contig_lengths(args.grid_contigs, args.grid_scale)
        contigs = []
        for c, n in enumerate(lengths):
            s_, e_, k_ = synthetic.poisson_coverage(n, seed=101 + c)
            contigs.append((k_, (e_ - s_).astype(np.int32)))
        stats = {}

        def one_step():
            # the dealing of the next step uses what the ranks measured in this one (cycles per
            # data point by penalty rank, the same numbers on every rank)
            out = solve_grid(contigs, penalties, dist, device, stats=stats,
                             cycles_per_step=stats.get("cycles_per_step"))
            return stats.get("forward_ms", 0.0), out

        units_per_step = sum(lengths) * args.penalties
        create_s = None

    for _ in range(args.warmup):
        one_step()
    sync()
    t0 = time.time()
    fwd = []
    for _ in range(args.steps):
        f_ms, gathered = one_step()
        fwd.append(f_ms)
    sync()
    elapsed = time.time() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if on_gpu else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if rank == 0 and args.dump_outputs:
        if args.mode == "weak":
            # every rank's tables, rank by rank, each in penalty order
            dump_outputs(args.dump_outputs, [t for tables, _ in gathered for t in tables])
        else:
            keys = sorted(gathered)  # (contig, penalty index)
            dump_outputs(args.dump_outputs,
                         [(gathered[k]["seg_start"], gathered[k]["seg_mean"]) for k in keys],
                         np.array([gathered[k]["summary"] for k in keys], dtype=np.float64))
    if not args.full:
        if rank == 0:
            print(json.dumps(headline(args, world, units_per_step, elapsed, lengths)))
        finish()
        return

    # parity gate on what was just computed: structural checks that hold for every solution
    if args.mode == "weak":
        results = [pset.result(p) for p in range(len(problems))]
        for p, r in enumerate(results):
            assert r.status == 0, "problem %d failed with kernel status %d" % (p, r.kernel_status)
            start, mean = pset.segments(p)
            assert len(start) == r.n_segments and len(start) % 2 == 1
            assert start[-1] == -1 and (np.diff(start[:-1]) < 0).all()
        total_pieces = sum(r.total_intervals for r in results)
        bins_launch = args.bins * args.penalties
        alg_bytes = 24.0 * bins_launch + 20.0 * total_pieces
        for r in results:  # decoding: one function looked up per segment
            alg_bytes += r.n_segments * (20.0 + 28.0 * r.total_intervals / (2.0 * args.bins))
        extra = {"hbm_bytes_resident": pset.hbm_bytes, "arena_bytes_used": pset.arena_bytes_used,
                 "kernel_build": pset.kernel_build,
                 "serial_env_replays": int(sum(r.n_serial_env for r in results))}
        if rank == 0:
            # what the last step's gather left on rank 0: every rank's tables, exact sizes
            assert len(gathered) == world
            extra["tables_on_rank0"] = int(sum(len(t) for t, _ in gathered))
            assert extra["tables_on_rank0"] == world * len(problems)
            for p, (gs, gm) in enumerate(gathered[0][0]):
                start, mean = pset.segments(p)
                assert np.array_equal(gs, start) and np.array_equal(gm.view(np.uint64),
                                                                   mean.view(np.uint64))
    elif rank == 0:
        assert len(gathered) == len(lengths) * len(penalties)
        total_pieces = 0.0
        alg_bytes = 0.0
        for (c, p), res in gathered.items():
            n_seg, _, _, tot, _ = res["summary"]
            assert len(res["seg_start"]) == int(n_seg) and res["seg_start"][-1] == -1
            total_pieces += tot
            alg_bytes += n_seg * (20.0 + 28.0 * tot / (2.0 * lengths[c]))
        bins_launch = sum(lengths) * args.penalties
        alg_bytes += 24.0 * bins_launch + 20.0 * total_pieces
        # the ranks' kernels run concurrently: rank 0's launch moves about its share
        alg_bytes /= world
        bins_launch /= world
        extra = {"kernel_build": stats.get("kernel_build"),
                 "tables_on_rank0": len(gathered),
                 "dealing": "measured cycles per data point" if stats.get("cycles_per_step")
                            else "default ramp (nothing measured yet)",
                 "hbm_bytes_resident": stats.get("hbm_bytes"),
                 # 0: every cost function stored; K: the checkpointed store (picked when the
                 # full store of rank 0's share would not fit its HBM)
                 "checkpoint_interval": stats.get("checkpoint_interval"),
                 # kernel launches of rank 0's solve: 1 unless problems ran out of room and
                 # were resumed (full store) or solved again (checkpointed store)
                 "launches": stats.get("launches"),
                 "rank0_phase_seconds": {k: round(stats[k], 3) for k in
                                         ("create_s", "solve_s", "tables_s", "close_s")
                                         if k in stats}}

    if rank == 0:
        # HBM traffic of one forward launch from the PMC counters (collected separately with
        # rocprofv3 --pmc by tools/collect_profiles.sh); only valid for that workload
        traffic = None
        if args.mode == "weak":
            for rnd in ("r04", "r03", "r02", "r01"):
                try:
                    with open(os.path.join(ROOT, "profiles", rnd, "pmc_traffic.json")) as f:
                        pmc = json.load(f)
                    if pmc["workload"]["bins"] == args.bins and \
                            pmc["workload"]["penalties"] == args.penalties:
                        traffic = pmc["traffic_bytes_per_launch"]
                        extra["traffic_source"] = "profiles/%s/pmc_traffic.json" % rnd
                        break
                except (OSError, KeyError, ValueError):
                    pass
        fwd_s = float(np.mean(fwd)) / 1e3
        clock_hz = None
        if on_gpu:
            khz = _native.lib.peakseg_hip_device_clock_khz(device)
            clock_hz = khz * 1e3 if khz > 0 else None
        # latency build: 4 waves per problem (two chains + helpers), throughput build: 2
        n_prob_rank0 = len(problems) if args.mode == "weak" else stats.get("problems", 0)
        wave_slots_used = n_prob_rank0 * (4 if extra.get("kernel_build") == "lat" else 2)
        wave_slots_used = min(wave_slots_used, 8192)
        out = headline(args, world, units_per_step, elapsed, lengths)
        out["roofline"] = {
            "bound": "hbm", "kernel": "fpop_forward_kernel",
            "achieved": alg_bytes / fwd_s / 1e9 if fwd_s > 0 else None,
            "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": alg_bytes / fwd_s / 1e9 / HBM_PEAK_GBS if fwd_s > 0 else None,
            "traffic": traffic,
            "algorithmic_bytes_per_launch": alg_bytes,
            "kernel_ms": float(np.mean(fwd)),  # forward pass + decoding, one launch
            "dp_steps_per_s_per_problem":
                (args.bins / fwd_s if args.mode == "weak" and fwd_s > 0 else None),
            # what actually bounds the kernel: the length of one
            # wave's dependent instruction chain per data point, on the slowest problem of
            # the launch (the kernel ends when it does), and how little of the chip a
            # 64-problem grid can occupy
            "cycles_per_step_slowest_problem":
                (fwd_s * clock_hz / args.bins if args.mode == "weak" and clock_hz else None),
            "shader_clock_mhz": clock_hz / 1e6 if clock_hz else None,
            "wave_slots_used": wave_slots_used,
            "wave_slots": 8192,
            "mean_intervals": total_pieces / (2.0 * bins_launch * (world if args.mode == "grid" else 1)),
        }
        # What bounds a data point from below (tools/chain_floor.py, profiles/r04/chain_floor.json:
        # the dependent chain of the slower chain wave priced with this repository's own probe
        # latencies, and the cycles one wave needs just to issue its instructions): the kernel is
        # latency-bound, and THIS is the fraction a reader can grade -- the HBM fraction above is
        # four orders of magnitude from anything by construction.
        try:
            with open(os.path.join(ROOT, "profiles", "r04", "chain_floor.json")) as f:
                floor = json.load(f)
            cps = out["roofline"]["cycles_per_step_slowest_problem"]
            out["roofline"]["chain_floor_cycles_per_step"] = floor["chain_floor_cycles_per_step"]
            out["roofline"]["issue_floor_cycles_per_step"] = floor["issue_floor_cycles_per_step"]
            out["roofline"]["frac_of_chain_floor"] = \
                floor["chain_floor_cycles_per_step"] / cps if cps else None
            out["roofline"]["chain_floor_source"] = "profiles/r04/chain_floor.json"
        except (OSError, KeyError, ValueError):
            pass
        out.update(extra)
        if create_s is not None:
            # SURVEY.md 8(d) counts the upload in the wall time; the bench contract wants
            # `value` with the inputs already resident in HBM (the PCIe-inclusive rate is never
            # `value`).  Both are on the line: `value` = resident, `value_incl_upload` = the
            # same step with upload + allocation of the set counted.
            out["value_incl_upload"] = units_per_step / world / \
                (create_s + elapsed / args.steps)
            out["upload_alloc_s"] = create_s
            out["runtime_init_s"] = runtime_init_s  # device context, once per process: not in any rate
        if not args.no_cpu and world == 1 and args.mode == "weak":
            out["cpu_baseline"] = cpu_baseline(cs, ce, cnt, pen_str, args.cpu_bins,
                                               args.cpu_bins_all)
            out["gpu_over_cpu"] = out["value"] / out["cpu_baseline"]["value"]
            out["gpu_over_cpu_incl_upload"] = \
                out["value_incl_upload"] / out["cpu_baseline"]["value"]
            out["gpu_over_cpu_all_cores"] = out["value"] / out["cpu_baseline"]["all_cores"]["value"]
            out["gpu_over_cpu_core_at_length"] = \
                out["value"] / out["cpu_baseline"]["one_core_at_length"]["value"]
        print(json.dumps(out))
    finish()


if __name__ == "__main__":
    main()
