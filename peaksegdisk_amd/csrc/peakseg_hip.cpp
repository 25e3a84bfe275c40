/* peakseg_hip.cpp -- host driver and C ABI of libpeaksegdisk_hip.so.
 *
 * Host-side counterpart of the reference's solver driver
 * (/root/reference/src/PeakSegFPOPLog.cpp:143-463, "drv"): bedGraph parsing and validation,
 * the trivial one-segment branch, upload, kernel launches, and the two output files.  The
 * dynamic program itself only exists as HIP kernels (fpop_kernels.h): when no GPU is
 * visible the DP branch fails with ERROR_NO_HIP_DEVICE -- there is no CPU fallback.
 *
 * One translation unit: this file instantiates the three kernel builds and holds the thin
 * accessors of the C ABI; the rest of the host side is in the peakseg_*.h it includes, one file
 * per concern (text, set, devices, create, solve, pack, dense, reads, labels, features, fit, regions, clusters, joint, joint_path, joint_labels, heldout, strand, fanout, files, dir, search), each
 * headed by what it holds.
 *
 * Compiled with: hipcc -x hip --offload-arch=gfx950 -ffp-contract=off
 * (tests/emu builds the same file with g++ -DPSD_EMU against the SIMT emulator).
 */
#include "../../include/peaksegdisk_hip.h"

/* Two builds of the same kernel source:
 *   lat  latency build: 128 pieces per LDS list, a helper wave per chain, and the piece-list
 *        operations inlined into the kernel's loop (4 waves per workgroup, all registers of
 *        the SIMDs: 1 workgroup per CU).  Fastest per problem; used while every problem of
 *        the set gets a CU of its own (the 64-penalty grid of one contig runs here).
 *   thr  throughput build: 64 pieces per LDS list, no helper waves, operations out of line
 *        (2 waves per workgroup, 4 workgroups per CU).  ~12% slower per problem, four times
 *        the problems per CU; used for sets that oversubscribe the chip (many contigs x many
 *        penalties).  (Registers for 3 waves per SIMD with 56-piece lists -- 5 workgroups per
 *        CU, -DPSD_THR_LDS_CAP=56 -DPSD_THR_WAVES_PER_EU=3 -- gain 7.5 % on 6144 equal problems
 *        and lose 7 % on the 24-contig x 64-penalty shape, whose end is set by its longest
 *        problems: profiles/r02/ab_thr_occupancy.log.)
 * Both produce identical results. */
#define PSD_VARIANT lat
#define PSD_LDS_CAP 128
#define PSD_MATH_VK 1
#define PSD_HELPER_WAVES 1
#define PSD_FLAG_BARRIER 1
#include "fpop_kernels.h"
#undef PSD_VARIANT
#undef PSD_LDS_CAP
#undef PSD_HELPER_WAVES
#undef PSD_FLAG_BARRIER
#undef PSD_MATH_VK
#define PSD_VARIANT thr
#ifndef PSD_THR_LDS_CAP /* A/B builds: -DPSD_THR_LDS_CAP=56 -DPSD_THR_WAVES_PER_EU=3 */
#define PSD_THR_LDS_CAP 64
#endif
#ifndef PSD_THR_WAVES_PER_EU
#define PSD_THR_WAVES_PER_EU 2
#endif
#define PSD_LDS_CAP PSD_THR_LDS_CAP
#define PSD_KERNEL_WAVES_PER_EU PSD_THR_WAVES_PER_EU
#define PSD_CALL_LDS_OPS 1
#include "fpop_kernels.h"
#undef PSD_VARIANT
#undef PSD_LDS_CAP
#undef PSD_KERNEL_WAVES_PER_EU
#undef PSD_CALL_LDS_OPS

/*   pk   packed build (round 4): 40 pieces per LDS list, registers for three waves per SIMD
 *        (six workgroups per CU), operations out of line.  A problem on a SIMD shared three ways
 *        advances more slowly than on the throughput build, but a CU holds half as many again:
 *        +18 % on sets of many problems of similar length, -10 % where a set ends with its
 *        longest packed problems (profiles/r04/ab_thr_occupancy_*.log) -- the planner
 *        (plan_solve in peakseg_solve.h) picks it when it predicts the earlier end.  A function that
 *        outgrows 40 pieces does not go to the (ten times slower) HBM path here: the problem is
 *        parked and resumed on the throughput build, whose lists hold 64. */
#define PSD_VARIANT pk
#define PSD_LDS_CAP 40
#define PSD_KERNEL_WAVES_PER_EU 3
#define PSD_CALL_LDS_OPS 1
#define PSD_PARK_ON_LDS_OVERFLOW 1
#include "fpop_kernels.h"
#undef PSD_VARIANT
#undef PSD_LDS_CAP
#undef PSD_KERNEL_WAVES_PER_EU
#undef PSD_CALL_LDS_OPS
#undef PSD_PARK_ON_LDS_OVERFLOW

/* run-length encoding of dense coverage and the reference's segments table, on the device */
#include "dense_encode.h"
/* reads, maximum and summit of every segment from the resident runs */
#include "segment_stats.h"
/* coverage from aligned reads: the pile-up the dense encoder reads in place */
#include "reads_pileup.h"
/* label errors of every model from the resident tables */
#include "label_errors.h"
/* order statistics and moments of every contig's coverage from the resident runs */
#include "coverage_stats.h"
/* the fits of a penalty-learning regression over a regularisation path and the folds */
#include "penalty_fit.h"
/* the coverage of any regions from the resident runs: bases, sum and maximum */
#include "region_stats.h"
/* the clusters of overlapping peaks over the members of a group, and the cluster-by-member matrix */
#include "peak_clusters.h"
/* one common peak per window for all members of a group: the level-by-level search */
#include "joint_peaks.h"
/* the joint peaks at many penalties in one call, and the label errors of every such model */
#include "joint_path.h"
#include "joint_labels.h"
/* the Poisson loss of every model on another contig of the set: what thinning scores a penalty by */
#include "heldout_loss.h"
/* the sampling units of dense counts or reads split at random into folds */
#include "fold_units.h"
/* the strand cross-correlation of single-end reads, and their extension to a fragment length */
#include "strand_xcorr.h"
/* duplicate removal of reads: a stable radix sort of their keys, the first k units of every key */
#include "reads_dedup.h"
/* tests only: every form of the deterministic exp / log, element by element */
#include "math_forms_probe.h"

#include <ctype.h>
#include <errno.h>
#include <limits.h>
#include <algorithm>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#include "peakseg_text.h"
#include "peakseg_set.h"
#include "peakseg_devices.h"
#include "peakseg_create.h"
#include "peakseg_solve.h"
#include "peakseg_pack.h"
#include "peakseg_dense.h"
#include "peakseg_reads.h"
#include "peakseg_labels.h"
#include "peakseg_features.h"
#include "peakseg_fit.h"
#include "peakseg_regions.h"
#include "peakseg_clusters.h"
#include "peakseg_joint.h"
#include "peakseg_joint_path.h"
#include "peakseg_joint_labels.h"
#include "peakseg_heldout.h"
#include "peakseg_strand.h"
#include "peakseg_dedup.h"

extern "C" int peakseg_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

extern "C" const char *peakseg_hip_last_error(void) { return g_last_error.c_str(); }
extern "C" const char *peakseg_hip_last_warning(void) { return g_last_warning.c_str(); }

/* shader clock of a device in kHz (0 when unknown): bench.py turns kernel time into cycles per
 * data point with it */
extern "C" int peakseg_hip_device_clock_khz(int device) {
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, device) != hipSuccess) return 0;
  return khz;
}

extern "C" void peakseg_hip_set_print(void (*print)(const char *)) { g_print = print; }

extern "C" int peakseg_hip_last_fanout(int capacity, int *shard_device, int *shard_programs,
                                       double *shard_seconds) {
  const int n = (int)g_fanout.device.size();
  for (int s = 0; s < n && s < capacity; s++) {
    if (shard_device) shard_device[s] = g_fanout.device[(size_t)s];
    if (shard_programs) shard_programs[s] = g_fanout.programs[(size_t)s];
    if (shard_seconds) shard_seconds[s] = g_fanout.seconds[(size_t)s];
  }
  return n;
}

extern "C" int peakseg_hip_last_fanout_entries(int n, int *shard_of) {
  const int m = (int)g_fanout.entry_shard.size();
  for (int i = 0; i < n && i < m; i++)
    if (shard_of) shard_of[i] = g_fanout.entry_shard[(size_t)i];
  return m;
}

extern "C" void peakseg_hip_problem_set_destroy(psd_problem_set *s) {
  if (!s) return;
  free_arena(s);
  for (void *q : s->allocs) (void)hipFree(q);
  for (auto &e : s->ev)
    if (e) (void)hipEventDestroy(e);
  if (s->ev2) (void)hipEventDestroy(s->ev2);
  for (auto &e : s->stats.ev)
    if (e) (void)hipEventDestroy(e);
  for (auto &e : s->labels.ev)
    if (e) (void)hipEventDestroy(e);
  for (auto &e : s->features.ev)
    if (e) (void)hipEventDestroy(e);
  for (auto *ev : {s->regions.ev, s->clusters.ev, s->clusters.matrix.ev, s->joint.ev, s->joint.fold.ev,
                   s->joint_path.ev, s->joint_path.fold.ev, s->joint_labels.ev, s->heldout.ev,
                   s->heldout.fold.ev})
    for (int k = 0; k < 2; k++)
      if (ev[k]) (void)hipEventDestroy(ev[k]);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  if (s->stream2) (void)hipStreamDestroy(s->stream2);
  if (s->started) (void)hipHostFree(s->started);
  delete s;
}

extern "C" const char *peakseg_hip_problem_set_kernel_build(psd_problem_set *s) {
  if (s->run.plan.throughput && s->run.plan.n_lat_mixed > 0) return s->run.plan.packed ? "lat+pk" : "lat+thr";
  return s->run.plan.throughput ? (s->run.plan.packed ? "pk" : "thr") : "lat";
}

extern "C" int peakseg_hip_problem_set_solve_stats(psd_problem_set *s, int *launches,
                                                   unsigned long long *steps_run) {
  if (!s) return -1;
  if (launches) *launches = s->run.launches;
  if (steps_run) *steps_run = s->run.steps_run;
  return 0;
}

extern "C" int peakseg_hip_problem_set_arena_stats(psd_problem_set *s,
                                                   unsigned long long *block_pieces, int *blocks,
                                                   int *blocks_added_live) {
  if (!s) return -1;
  if (block_pieces) *block_pieces = 1ull << s->d.ar_block_log2;
  if (blocks) *blocks = (int)s->arena_blocks.size();
  if (blocks_added_live) *blocks_added_live = (int)s->run.live_blocks_added;
  return 0;
}

extern "C" unsigned long long peakseg_hip_problem_set_bytes(psd_problem_set *s) {
  return s ? s->bytes : 0;
}

extern "C" unsigned long long peakseg_hip_problem_set_arena_bytes_used(psd_problem_set *s) {
  return s ? s->arena_used * 20ull : 0;
}

extern "C" int peakseg_hip_problem_set_set_penalty(psd_problem_set *s, int p, double penalty) {
  if (!s || p < 0 || p >= s->n_problems) return -1;
  if (hipSetDevice(s->device) != hipSuccess) return -1;
  s->prob_penalty[(size_t)p] = penalty;
  if (hipMemcpyAsync(const_cast<double *>(s->d.prob_penalty) + p, &penalty, sizeof(double),
                     hipMemcpyHostToDevice, s->stream) != hipSuccess ||
      hipStreamSynchronize(s->stream) != hipSuccess) { /* (in order with the set's launches) */
    set_error("penalty upload failed");
    return -1;
  }
  s->solved = false;
  return 0;
}

extern "C" int peakseg_hip_problem_set_result(psd_problem_set *s, int p, psd_result *out) {
  if (!s || !s->solved || p < 0 || p >= s->n_problems) return -1;
  const psd::ProbResult &r = s->results[(size_t)p];
  out->status = r.status == 0 ? 0 : ERROR_DEVICE_SOLVER;
  out->kernel_status = r.status;
  out->n_segments = r.n_segments;
  out->n_peaks = (r.n_segments - 1) / 2;
  out->n_equality_constraints = r.n_equality;
  out->max_intervals = r.max_intervals;
  out->total_intervals = r.total_intervals;
  out->best_cost = r.best_cost;
  out->n_serial_env = r.n_serial_env;
  out->step_reached = r.step_reached;
  out->spill_steps = r.spill_steps;
  return 0;
}

extern "C" int peakseg_hip_problem_set_segments(psd_problem_set *s, int p, int capacity,
                                                int *seg_start, double *seg_mean) {
  if (!s || !s->solved || p < 0 || p >= s->n_problems) return -1;
  const psd::ProbResult &r = s->results[(size_t)p];
  if (r.status != 0 || r.n_segments > capacity) return -1;
  size_t n = (size_t)r.n_segments;
  long long off = s->prob_seg_off[(size_t)p];
  if (hipMemcpy(seg_start, s->d.seg_start + off, n * sizeof(int), hipMemcpyDeviceToHost) !=
          hipSuccess ||
      hipMemcpy(seg_mean, s->d.seg_mean + off, n * sizeof(double), hipMemcpyDeviceToHost) !=
          hipSuccess) {
    set_error("segment table download failed");
    return -1;
  }
  return r.n_segments;
}

extern "C" int peakseg_hip_problem_set_checkpoint_interval(psd_problem_set *s) {
  return s ? s->ckpt_interval : 0;
}

extern "C" int peakseg_hip_problem_set_export_db(psd_problem_set *s, int p, const int *chromEnd,
                                                 const char *path) {
  if (!s || !s->solved || p < 0 || p >= s->n_problems) return -1;
  if (s->ckpt_interval > 0) return -1; /* checkpointed store: the functions were not all kept */
  int N = s->contig_n[(size_t)s->prob_contig[(size_t)p]];
  std::vector<unsigned long long> ref((size_t)2 * N);
  if (hipMemcpy(ref.data(), s->d.fn_ref + s->prob_fn_off[(size_t)p], ref.size() * 8,
                hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  FILE *f = fopen(path, "wb");
  if (!f) return -1;
  /* table of 2N std::streampos (16 bytes: offset + zero state), then records in the order
   * the reference writes them: down_0, then (down_t, up_t) for t >= 1 (drv:388-392) */
  std::vector<long long> table((size_t)4 * N, 0);
  long long pos = 32ll * N;
  std::vector<char> body;
  /* the records are read from host copies of the arena's blocks (two at a time: the two chains
   * of a problem write into different chunk runs), not with three small copies per function */
  const int blg = s->d.ar_block_log2;
  const size_t block_bytes = arena_block_bytes(s);
  struct HostBlock {
    size_t blk = (size_t)-1;
    std::vector<char> bytes;
    unsigned long long used = 0;
  } cache[2];
  unsigned long long tick = 0;
  auto host_block = [&](size_t blk) -> const char * {
    for (auto &c : cache)
      if (c.blk == blk) {
        c.used = ++tick;
        return c.bytes.data();
      }
    HostBlock &c = cache[0].used <= cache[1].used ? cache[0] : cache[1];
    if (blk >= s->arena_blocks.size()) return nullptr;
    c.bytes.resize(block_bytes);
    if (hipMemcpy(c.bytes.data(), s->arena_blocks[blk].base, block_bytes, hipMemcpyDeviceToHost) !=
        hipSuccess)
      return nullptr;
    c.blk = blk;
    c.used = ++tick;
    return c.bytes.data();
  };
  for (int t = 0; t < N; t++) {
    for (int which = 0; which < 2; which++) {
      int element = which == 0 ? N + t : t;
      if (which == 1 && t == 0) continue;
      unsigned long long r = ref[(size_t)element];
      unsigned long long off = r >> psd::FN_COUNT_BITS;
      int n = (int)(r & ((1ull << psd::FN_COUNT_BITS) - 1));
      /* the record's block and its three arrays (fpop_types.h) */
      const size_t w = (size_t)(off & ((1ull << blg) - 1ull));
      const char *bb = host_block((size_t)(off >> blg));
      if (!bb || w + (size_t)n > ((size_t)1 << blg)) {
        fclose(f);
        return -1;
      }
      const double *mx = (const double *)bb + w;
      const double *prv = (const double *)(bb + ((size_t)8 << blg)) + w;
      const int *di = (const int *)(bb + ((size_t)16 << blg)) + w;
      table[(size_t)2 * element] = pos;
      int size = 20 * n + 8;
      size_t at = body.size();
      body.resize(at + 4 + (size_t)size);
      char *q = body.data() + at;
      memcpy(q, &size, 4);
      q += 4;
      memcpy(q, &n, 4);
      q += 4;
      memcpy(q, &chromEnd[t], 4);
      q += 4;
      for (int i = 0; i < n; i++) {
        memcpy(q, &mx[(size_t)i], 8);
        q += 8;
        memcpy(q, &di[(size_t)i], 4);
        q += 4;
        memcpy(q, &prv[(size_t)i], 8);
        q += 8;
      }
      pos += 4 + size;
    }
  }
  bool ok = fwrite(table.data(), 8, table.size(), f) == table.size() &&
            fwrite(body.data(), 1, body.size(), f) == body.size();
  ok = fclose(f) == 0 && ok;
  return ok ? 0 : -1;
}

/* Tests: parse a bedGraph file with the fast path (use_fast != 0) or with sscanf only, and
 * report the status, the line count and an FNV-1a hash of everything parsed. */
extern "C" int peakseg_hip_parse_probe(const char *path, int use_fast, int *n_lines,
                                       unsigned long long *hash) {
  Coverage cv;
  int st = read_bedGraph_impl(path, cv, use_fast != 0);
  unsigned long long h = 1469598103934665603ull;
  auto mix = [&h](const void *q, size_t n) {
    const unsigned char *b = (const unsigned char *)q;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  };
  if (st == 0) {
    mix(cv.chromEnd.data(), cv.chromEnd.size() * 4);
    mix(cv.count.data(), cv.count.size() * 4);
    mix(cv.weight.data(), cv.weight.size() * 4);
    mix(cv.chrom.data(), cv.chrom.size());
    mix(&cv.first_chromStart, 4);
    mix(&cv.cum_weight, 8);
    mix(&cv.cum_weighted_count, 8);
    mix(&cv.min_log_mean, 8);
    mix(&cv.max_log_mean, 8);
  }
  if (n_lines) *n_lines = cv.n();
  if (hash) *hash = h;
  return st;
}

/* diagnostic builds (-DPSD_PROFILE) only: per-wave cycle counters of the forward kernel */
extern "C" int peakseg_hip_problem_set_profile(psd_problem_set *s, int p, long long *out) {
#ifdef PSD_PROFILE
  if (!s || !s->solved || p < 0 || p >= s->n_problems) return -1;
  if (hipMemcpy(out, s->d.prof + (size_t)p * 2 * psd::N_PROF, sizeof(long long) * 2 * psd::N_PROF,
                hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  return psd::N_PROF;
#else
  (void)s, (void)p, (void)out;
  return -1;
#endif
}

extern "C" int peakseg_hip_math_probe(int op, int n, const double *x, double *y) {
  if (peakseg_hip_device_count() <= 0) {
    set_error("no HIP device visible (this library has no CPU fallback)");
    return ERROR_NO_HIP_DEVICE;
  }
  if (n <= 0) return 0;
  double *dx = nullptr, *dy = nullptr;
  const size_t n_in = op >= 2 ? (size_t)2 * (size_t)n : (size_t)n; /* (division: two operands) */
  HIP_TRY(hipMalloc(&dx, n_in * 8));
  HIP_TRY(hipMalloc(&dy, (size_t)n * 8));
  HIP_TRY(hipMemcpy(dx, x, n_in * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(psd::lat::math_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t) nullptr, op, n, dx, dy);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(y, dy, (size_t)n * 8, hipMemcpyDeviceToHost));
  (void)hipFree(dx);
  (void)hipFree(dy);
  return 0;
}

extern "C" int peakseg_hip_math_forms_probe(int form, int set, int n, const double *x0,
                                            const double *x1, const double *z, double *y0,
                                            double *y1, double *lz, int *rare) {
  if (peakseg_hip_device_count() <= 0) {
    set_error("no HIP device visible (this library has no CPU fallback)");
    return ERROR_NO_HIP_DEVICE;
  }
  if (form < 0 || form >= psd::forms_probe::N_FORMS || set < 0 || set >= psd::forms_probe::N_SETS ||
      n < 0) {
    set_error("math forms probe: form %d, set %d or n %d out of range", form, set, n);
    return -1;
  }
  if (n == 0) return 0;
  /* three inputs, three outputs and the records: n elements each; an input the caller leaves out
   * (NULL: the form does not read it) is zeros */
  const size_t bytes = (size_t)n * 8;
  double *d[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int *d_rare = nullptr;
  for (auto &q : d) {
    HIP_TRY(hipMalloc(&q, bytes));
    HIP_TRY(hipMemset(q, 0, bytes));
  }
  HIP_TRY(hipMalloc(&d_rare, (size_t)n * 4));
  HIP_TRY(hipMemset(d_rare, 0, (size_t)n * 4));
  const double *in[3] = {x0, x1, z};
  for (int k = 0; k < 3; k++)
    if (in[k]) HIP_TRY(hipMemcpy(d[k], in[k], bytes, hipMemcpyHostToDevice));
  const unsigned blocks = ((unsigned)n + psd::forms_probe::THREADS - 1u) / psd::forms_probe::THREADS;
  hipLaunchKernelGGL(psd::forms_probe::math_forms_probe_kernel, dim3(blocks),
                     dim3(psd::forms_probe::THREADS), 0, (hipStream_t) nullptr, form, set, n, d[0],
                     d[1], d[2], d[3], d[4], d[5], d_rare);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  double *out[3] = {y0, y1, lz};
  for (int k = 0; k < 3; k++)
    if (out[k]) HIP_TRY(hipMemcpy(out[k], d[3 + k], bytes, hipMemcpyDeviceToHost));
  if (rare) HIP_TRY(hipMemcpy(rare, d_rare, (size_t)n * 4, hipMemcpyDeviceToHost));
  for (auto &q : d) (void)hipFree(q);
  (void)hipFree(d_rare);
  return 0;
}

extern "C" int peakseg_hip_problem_set_park_stats(psd_problem_set *s, int *parks,
                                                  unsigned long long *overflow_pool_pieces) {
  if (!s) return -1;
  if (parks) *parks = s->run.parks;
  if (overflow_pool_pieces) *overflow_pool_pieces = s->run.park_pool_pieces;
  return 0;
}

/* shader cycles the problem's workgroup ran in the last launch that touched it */
extern "C" long long peakseg_hip_problem_set_cycles(psd_problem_set *s, int p) {
  if (!s || !s->solved || p < 0 || p >= s->n_problems) return -1;
  return s->results[(size_t)p].cycles;
}

/* data points per second one problem advanced at in this process's last clean single-build
 * solves (what the mixed-launch planner reasons with); the defaults before any */
extern "C" void peakseg_hip_measured_rates(double *lat_rate, double *thr_rate) {
  if (lat_rate) *lat_rate = g_lat_rate.load();
  if (thr_rate) *thr_rate = g_thr_rate.load();
}

/* the bound on the polls of a wait between waves (tests/test_gpu_round4.py) and, in builds with
 * -DPSD_SPIN_STATS, the largest poll count a problem's waves saw */
extern "C" long long peakseg_hip_spin_limit(void) { return (long long)psd::lat::WAIT_SPIN_LIMIT; }
extern "C" int peakseg_hip_problem_set_max_spin(psd_problem_set *s, int p) {
  if (!s || !s->solved || p < 0 || p >= s->n_problems) return -1;
  return s->results[(size_t)p].max_spin;
}

/* builds with -DPSD_LOOP_STATS (tests): per chain wave, the data points of the problem's last
 * launch taken inside the inner loop of the usual data point, those taken by the general code
 * and the entries into the inner loop, six numbers; returns 6, or 0 in every other build */
extern "C" int peakseg_hip_problem_set_loop_stats(psd_problem_set *s, int p, int *out) {
  if (!s || !s->solved || p < 0 || p >= s->n_problems || !out) return -1;
#ifdef PSD_LOOP_STATS
  for (int i = 0; i < 6; i++) out[i] = s->results[(size_t)p].loop_stats[i];
  return 6;
#else
  return 0;
#endif
}

/* ---- the dynamic programs of a call on the devices, the file-level solver (the reference's
 *      boundary), the directory-level batch with the cache protocol, the penalty searches ------ */
#include "peakseg_fanout.h"
#include "peakseg_files.h"
#include "peakseg_dir.h"
#include "peakseg_search.h"

extern "C" char *PeakSegFPOP_status_message(int status, const char *bedGraph, const char *penalty,
                                            const char *db, char *buf, size_t buf_len) {
  if (!buf || buf_len == 0) return buf;
  buf[0] = 0;
#define PSD_MESSAGE(code, ...) case code: snprintf(buf, buf_len, __VA_ARGS__); break
  switch (status) { /* texts of /root/reference/src/interface.cpp:16-55 */
    case 0:
      break;
    PSD_MESSAGE(ERROR_PENALTY_NOT_FINITE, "penalty=%s but must be finite", penalty);
    PSD_MESSAGE(ERROR_PENALTY_NEGATIVE, "penalty=%s must be non-negative", penalty);
    PSD_MESSAGE(ERROR_UNABLE_TO_OPEN_BEDGRAPH, "unable to open input file for reading %s", bedGraph);
    PSD_MESSAGE(ERROR_NOT_ENOUGH_COLUMNS,
                "each line of input data file %s should have exactly four columns", bedGraph);
    PSD_MESSAGE(ERROR_NON_INTEGER_DATA, "fourth column of input data file %s should be integer",
                bedGraph);
    PSD_MESSAGE(ERROR_INCONSISTENT_CHROMSTART_CHROMEND,
                "there should be no gaps (columns 2-3) in input data file %s", bedGraph);
    PSD_MESSAGE(ERROR_WRITING_COST_FUNCTIONS, "unable to write to cost function database file %s", db);
    PSD_MESSAGE(ERROR_WRITING_LOSS_OUTPUT, "unable to write to loss output file %s_penalty=%s_loss.tsv",
                bedGraph, penalty);
    PSD_MESSAGE(ERROR_WRITING_SEGMENTS_OUTPUT,
                "unable to write to segments output file %s_penalty=%s_segments.bed", bedGraph, penalty);
    PSD_MESSAGE(ERROR_NO_DATA, "input file %s contains no data", bedGraph);
    PSD_MESSAGE(ERROR_PENALTY_NOT_NUMERIC,
                "penalty string '%s' is not numeric; it should be convertible to double", penalty);
    PSD_MESSAGE(ERROR_NO_HIP_DEVICE,
                "error code %d: no HIP device (MI355X) is visible and this solver has no CPU path", status);
    PSD_MESSAGE(ERROR_DENSE_ARGUMENTS,
                "error code %d: dense counts that cannot be solved (2^31 or more bases, a negative "
                "count, counts that sum to 2^53 or more, or 2^30 or more runs in a contig)", status);
    PSD_MESSAGE(ERROR_READS_ARGUMENTS,
                "error code %d: aligned reads that cannot be piled up (an empty or negative extent, a "
                "read with chromStart >= chromEnd or a negative count, or counts that sum to 2^31 or "
                "more in a contig)", status);
    PSD_MESSAGE(ERROR_LABEL_ARGUMENTS,
                "error code %d: labels that cannot be counted (a negative number of labels, a NULL or "
                "misaligned array, a label with chromStart >= chromEnd or an annotation code outside "
                "0..3)", status);
    PSD_MESSAGE(ERROR_FEATURE_ARGUMENTS,
                "error code %d: coverage statistics that cannot be computed (a negative number of "
                "ranks or more than peakseg_hip_coverage_stats_max_ranks, or a rank outside "
                "0 .. bases - 1 of its contig)", status);
    PSD_MESSAGE(ERROR_FIT_ARGUMENTS,
                "error code %d: a penalty model that cannot be fitted (a bad shape, a feature that is "
                "not finite, a NaN limit or lo > hi, a row with both limits infinite, a fold outside "
                "its range or one that leaves no training row, regularizations that do not increase, "
                "a gram_lambda_max, threshold or max_iterations that is not positive -- or no "
                "regularization whose fits all converged)", status);
    PSD_MESSAGE(ERROR_REGION_ARGUMENTS,
                "error code %d: regions or groups that cannot be served (a negative number of regions "
                "or groups, a NULL or misaligned array, a region with chromStart >= chromEnd, or a "
                "problem in a group outside -1 .. n_groups - 1)", status);
    PSD_MESSAGE(ERROR_HELDOUT_ARGUMENTS,
                "error code %d: pairs that cannot be scored (a negative number of pairs, a NULL or "
                "misaligned array, a problem or contig out of range, a scale that is not finite and "
                "positive, or a contig that has not the bases of its problem's contig) or folds that "
                "cannot be made (a number of folds that is not 2, 4 or 8, or a base whose count "
                "exceeds peakseg_hip_fold_max_count)", status);
    PSD_MESSAGE(ERROR_STRAND_ARGUMENTS,
                "error code %d: stranded reads that cannot be served (a strand that is neither +1 nor "
                "-1, a NULL strand array, a max_shift outside 0 .. peakseg_hip_xcorr_max_shift, a "
                "fragment_length below 1, or an extent with hi <= lo)", status);
    PSD_MESSAGE(ERROR_DEDUP_ARGUMENTS,
                "error code %d: a duplicate removal that cannot be served (keep below 1, an unknown "
                "by, five_prime without strands, 2^31 or more rows in one call, or an output that "
                "overlaps an input)", status);
    default:
      snprintf(buf, buf_len, "error code %d", status);
      break;
  }
#undef PSD_MESSAGE
  return buf;
}
