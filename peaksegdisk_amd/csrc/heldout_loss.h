/* heldout_loss.h -- the Poisson loss of a solved model on ANOTHER contig of the same set: what a
 * penalty chosen by thinning is scored with (the definition is the contract of
 * peakseg_hip_problem_set_pack_heldout_loss in include/peaksegdisk_hip.h).
 *
 * A pair is (problem p, contig c, scale a); contig c has the bases of p's own contig.  Row k of p's
 * segments table has [start_k, end_k), B_k = end_k - start_k bases and mean_k; Y_k is the sum of
 * contig c's per-base counts over [start_k, end_k).  With x_k = a * mean_k the row's term is
 *   x_k B_k - Y_k log(x_k)   Y_k > 0 and mean_k > 0
 *   x_k B_k                  Y_k == 0 (no logarithm is taken)
 *   +Inf                     mean_k == 0 and Y_k > 0 (counted in zero_mean_rows)
 * and the pair's loss is the sum of its rows' terms.
 *
 * The launches of a call, however many pairs and rows there are (the host side is
 * peakseg_heldout.h; the three of region_stats.h lie between rows_kernel and loss_kernel):
 *   pairs_kernel  a thread per pair: the pair is checked (the first bad one is kept in the call's
 *                 check word: key = ~index with the reason in the low bits, a 64-bit max on a zeroed
 *                 word), its row count goes through the workgroup's scan (off[], block_sum[]) and
 *                 into the call's total.
 *   (region_stats.h's scan_top_kernel makes block_sum[] the second level of the prefix.)
 *   rows_kernel   a thread per (pair, row): the row's pair from the two levels of the prefix (as
 *                 fold_kernel finds an item's region), and the row as a flat region of contig c.
 *   loss_kernel   a workgroup per pair.  Lane t adds the terms of rows t, t + THREADS, ... in that
 *                 order to its own sum; the lanes of a wave are added by the tree of distances 32,
 *                 16, .. 1, lane 0 of every wave leaves its sum in LDS, and thread 0 adds waves 1,
 *                 2, 3 to its own in that order.  The order of additions depends on the row count
 *                 only; a term passes through at most ceil(rows / THREADS) + 6 + 3 of them.  No
 *                 floating-point atomics.  bases, sum and zero_mean_rows are integers and take the
 *                 same way.
 * Every product and difference is rounded once (-ffp-contract=off); the logarithm is psd_log, whose
 * tables the workgroup copies to LDS first.
 * The kernels are templates (`template <int = 0>`) for their place in the code object: joint_path.h
 * says why.
 * Written against psd_platform.h only: the SIMT emulator of tests/emu runs this source. */
#ifndef PSD_HELDOUT_LOSS_H
#define PSD_HELDOUT_LOSS_H

#include <math.h>

#include "psd_platform.h"
#include "region_stats.h"

namespace psd {
namespace heldout {

constexpr int THREADS = psd::regions::THREADS;
constexpr int WAVES = THREADS / WAVE;

typedef unsigned long long u64;

/* why a pair is refused (the low bits of the check word) */
constexpr int BAD_PROBLEM = 1, BAD_CONTIG = 2, BAD_SCALE = 3, BAD_BASES = 4;
constexpr int REASON_BITS = 3;

/* what the kernels need of a problem */
struct Problem {
  long long seg_off; /* its table in seg_start / seg_mean */
  long long run0;    /* first run of its contig in run_end[] */
  long long bases;   /* bases of its contig */
  int rows;          /* rows of its table (0: its solve reported a failure) */
  int pad;
};

/* the head of a call: what the host reads after pairs_kernel */
struct Head {
  u64 check;       /* 0, or the first bad pair */
  long long rows;  /* rows of all pairs */
};

PSD_D u64 check_key(long long pair, int reason) {
  return ((~(u64)pair) << REASON_BITS) | (u64)reason;
}

/* 0, or why the pair cannot be scored */
PSD_D int pair_reason(int p, int c, double a, const Problem *problems, int n_problems,
                      const long long *contig_bases, int n_contigs) {
  if (p < 0 || p >= n_problems) return BAD_PROBLEM;
  if (c < 0 || c >= n_contigs) return BAD_CONTIG;
  if (!(a > 0.0) || !(a < INFINITY)) return BAD_SCALE;
  if (contig_bases[c] != problems[p].bases) return BAD_BASES;
  return 0;
}

/* A thread per pair i < n.  No thread leaves before the scan. */
template <int = 0>
__global__ __launch_bounds__(THREADS) void pairs_kernel(
    long long n, const int *problem, const int *contig, const double *scale, const Problem *problems,
    int n_problems, const long long *contig_bases, int n_contigs, int *off, long long *block_sum,
    Head *head) {
  PSD_LDS int w_tot[WAVES];
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  int rows = 0;
  if (i < n) {
    const int p = problem[i];
    const int why = pair_reason(p, contig[i], scale[i], problems, n_problems, contig_bases, n_contigs);
    if (why)
      atomic_max_u64(&head->check, check_key(i, why));
    else
      rows = problems[p].rows;
  }
  int total;
  const int before = psd::regions::block_scan(rows, w_tot, total);
  if (i < n) off[i] = before;
  if (threadIdx.x == 0) {
    block_sum[blockIdx.x] = total;
    if (total) atomic_add_i64(&head->rows, (long long)total);
  }
}

/* A thread per row g of all pairs (head->rows of them): flat region g is row k of its pair's model,
 * on the pair's contig.  Rows come in the reference's order: row 0 is the last segment. */
template <int = 0>
__global__ __launch_bounds__(THREADS) void rows_kernel(
    long long n, const int *problem, const int *contig, const Problem *problems, const int *off,
    const long long *block_sum, const Head *head, const int *seg_start, const int *run_end,
    int *flat_start, int *flat_end, int *flat_contig) {
  const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (g >= head->rows) return;
  const long long nb = (n + THREADS - 1) / THREADS;
  const long long blk = psd::regions::last_at_most(block_sum, nb, g);
  const long long rest = g - block_sum[blk];
  const long long i0 = blk * THREADS;
  const long long in_blk = n - i0 < THREADS ? n - i0 : THREADS;
  const long long i = i0 + psd::regions::last_at_most(off + i0, in_blk, rest);
  const Problem q = problems[problem[i]];
  const long long k = rest - off[i];
  const int s = seg_start[q.seg_off + k];
  flat_start[g] = s < 0 ? 0 : run_end[q.run0 + s];
  if (k == 0) {
    flat_end[g] = (int)q.bases;
  } else {
    const int sp = seg_start[q.seg_off + k - 1];
    flat_end[g] = sp < 0 ? 0 : run_end[q.run0 + sp];
  }
  flat_contig[g] = contig[i];
}

/* the term of a row: x = a * mean, B bases, Y the held-out sum; zero_mean: the +Inf case */
PSD_D double row_term(double a, double mean, long long B, long long Y, int &zero_mean) {
  const double x = a * mean;
  const double xb = x * (double)B;
  zero_mean = 0;
  if (Y == 0) return xb;
  if (!(mean > 0.0)) {
    zero_mean = 1;
    return INFINITY;
  }
  const double yl = (double)Y * psd_log(x);
  return xb - yl;
}

/* A workgroup per pair; bases[] and sum[] are the fold's columns of the flat regions. */
template <int = 0>
__global__ __launch_bounds__(THREADS) void loss_kernel(
    long long n, const int *problem, const double *scale, const Problem *problems, const int *off,
    const long long *block_sum, const double *seg_mean, const int *bases, const long long *sum,
    double *out_loss, int *out_rows, long long *out_bases, long long *out_sum, int *out_zero) {
  PSD_LDS double w_loss[WAVES];
  PSD_LDS long long w_bases[WAVES], w_sum[WAVES];
  PSD_LDS int w_zero[WAVES];
  psd_tables_init(); /* log tables -> LDS */
  const long long i = blockIdx.x;
  const int tid = (int)threadIdx.x, lane = lane_id(), wave = wave_id();
  const Problem q = problems[problem[i]];
  const double a = scale[i];
  const long long row0 = psd::regions::scan_at(off, block_sum, i);
  double loss = 0.0;
  long long nb = 0, ny = 0;
  int nz = 0;
  for (int k = tid; k < q.rows; k += THREADS) {
    const long long B = bases[row0 + k], Y = sum[row0 + k];
    int z;
    loss = loss + row_term(a, seg_mean[q.seg_off + k], B, Y, z);
    nb += B;
    ny += Y;
    nz += z;
  }
  for (int d = WAVE / 2; d > 0; d >>= 1) {
    const int src = lane + d < WAVE ? lane + d : lane;
    const double ol = shfl_d(loss, src);
    const long long ob = (long long)psd::stats::shfl_u64((u64)nb, src);
    const long long oy = (long long)psd::stats::shfl_u64((u64)ny, src);
    const int oz = shfl_i(nz, src);
    if (lane + d < WAVE) {
      loss = loss + ol;
      nb += ob;
      ny += oy;
      nz += oz;
    }
  }
  if (lane == 0) {
    w_loss[wave] = loss;
    w_bases[wave] = nb;
    w_sum[wave] = ny;
    w_zero[wave] = nz;
  }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < WAVES; k++) {
      loss = loss + w_loss[k];
      nb += w_bases[k];
      ny += w_sum[k];
      nz += w_zero[k];
    }
    out_loss[i] = loss;
    out_rows[i] = q.rows;
    out_bases[i] = nb;
    out_sum[i] = ny;
    out_zero[i] = nz;
  }
}

}  // namespace heldout
}  // namespace psd
#endif
