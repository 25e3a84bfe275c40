/* region_stats.h -- the coverage of caller-chosen regions from the runs resident in HBM: for every
 * region [rs, re) of a contig the bases of it that lie inside the contig, the sum of the per-base
 * counts over them (a run cut by an edge counts with the cut length only) and the largest count of
 * a run that meets it.  The same fold serves the cluster-by-member matrix of
 * peak_clusters.h, whose regions are the clusters: the fold exists once.
 *
 * Regions come in any order, may overlap, and may lie partly or wholly outside their contig.  With
 * a = max(rs - first, 0) and b = min(re - first, B) for a contig of B bases, the runs that meet the
 * region are j0 .. j1: j0 the first run that ends after a, j1 the first that ends at or after b.
 *
 * Three launches per call, however many contigs and regions there are; no workgroup waits for
 * another:
 *   locate_kernel    a thread per region: two binary searches of the contig's run_end[] (as
 *                    label_errors.h's runs_before).  A region of at most SMALL runs is finished on
 *                    the spot by its thread: no workgroup, no atomic.  A longer one gets its two
 *                    edge runs (the only cut ones) from its thread, which writes them to sum[] and
 *                    max[], and leaves its whole runs j0 + 1 .. j1 - 1 as a span and a number of
 *                    tiles: the tiles of TILE runs of the contig's 16-byte aligned range
 *                    (segment_stats.h) that the span meets.  The workgroup scans its threads' tile
 *                    counts (off[]) and writes their sum (block_sum[]).
 *   scan_top_kernel  one workgroup: the exclusive prefix sums of block_sum[] and the total.
 *   fold_kernel      a fixed number of workgroups, each taking the items blockIdx.x,
 *                    blockIdx.x + gridDim.x, ... of the work list of (region, tile) pairs, which
 *                    exists only as the two levels of prefix sums: an item finds its region by a
 *                    binary search of block_sum[] and one of the 256 off[] of that block (uniform
 *                    addresses).  Every lane loads 16 aligned bytes of count[] and of weight[],
 *                    lanes and waves are combined by shuffles and LDS, and the workgroup adds once:
 *                    a 64-bit add to sum[] and a 32-bit max to max[].  Integer atomics commute: the
 *                    results do not depend on the schedule.
 * So a region over a contig of millions of runs is folded by as many workgroups as it has tiles,
 * and very many regions of a few runs cost a thread each.  A region of SMALL + 1 .. TILE runs costs
 * one item whose lanes are mostly idle: the price of having one fold.
 * Algorithmic traffic: per region 8 B of rs / re, 2 ceil(log2(R + 1)) probes of run_end for R runs,
 * 12 B per run of a small region or 24 B for the two edges, 16 B of span, 4 B of off and 16 B of
 * bases / sum / max written; per item about log2(regions / 256) + 8 probes of the prefix sums, 16 B
 * of span, 8 B per run of count and weight, and two atomics.
 * Written against psd_platform.h only: the SIMT emulator of tests/emu runs this source. */
#ifndef PSD_REGION_STATS_H
#define PSD_REGION_STATS_H

#include "psd_platform.h"
#include "segment_stats.h"

namespace psd {
namespace regions {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;
constexpr int TILE = THREADS * 4; /* runs of a tile: four per lane */
constexpr int SMALL = 16;         /* a region of at most this many runs is its thread's alone */

typedef unsigned long long u64;
typedef psd::dense::Quad Quad;

struct Contig {
  const gint *start, *end; /* the contig's regions (not read when the call has flat arrays) */
  long long reg0;          /* index of its first region among all regions */
  long long run0, n_runs;  /* its runs in run_end[] / count[] / weight[] */
  long long first, bases;  /* chromStart of its first base, and its bases */
};

/* the whole runs of a long region: lo .. hi - 1 of the contig whose runs begin at run0 */
struct Span {
  long long run0;
  int lo, hi;
};

/* the exclusive prefix sum of v over the threads of the workgroup, and the sum of all; every thread
 * of the workgroup calls it; w_tot: WAVES ints of LDS */
PSD_D int block_scan(int v, int *w_tot, int &total) {
  const int lane = lane_id(), wave = wave_id();
  int inc = v;
  for (int d = 1; d < WAVE; d <<= 1) {
    const int o = shfl_i(inc, lane >= d ? lane - d : lane);
    if (lane >= d) inc += o;
  }
  if (lane == WAVE - 1) w_tot[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
  for (int k = 0; k < WAVES; k++) {
    if (k < wave) before += w_tot[k];
    all += w_tot[k];
  }
  __syncthreads(); /* (w_tot may be written again) */
  total = all;
  return before + inc - v;
}

/* entry j of a two-level prefix sum: off[] within workgroups of THREADS, block_sum[] before them */
PSD_D long long scan_at(const int *off, const long long *block_sum, long long j) {
  return block_sum[j / THREADS] + off[j];
}

/* the runs of a contig whose end is below x (or, with `or_equal`, at most x) */
PSD_D long long runs_ending(const int *run_end, long long n_runs, long long x, bool or_equal) {
  long long lo = 0, hi = n_runs;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    const long long e = run_end[mid];
    if (e < x || (or_equal && e == x))
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

/* A thread per region g < n.  Regions of contig c are reg_off[c] .. reg_off[c + 1] - 1 and lie in
 * the contig's own arrays; or (flat_contig != NULL) region g is flat_start[g], flat_end[g] of contig
 * flat_contig[g].  check (may be NULL): per contig, ~index of its first region with rs >= re.  No
 * thread leaves before the scan. */
__global__ __launch_bounds__(THREADS) void locate_kernel(
    const Contig *contigs, const long long *reg_off, int n_contigs, long long n, const int *flat_start,
    const int *flat_end, const int *flat_contig, const int *run_end, const int *count,
    const int *weight, int *bases, long long *sum, int *mx, Span *span, int *off,
    long long *block_sum, u64 *check) {
  PSD_LDS int w_tot[WAVES];
  const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;
  int tiles = 0;
  if (g < n) {
    int c, rs, re;
    if (flat_contig) {
      c = flat_contig[g];
      rs = flat_start[g];
      re = flat_end[g];
    } else {
      int lo = 0, hi = n_contigs - 1; /* the last contig whose first region is not beyond g */
      while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (reg_off[mid] <= g)
          lo = mid;
        else
          hi = mid - 1;
      }
      c = lo;
      const long long i = g - contigs[c].reg0;
      rs = contigs[c].start[i];
      re = contigs[c].end[i];
      if (rs >= re && check) atomic_max_u64(check + c, ~(u64)i);
    }
    const Contig *k = contigs + c;
    const long long run0 = k->run0, n_runs = k->n_runs;
    long long a = (long long)rs - k->first, b = (long long)re - k->first;
    a = a > 0 ? a : 0;
    b = b < k->bases ? b : k->bases;
    Span sp;
    sp.run0 = run0;
    sp.lo = sp.hi = 0;
    long long s = 0;
    int m = 0;
    if (b > a && n_runs > 0) {
      const int *ends = run_end + run0, *cnt = count + run0, *wgt = weight + run0;
      const long long j0 = runs_ending(ends, n_runs, a, true);
      long long j1 = runs_ending(ends, n_runs, b, false);
      if (j1 >= n_runs) j1 = n_runs - 1; /* (b <= bases = the last run's end: not taken) */
      if (j1 - j0 < SMALL) {
        for (long long j = j0; j <= j1; j++) {
          const long long e = ends[j], st = e - wgt[j];
          const long long len = (e < b ? e : b) - (st > a ? st : a);
          const int v = cnt[j];
          s += (long long)v * len;
          m = v > m ? v : m;
        }
      } else {
        const int v0 = cnt[j0], v1 = cnt[j1];
        s = (long long)v0 * ((long long)ends[j0] - a) +
            (long long)v1 * (b - ((long long)ends[j1] - wgt[j1]));
        m = v0 > v1 ? v0 : v1;
        const long long lead = run0 & 3;
        sp.lo = (int)(j0 + 1);
        sp.hi = (int)j1;
        tiles = (int)((j1 - 1 + lead) / TILE - (j0 + 1 + lead) / TILE + 1);
      }
    }
    bases[g] = b > a ? (int)(b - a) : 0;
    sum[g] = s;
    mx[g] = m;
    span[g] = sp;
  }
  int total;
  const int before = block_scan(tiles, w_tot, total);
  if (g < n) off[g] = before;
  if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

/* One workgroup: block_sum[0 .. nb) becomes its exclusive prefix sums, block_sum[nb] the total. */
__global__ __launch_bounds__(THREADS) void scan_top_kernel(long long *block_sum, long long nb) {
  PSD_LDS long long part[THREADS];
  const int tid = (int)threadIdx.x;
  const long long per = (nb + THREADS - 1) / THREADS;
  const long long lo = tid * per < nb ? tid * per : nb, hi = lo + per < nb ? lo + per : nb;
  long long s = 0;
  for (long long i = lo; i < hi; i++) s += block_sum[i];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int k = 0; k < THREADS; k++) {
      const long long t = part[k];
      part[k] = run;
      run += t;
    }
    block_sum[nb] = run;
  }
  __syncthreads();
  long long run = part[tid];
  for (long long i = lo; i < hi; i++) {
    const long long t = block_sum[i];
    block_sum[i] = run;
    run += t;
  }
}

/* the last index in [0, n) whose entry is at most x; entry 0 is */
template <class T>
PSD_D long long last_at_most(const T *v, long long n, long long x) {
  long long lo = 0, hi = n - 1;
  while (lo < hi) {
    const long long mid = (lo + hi + 1) >> 1;
    if ((long long)v[mid] <= x)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

/* Item after item of the work list (the header has the scheme); n: regions. */
__global__ __launch_bounds__(THREADS) void fold_kernel(long long n, const int *off,
                                                       const long long *block_sum, const Span *span,
                                                       const int *count, const int *weight,
                                                       long long *sum, int *mx) {
  PSD_LDS long long w_sum[WAVES];
  PSD_LDS int w_max[WAVES];
  const long long nb = (n + THREADS - 1) / THREADS;
  const long long total = block_sum[nb];
  const int lane = lane_id(), wave = wave_id(), tid = (int)threadIdx.x;
  for (long long item = blockIdx.x; item < total; item += gridDim.x) {
    const long long blk = last_at_most(block_sum, nb, item);
    const long long rest = item - block_sum[blk];
    const long long g0 = blk * THREADS;
    const long long in_blk = n - g0 < THREADS ? n - g0 : THREADS;
    const long long g = g0 + last_at_most(off + g0, in_blk, rest);
    const Span sp = span[g];
    const long long lead = sp.run0 & 3;
    const long long u_lo = sp.lo + lead, u_hi = sp.hi + lead;
    const long long tile = u_lo / TILE + (rest - off[g]);
    const long long u = tile * TILE + 4 * tid;
    Quad c, w;
    psd::stats::load_quad(count + sp.run0 - lead, u, u_lo, u_hi, c);
    psd::stats::load_quad(weight + sp.run0 - lead, u, u_lo, u_hi, w);
    long long s = (long long)c.x * w.x + (long long)c.y * w.y + (long long)c.z * w.z +
                  (long long)c.w * w.w;
    int m = c.x > c.y ? c.x : c.y;
    m = c.z > m ? c.z : m;
    m = c.w > m ? c.w : m;
    for (int d = WAVE / 2; d > 0; d >>= 1) {
      const int src = lane + d < WAVE ? lane + d : lane;
      const long long os = (long long)psd::stats::shfl_u64((u64)s, src);
      const int om = shfl_i(m, src);
      if (lane + d < WAVE) {
        s += os;
        m = om > m ? om : m;
      }
    }
    if (lane == 0) {
      w_sum[wave] = s;
      w_max[wave] = m;
    }
    __syncthreads();
    if (tid == 0) {
      for (int k = 1; k < WAVES; k++) {
        s += w_sum[k];
        m = w_max[k] > m ? w_max[k] : m;
      }
      if (s) atomic_add_i64(sum + g, s);
      if (m) atomic_max_i32(mx + g, m);
    }
    __syncthreads(); /* (the next item writes w_sum again) */
  }
}

}  // namespace regions
}  // namespace psd
#endif
