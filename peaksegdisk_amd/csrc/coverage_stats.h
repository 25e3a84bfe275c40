/* coverage_stats.h -- order statistics and moments of every contig's per-base coverage, from the
 * runs resident in HBM.  A contig's runs (count_i, weight_i) stand for the vector x that repeats
 * count_i weight_i times; B = sum of the weights < 2^31 is its number of bases.
 *
 *   order statistic  x_(r), 0 <= r < B: the smallest v with  sum over count_i <= v of weight_i  > r
 *   moments          bases, runs, S1 = sum w c, and S2 = sum w c^2 as three words: with
 *                    c = ch 2^16 + cl,  Q0 = sum w cl^2, Q1 = sum w cl ch, Q2 = sum w ch^2, each
 *                    below 2^63 because sum w < 2^31;  S2 = Q0 + 2^17 Q1 + 2^32 Q2
 *
 * The selection is a radix select, most significant digit first, over 8-bit digits.  Every rank of
 * a contig carries the digits fixed so far (`prefix`) and what is left of its rank among the runs
 * that share them (`resid`); ranks with equal prefixes share one histogram, that of the first of
 * them (its `leader`).  The launches of a call, however many contigs the set has, and no workgroup
 * waits for another:
 *   moments_kernel  a workgroup per tile of TILE runs of a contig: lane sums, a butterfly of
 *                   shuffles per wave, the waves meet in LDS, one 64-bit integer atomic per word.
 *   per digit pass:
 *   hist_kernel     the same tiles: the weighted 256-bin histogram of the digit at hand for each
 *                   distinct prefix of the contig, built in LDS (ds_add_u32: a workgroup's weights
 *                   sum to less than 2^31); the non-zero bins go to HBM by 64-bit integer atomics
 *                   on zeroed words.
 *   pick_kernel     a wave per contig: for every rank a scan of its leader's 256 bins (four per
 *                   lane) finds the digit whose cumulative weight first exceeds resid, and what
 *                   lies below the digit leaves resid; then the new leaders.
 * The host knows every contig's largest count from the encoder, so the passes over digits that are
 * zero in the whole set are not launched: counts below 256 take one pass, full-range counts four.
 * Integer atomics commute: the results do not depend on the schedule.
 *
 * Algorithmic traffic: moments_kernel and every hist_kernel read the 8 R bytes of count and weight
 * of a contig of R runs once; a pass zeroes 2 KB per contig and rank that may lead (the first
 * pass of a call: one), adds its non-zero bins, and pick_kernel reads 2 KB per distinct prefix.
 *
 * The tiles are segment_stats.h's: laid over the 16-byte aligned range that holds the contig, so
 * that every lane loads 16 aligned bytes of count[] and of weight[] (stats::load_quad).  Written
 * against psd_platform.h only: the SIMT emulator of tests/emu runs this source. */
#ifndef PSD_COVERAGE_STATS_H
#define PSD_COVERAGE_STATS_H

#include "psd_platform.h"
#include "segment_stats.h"

namespace psd {
namespace cover {

constexpr int THREADS = psd::stats::THREADS;
constexpr int WAVES = THREADS / WAVE;
constexpr int TILE = psd::stats::TILE;
constexpr int MAX_RANKS = 16; /* ranks per contig and call: a histogram each in LDS (16 KB) */
constexpr int BINS = 256;
constexpr int DESC = 4;       /* long longs per contig in the descriptor array */
constexpr int MOMENTS = 6;    /* words per contig */

typedef unsigned long long u64;
typedef psd::stats::Quad Quad;

/* per contig, desc[DESC c + ...] */
enum {
  D_RUN0 = 0,  /* first run of the contig in count / weight */
  D_RUNS = 1,  /* its runs */
  D_TILE0 = 2, /* index of its first tile in the grid */
};

/* per contig, moments[MOMENTS c + ...] */
enum { M_BASES = 0, M_RUNS = 1, M_S1 = 2, M_Q0 = 3, M_Q1 = 4, M_Q2 = 5 };

struct Sums {
  u64 bases, s1, q0, q1, q2;
};

PSD_D void fold_run(Sums &s, int count, int weight) {
  const u64 w = (u64)(unsigned)weight, c = (u64)(unsigned)count;
  const u64 cl = c & 0xffffull, ch = c >> 16;
  s.bases += w;
  s.s1 += w * c;
  s.q0 += w * cl * cl;
  s.q1 += w * cl * ch;
  s.q2 += w * ch * ch;
}

/* the sum over the wave, in every lane */
PSD_D u64 wave_sum(u64 v, int lane) {
  for (int off = 1; off < WAVE; off <<= 1) v += psd::stats::shfl_u64(v, lane ^ off);
  return v;
}

/* the tile of the workgroup: its contig's descriptor and the four entries of the lane (entries
 * outside the contig read as count 0, weight 0); -> how many of the four are runs of the contig */
PSD_D int load_tile(const long long *desc, const int *tile_contig, const int *count, const int *weight,
                    int &contig, Quad &c, Quad &w) {
  contig = tile_contig[blockIdx.x];
  const long long *d = desc + (long long)DESC * contig;
  const long long run0 = d[D_RUN0], n_runs = d[D_RUNS];
  const long long lead = run0 & 3;
  const long long u = ((long long)blockIdx.x - d[D_TILE0]) * TILE + 4 * (long long)threadIdx.x;
  psd::stats::load_quad(count + run0 - lead, u, lead, lead + n_runs, c);
  psd::stats::load_quad(weight + run0 - lead, u, lead, lead + n_runs, w);
  const long long lo = u > lead ? u : lead;
  const long long hi = u + 4 < lead + n_runs ? u + 4 : lead + n_runs;
  return hi > lo ? (int)(hi - lo) : 0;
}

__global__ __launch_bounds__(THREADS) void moments_kernel(const long long *desc, const int *tile_contig,
                                                          const int *count, const int *weight,
                                                          u64 *moments) {
  const int lane = lane_id(), wave = wave_id(), tid = (int)threadIdx.x;
  int contig;
  Quad c, w;
  const int n_valid = load_tile(desc, tile_contig, count, weight, contig, c, w);
  Sums s;
  s.bases = s.s1 = s.q0 = s.q1 = s.q2 = 0;
  fold_run(s, c.x, w.x);
  fold_run(s, c.y, w.y);
  fold_run(s, c.z, w.z);
  fold_run(s, c.w, w.w);
  PSD_LDS u64 w_part[WAVES * MOMENTS];
  const u64 bases = wave_sum(s.bases, lane), runs = wave_sum((u64)n_valid, lane);
  const u64 s1 = wave_sum(s.s1, lane), q0 = wave_sum(s.q0, lane), q1 = wave_sum(s.q1, lane),
            q2 = wave_sum(s.q2, lane);
  if (lane == 0) {
    u64 *p = w_part + wave * MOMENTS;
    p[M_BASES] = bases;
    p[M_RUNS] = runs;
    p[M_S1] = s1;
    p[M_Q0] = q0;
    p[M_Q1] = q1;
    p[M_Q2] = q2;
  }
  __syncthreads();
  if (tid < MOMENTS) { /* one atomic per word and workgroup */
    u64 v = 0;
    for (int k = 0; k < WAVES; k++) v += w_part[k * MOMENTS + tid];
    if (v) atomic_add_i64((long long *)(moments + (long long)MOMENTS * contig + tid), (long long)v);
  }
}

/* one run into the histograms of the workgroup's groups */
PSD_D void bin_run(unsigned *l_hist, const unsigned *l_prefix, int n_groups, int shift, int count,
                   int weight) {
  if (weight <= 0) return; /* (no run) */
  const u64 c = (u64)(unsigned)count;
  const u64 high = c >> (shift + 8);
  const int digit = (int)((c >> shift) & 255ull);
  for (int g = 0; g < n_groups; g++)
    if (((u64)l_prefix[g] >> (shift + 8)) == high) lds_add_u32(l_hist + g * BINS + digit, (unsigned)weight);
}

/* the histogram of rank k of contig c: a plane of n_contigs x BINS words per rank, so that the
 * first pass of a call, where every rank's leader is rank 0, zeroes and reads one plane only */
PSD_D long long hist_row(int rank, int contig, int n_contigs) {
  return ((long long)rank * n_contigs + contig) * BINS;
}

/* prefix, leader: n_ranks per contig; hist: zeroed (the planes of the ranks that may lead), of
 * which the leaders' rows are filled */
__global__ __launch_bounds__(THREADS) void hist_kernel(const long long *desc, const int *tile_contig,
                                                       const int *count, const int *weight,
                                                       int n_contigs, int n_ranks, int shift,
                                                       const int *prefix, const int *leader, u64 *hist) {
  const int lane = lane_id(), wave = wave_id(), tid = (int)threadIdx.x;
  PSD_LDS unsigned l_hist[MAX_RANKS * BINS];
  PSD_LDS unsigned l_prefix[MAX_RANKS];
  PSD_LDS int l_rank[MAX_RANKS];
  PSD_LDS int l_groups;
  int contig;
  Quad c, w;
  (void)load_tile(desc, tile_contig, count, weight, contig, c, w);
  const long long state = (long long)contig * n_ranks;
  if (wave == 0) { /* the contig's distinct prefixes, in the order of their first ranks */
    const bool leads = lane < n_ranks && leader[state + lane] == lane;
    const unsigned long long m = ballot(leads);
    if (leads) {
      const int g = popc64(m & lanes_below(lane));
      l_prefix[g] = (unsigned)prefix[state + lane];
      l_rank[g] = lane;
    }
    if (lane == 0) l_groups = popc64(m);
  }
  __syncthreads();
  const int n_groups = l_groups;
  for (int j = tid; j < n_groups * BINS; j += THREADS) l_hist[j] = 0;
  __syncthreads();
  bin_run(l_hist, l_prefix, n_groups, shift, c.x, w.x);
  bin_run(l_hist, l_prefix, n_groups, shift, c.y, w.y);
  bin_run(l_hist, l_prefix, n_groups, shift, c.z, w.z);
  bin_run(l_hist, l_prefix, n_groups, shift, c.w, w.w);
  __syncthreads();
  for (int j = tid; j < n_groups * BINS; j += THREADS) {
    const unsigned v = l_hist[j];
    if (v)
      atomic_add_i64((long long *)(hist + hist_row(l_rank[j / BINS], contig, n_contigs) + (j % BINS)),
                     (long long)v);
  }
}

/* A workgroup of one wave per contig.  value[]: the digits fixed so far, the order statistic
 * after the pass of shift 0. */
__global__ __launch_bounds__(WAVE) void pick_kernel(int n_ranks, int shift, const u64 *hist, int *prefix,
                                                    long long *resid, int *leader, int *value) {
  const int lane = lane_id(), contig = (int)blockIdx.x, n_contigs = (int)gridDim.x;
  const long long state = (long long)contig * n_ranks;
  int my_prefix = 0;
  long long my_resid = 0;
  for (int k = 0; k < n_ranks; k++) {
    const u64 r = (u64)resid[state + k];
    const u64 *h = hist + hist_row(leader[state + k], contig, n_contigs) + 4 * lane;
    const u64 b0 = h[0], b1 = h[1], b2 = h[2], b3 = h[3];
    const u64 mine = b0 + b1 + b2 + b3;
    u64 incl = mine;
    for (int off = 1; off < WAVE; off <<= 1) {
      const u64 o = psd::stats::shfl_u64(incl, lane >= off ? lane - off : lane);
      if (lane >= off) incl += o;
    }
    /* the first lane whose bins reach beyond r holds the digit (a rank below the contig's bases
     * always finds one) */
    const unsigned long long reach = ballot(incl > r);
    const int src = reach ? ctz64(reach) : WAVE - 1;
    u64 below = incl - mine;
    int digit = 4 * lane;
    if (below + b0 <= r) {
      below += b0;
      digit += 1;
      if (below + b1 <= r) {
        below += b1;
        digit += 1;
        if (below + b2 <= r) {
          below += b2;
          digit += 1;
        }
      }
    }
    digit = shfl_i(digit, src);
    below = psd::stats::shfl_u64(below, src);
    if (lane == k) {
      my_prefix = (int)((unsigned)prefix[state + k] | ((unsigned)digit << shift));
      my_resid = (long long)(r - below);
    }
  }
  int my_leader = lane;
  for (int j = n_ranks - 1; j >= 0; j--) {
    const int other = shfl_i(my_prefix, j);
    if (j <= lane && other == my_prefix) my_leader = j;
  }
  if (lane < n_ranks) {
    prefix[state + lane] = my_prefix;
    resid[state + lane] = my_resid;
    leader[state + lane] = my_leader;
    value[state + lane] = my_prefix;
  }
}

}  // namespace cover
}  // namespace psd
#endif
