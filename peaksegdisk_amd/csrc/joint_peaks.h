/* joint_peaks.h -- one common peak per window for all members of a group (DESIGN.md section 16;
 * PeakSegPipeline's PeakSegJoint step): for every window [ws, we) the peak [s, e), ws < s < e < we,
 * that maximises  G(s, e) = sum over the feasible members of max(0, gain_i(s, e) - penalty),
 * gain_i the Poisson loss of member i's flat model over the window minus that of its three-segment
 * model (flank, peak, flank; feasible: the peak's mean above both flanks').
 * include/peaksegdisk_hip.h has the definitions; they are the contract.
 *
 * The search goes level by level.  Level 0 cuts the window into n <= 64 bins of b bases (b the
 * smallest power of two that allows it) and tries every pair of bin boundaries; every further level
 * halves b and tries the 9 x 9 positions within four half-bins of the choice so far, until b is 1.
 * All windows of a call advance in lockstep; per level
 *   bins_kernel    a thread per (window, member, slot): the region whose sum the level needs, into
 *                  the flat arrays that region_stats.h's three launches fold.  Level 0: the n bins.
 *                  Later levels, 18 slots: with a_0 .. a_8 the candidate starts and a_9 .. a_17 the
 *                  candidate ends (clamped into the window), [ws, a_0), the eight [a_0, a_k), the
 *                  stretch between a_8 and a_9 (whichever is first), and the eight [a_9, a_k): the
 *                  window is folded once, not once per position.  The last pass, 3 slots: the two
 *                  flanks and the peak.
 *   search_kernel  one workgroup per window.  Each wave takes members wave, wave + WAVES, ... of a
 *                  slab of 64: a lane per bin, a wave-wide inclusive scan of the bins' sums, the
 *                  prefix sums into a 65-word row of LDS.  Then every lane takes candidates tid,
 *                  tid + THREADS, ... and walks the slab's members IN ORDER, adding to the
 *                  candidate's G (kept in LDS between slabs): the order of the additions is part of
 *                  the definition, so the work is spread over candidates, never over members.  After
 *                  the last slab the best (G, s, e) -- largest G, then smallest s, then smallest e,
 *                  an exact comparison that no schedule can change -- is reduced over lanes by
 *                  shuffles and over waves through LDS.
 *   report_kernel  (once) a thread per (window, member): gain, up, sum and bases at the final peak,
 *                  and a 32-bit add to samples_up.
 * sum[] is exact int64 and the feasibility test compares exact 128-bit products: no floating-point
 * atomics, no result that depends on the schedule.
 * LDS of search_kernel: 64 rows x 65 words of int64 (33 280 B; a row's stride of 130 dwords puts
 * successive members two banks apart), 2048 candidates' G (16 384 B), the members' totals and
 * t(T, W) (1 024 B), and the tables of psd_log.
 * Written against psd_platform.h only: the SIMT emulator of tests/emu runs this source. */
#ifndef PSD_JOINT_PEAKS_H
#define PSD_JOINT_PEAKS_H

#include <math.h>

#include "psd_platform.h"
#include "region_stats.h"

namespace psd {
namespace joint {

constexpr int THREADS = psd::regions::THREADS;
constexpr int WAVES = THREADS / WAVE;
constexpr int BINS = 64;        /* bins of level 0, and its slots per (window, member) */
constexpr int SLAB = 64;        /* members whose prefix sums are in LDS at a time */
constexpr int ROW = BINS + 1;   /* words of a member's row */
constexpr int REFINE = 18;      /* slots of a later level */
constexpr int FINAL = 3;        /* slots of the last pass */
constexpr int MAX_CAND = 2048;  /* at least 63 * 62 / 2 = 1953 pairs of level 0 */

typedef unsigned long long u64;

/* the head of a call: what the host reads after setup_kernel */
struct Head {
  u64 check;      /* ~index of the first window with start >= end, or 0 */
  int max_levels; /* levels the widest window needs */
  int pad;
};

/* the windows of a call and what is known of their peaks; one entry per window each */
struct Windows {
  int *group;                 /* its group */
  int *ws, *we;               /* the clipped window */
  int *b;                     /* bin size of the level to run next; 0: nothing more to do */
  int *s, *e;                 /* the choice so far, at last the peak; -1: none */
  int *levels, *samples_up;
  double *objective;
};

/* the groups of a call; groups + 1 entries where an offset */
struct Groups {
  const int *member0;           /* first member */
  const long long *win_off;     /* first window */
  const long long *entry_off;   /* first (window, member) entry */
  const long long *lo, *hi;     /* the intersection of the members' extents (lo > hi: no member) */
  const gint *const *start;     /* the group's windows as given */
  const gint *const *end;
};

/* (window, member) of entry x, and the entry's group */
PSD_D void entry_of(const Groups &g, int n_groups, long long x, long long &w, int &m) {
  const int k = (int)psd::regions::last_at_most(g.entry_off, (long long)n_groups, x);
  const int members = g.member0[k + 1] - g.member0[k];
  const long long r = x - g.entry_off[k];
  w = g.win_off[k] + r / members;
  m = g.member0[k] + (int)(r % members);
}

PSD_D int clamp_into(long long x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : (int)x); }

/* position k of a later level around the choice (s, e): k = 0 .. 8 the starts s + (k - 4) half,
 * k = 9 .. 17 the ends e + (k - 13) half */
PSD_D long long position(int k, int s, int e, int half) {
  return k < 9 ? (long long)s + (long long)(k - 4) * half : (long long)e + (long long)(k - 13) * half;
}

/* a > b for a = x * l, b = y * k: the exact products (sums below 2^63, lengths below 2^32) */
PSD_D bool product_above(long long x, long long l, long long y, long long k) {
  u64 a_hi, b_hi;
  const u64 a_lo = mul_wide_u64((u64)x, (u64)l, a_hi), b_lo = mul_wide_u64((u64)y, (u64)k, b_hi);
  return a_hi > b_hi || (a_hi == b_hi && a_lo > b_lo);
}

/* t(S, L) = S log(S / L), 0 for S = 0 (the logarithm of 1 is an exact 0) */
PSD_D double term(long long sum, long long len) {
  const double s = (double)sum;
  const double q = sum == 0 ? 1.0 : psd_div(s, (double)len);
  return s * psd_log(q);
}

PSD_D bool feasible(long long s1, long long s2, long long s3, long long l1, long long l2, long long l3) {
  return product_above(s2, l1, s1, l2) && product_above(s2, l3, s3, l2);
}

/* gain of a member at a candidate; t_flat = t(T, W) */
PSD_D double gain_of(long long s1, long long s2, long long s3, long long l1, long long l2,
                     long long l3, double t_flat) {
  return ((term(s1, l1) + term(s2, l2)) + term(s3, l3)) - t_flat;
}

/* (g1, s1, e1) before (g0, s0, e0): the larger G, then the smaller s, then the smaller e */
PSD_D bool before(double g1, int s1, int e1, double g0, int s0, int e0) {
  return g1 > g0 || (g1 == g0 && (s1 < s0 || (s1 == s0 && e1 < e0)));
}

/* A thread per window w < n: its clipped extent, its first bin size, and empty results.
 * expand: the windows as given are clusters [cs, ce) and the window is [cs - (ce - cs), ce + (ce - cs));
 * otherwise a window with start >= end goes to head->check.  head holds zeros. */
__global__ __launch_bounds__(THREADS) void setup_kernel(Groups g, int n_groups, long long n, int expand,
                                                        Windows win, Head *head) {
  const long long w = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (w >= n) return;
  const int k = (int)psd::regions::last_at_most(g.win_off, (long long)n_groups, w);
  const long long i = w - g.win_off[k];
  long long rs = g.start[k][i], re = g.end[k][i];
  if (expand) {
    const long long width = re - rs;
    rs -= width;
    re += width;
  } else if (rs >= re) {
    atomic_max_u64(&head->check, ~(u64)w);
  }
  const long long lo = g.lo[k], hi = g.hi[k];
  long long a = rs > lo ? rs : lo, z = re < hi ? re : hi;
  if (lo > hi) a = z = 0;
  if (z < a) z = a;
  const long long width = z - a;
  int b = 0;
  if (width >= 3) {
    int levels = 1;
    b = 1;
    while ((width + b - 1) / b > BINS) {
      b <<= 1;
      levels++;
    }
    atomic_max_i32(&head->max_levels, levels);
  }
  win.group[w] = k;
  win.ws[w] = (int)a;
  win.we[w] = (int)z;
  win.b[w] = b;
  win.s[w] = win.e[w] = -1;
  win.levels[w] = win.samples_up[w] = 0;
  win.objective[w] = 0.0;
}

/* A thread per (entry, slot): slots = BINS (level 0), REFINE (a later level) or FINAL (the last
 * pass).  member_contig[m]: the contig of member m. */
__global__ __launch_bounds__(THREADS) void bins_kernel(Groups g, int n_groups, long long n_entries,
                                                       int slots, Windows win, const int *member_contig,
                                                       int *region_start, int *region_end,
                                                       int *region_contig) {
  const long long x = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (x >= n_entries * slots) return;
  const long long entry = x / slots;
  const int slot = (int)(x % slots);
  long long w;
  int m;
  entry_of(g, n_groups, entry, w, m);
  const int ws = win.ws[w], we = win.we[w], b = win.b[w], s = win.s[w], e = win.e[w];
  int rs = 0, re = 0; /* (an empty region: no bases, sum 0) */
  if (slots == BINS) {
    const long long from = (long long)ws + (long long)slot * b;
    if (b > 0 && from < we) {
      rs = (int)from;
      re = clamp_into(from + b, ws, we);
    }
  } else if (slots == REFINE) {
    if (b > 0) {
      const int a0 = clamp_into(position(0, s, e, b), ws, we);
      const int a8 = clamp_into(position(8, s, e, b), ws, we);
      const int a9 = clamp_into(position(9, s, e, b), ws, we);
      const int ak = clamp_into(position(slot, s, e, b), ws, we);
      if (slot == 0) {
        rs = ws;
        re = a0;
      } else if (slot < 9) {
        rs = a0;
        re = ak;
      } else if (slot == 9) {
        rs = a8 < a9 ? a8 : a9;
        re = a8 < a9 ? a9 : a8;
      } else {
        rs = a9;
        re = ak;
      }
    }
  } else if (s >= 0) {
    rs = slot == 0 ? ws : (slot == 1 ? s : e);
    re = slot == 0 ? s : (slot == 1 ? e : we);
  }
  region_start[x] = rs;
  region_end[x] = re;
  region_contig[x] = member_contig[m];
}

/* One workgroup per window, all of one level: level0 != 0 the first, otherwise a later one (the
 * header has the scheme).  sum[]: the fold of the slots bins_kernel wrote for this level.
 * total[]: per entry, the member's sum over the window (written at level 0). */
__global__ __launch_bounds__(THREADS) void search_kernel(Groups g, int level0, Windows win,
                                                         double penalty, const long long *sum,
                                                         long long *total) {
  PSD_LDS long long prefix[SLAB * ROW];
  PSD_LDS double g_acc[MAX_CAND];
  PSD_LDS long long m_total[SLAB];
  PSD_LDS double m_flat[SLAB];
  PSD_LDS double w_g[WAVES];
  PSD_LDS int w_s[WAVES], w_e[WAVES];
  psd_tables_init(); /* exp/log tables -> LDS */
  const long long w = blockIdx.x;
  const int tid = (int)threadIdx.x, lane = lane_id(), wave = wave_id();
  const int b = win.b[w];
  if (b == 0) return; /* (the whole workgroup) */
  const int k = win.group[w];
  const int ws = win.ws[w], we = win.we[w], s0 = win.s[w], e0 = win.e[w];
  const long long width = (long long)we - ws;
  const int n = level0 ? (int)((width + b - 1) / b) : 0;
  const int member0 = g.member0[k], members = g.member0[k + 1] - member0;
  const long long entry0 = g.entry_off[k] + (w - g.win_off[k]) * members;
  const int slots = level0 ? BINS : REFINE;
  const int n_cand = level0 ? (n - 1) * (n - 2) / 2 : 81;
  for (int base = 0; base < members; base += SLAB) {
    const int in_slab = members - base < SLAB ? members - base : SLAB;
    /* the slab's rows: the sums below every position a candidate can take */
    for (int r = wave; r < in_slab; r += WAVES) {
      const long long entry = entry0 + base + r;
      const long long *from = sum + entry * slots;
      long long *row = prefix + r * ROW;
      long long all;
      if (level0) {
        long long inc = lane < n ? from[lane] : 0;
        for (int d = 1; d < WAVE; d <<= 1) {
          const long long o = (long long)psd::stats::shfl_u64((u64)inc, lane >= d ? lane - d : lane);
          if (lane >= d) inc += o;
        }
        row[lane + 1] = inc;
        if (lane == 0) row[0] = 0;
        all = (long long)psd::stats::shfl_u64((u64)inc, WAVE - 1);
        if (lane == 0) total[entry] = all;
      } else {
        if (lane < REFINE) {
          const int a8 = clamp_into(position(8, s0, e0, b), ws, we);
          const int a9 = clamp_into(position(9, s0, e0, b), ws, we);
          long long v = from[0];
          if (lane >= 9) v += from[8] + (a8 < a9 ? from[9] : -from[9]);
          if (lane != 0 && lane != 9) v += from[lane];
          row[lane] = v;
        }
        all = total[entry];
      }
      if (lane == 0) {
        m_total[r] = all;
        m_flat[r] = term(all, width);
      }
    }
    __syncthreads();
    for (int c = tid; c < n_cand; c += THREADS) {
      int i, j;
      long long s, e;
      if (level0) {
        /* pair c of 1 <= i < j <= n - 1, in increasing j, then i */
        int q = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)c)) * 0.5f);
        while (q * (q - 1) / 2 > c) q--;
        while (q * (q + 1) / 2 <= c) q++;
        j = q + 1;
        i = c - q * (q - 1) / 2 + 1;
        s = (long long)ws + (long long)i * b;
        e = (long long)ws + (long long)j * b;
      } else {
        i = c / 9;
        j = 9 + c % 9;
        s = position(i, s0, e0, b);
        e = position(j, s0, e0, b);
      }
      double acc = base == 0 ? 0.0 : g_acc[c];
      if (ws < s && s < e && e < we) {
        const long long l1 = s - ws, l2 = e - s, l3 = we - e;
        for (int r = 0; r < in_slab; r++) {
          const long long *row = prefix + r * ROW;
          const long long p_s = row[i], p_e = row[j];
          const long long s1 = p_s, s2 = p_e - p_s, s3 = m_total[r] - p_e;
          const double gain = gain_of(s1, s2, s3, l1, l2, l3, m_flat[r]);
          const double more = gain - penalty;
          acc += feasible(s1, s2, s3, l1, l2, l3) && more > 0.0 ? more : 0.0;
        }
      } else {
        acc = -1.0; /* no candidate */
      }
      g_acc[c] = acc;
    }
    __syncthreads(); /* (the next slab writes the rows again) */
  }
  /* the best candidate of this lane, of its wave, of the workgroup */
  double best_g = -1.0;
  int best_s = 0, best_e = 0;
  for (int c = tid; c < n_cand; c += THREADS) {
    int cs, ce;
    if (level0) {
      int q = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)c)) * 0.5f);
      while (q * (q - 1) / 2 > c) q--;
      while (q * (q + 1) / 2 <= c) q++;
      cs = (int)((long long)ws + (long long)(c - q * (q - 1) / 2 + 1) * b);
      ce = (int)((long long)ws + (long long)(q + 1) * b);
    } else {
      cs = clamp_into(position(c / 9, s0, e0, b), ws, we);
      ce = clamp_into(position(9 + c % 9, s0, e0, b), ws, we);
    }
    const double v = g_acc[c];
    if (v >= 0.0 && (best_g < 0.0 || before(v, cs, ce, best_g, best_s, best_e))) {
      best_g = v;
      best_s = cs;
      best_e = ce;
    }
  }
  for (int d = WAVE / 2; d > 0; d >>= 1) {
    const int src = lane + d < WAVE ? lane + d : lane;
    const double og = shfl_d(best_g, src);
    const int os = shfl_i(best_s, src), oe = shfl_i(best_e, src);
    if (og >= 0.0 && (best_g < 0.0 || before(og, os, oe, best_g, best_s, best_e))) {
      best_g = og;
      best_s = os;
      best_e = oe;
    }
  }
  if (lane == 0) {
    w_g[wave] = best_g;
    w_s[wave] = best_s;
    w_e[wave] = best_e;
  }
  __syncthreads();
  if (tid == 0) {
    for (int v = 1; v < WAVES; v++)
      if (w_g[v] >= 0.0 && (best_g < 0.0 || before(w_g[v], w_s[v], w_e[v], best_g, best_s, best_e))) {
        best_g = w_g[v];
        best_s = w_s[v];
        best_e = w_e[v];
      }
    if (level0 && !(best_g > 0.0)) {
      win.b[w] = 0; /* no joint peak */
    } else {
      win.s[w] = best_s;
      win.e[w] = best_e;
      win.objective[w] = best_g;
      win.levels[w] += 1;
      win.b[w] = b >> 1; /* (0 after the level of single bases) */
    }
  }
}

/* A thread per entry: the member at the window's peak.  sum[]: the fold of the FINAL slots. */
__global__ __launch_bounds__(THREADS) void report_kernel(Groups g, int n_groups, long long n_entries,
                                                         Windows win, double penalty,
                                                         const long long *sum, double *m_gain,
                                                         int *m_up, long long *m_sum, int *m_bases) {
  psd_tables_init();
  const long long x = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (x >= n_entries) return;
  long long w;
  int m;
  entry_of(g, n_groups, x, w, m);
  const int s = win.s[w], e = win.e[w];
  double gain = 0.0;
  long long s2 = 0;
  int up = 0, bases = 0;
  if (s >= 0) {
    const int ws = win.ws[w], we = win.we[w];
    const long long s1 = sum[x * FINAL], s3 = sum[x * FINAL + 2];
    const long long l1 = (long long)s - ws, l2 = (long long)e - s, l3 = (long long)we - e;
    s2 = sum[x * FINAL + 1];
    bases = (int)l2;
    const double v = gain_of(s1, s2, s3, l1, l2, l3, term(s1 + s2 + s3, (long long)we - ws));
    if (feasible(s1, s2, s3, l1, l2, l3)) {
      gain = v;
      up = v - penalty > 0.0;
    }
  }
  m_gain[x] = gain;
  m_up[x] = up;
  m_sum[x] = s2;
  m_bases[x] = bases;
  if (up) atomic_add_i32(win.samples_up + w, 1);
}

}  // namespace joint
}  // namespace psd
#endif
