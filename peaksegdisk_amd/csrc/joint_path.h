/* joint_path.h -- the joint peaks of joint_peaks.h at P penalties in one call (DESIGN.md section
 * 17): model (p, w) is what joint_peaks.h's kernels give for window w at penalty p, bit for bit;
 * what does not depend on the penalty is computed once per window.
 *
 * The state of a window -- b, s, e, levels, samples_up, objective, and ws, we, group repeated -- is
 * kept per (penalty, window) at p * n_windows + w: psd::joint::Windows over P times as many rows.
 * Level 0 needs the rows of p = 0 only (all penalties share its bins), so joint_peaks.h's
 * bins_kernel makes its regions.  Per level
 *   bins_kernel    a thread per (penalty, entry, slot) of a later level (18 slots) or the last pass
 *                  (3 slots): the regions of joint_peaks.h's bins_kernel around this penalty's
 *                  choice; a penalty without a peak gets empty regions.
 *   search0_kernel level 0, one workgroup per window: the members' prefix sums into LDS slab by
 *                  slab exactly as joint_peaks.h's search_kernel has them.  A lane takes candidates
 *                  tid, tid + THREADS, ...; for each it walks the slab's members IN ORDER, computes
 *                  the feasibility test and the gain ONCE and adds max(0, gain - penalty_p) to PT
 *                  accumulators in registers (PT: the number of penalties rounded up to a power of
 *                  two, a template parameter, the loops over it unrolled; the penalties past the
 *                  last are +Inf and add an exact 0).  Groups of more than 64 members: between
 *                  slabs the accumulators wait in a table in HBM, [window][penalty][candidate]
 *                  (in LDS they would need 16 x 16 KiB).  After the last slab the lane keeps the
 *                  best (G, s, e) of every penalty in registers -- the three-key order is total on
 *                  the candidates of a window, so any order of comparison gives the same winner --
 *                  and they are reduced over lanes by shuffles and over waves through LDS.
 *   refine_kernel  a later level, one workgroup per window: the P x 81 (penalty, candidate) pairs
 *                  of the penalties that still have a bin size are spread over the lanes; the
 *                  rows of 18 prefix sums, one per (penalty, member), go through LDS in slabs of
 *                  as many members as fit (4160 / (18 PT) words), G waits in LDS between slabs.  A
 *                  penalty whose window has no peak or is finished idles; a window whose penalties
 *                  all idle returns at once.
 *   report_kernel  (once) a thread per (penalty, entry): joint_peaks.h's report_kernel.
 * term, feasible, gain_of, before, position, entry_of and clamp_into are joint_peaks.h's: the
 * arithmetic exists once.  Nothing here adds floating-point numbers in an order that a schedule
 * could change.
 * Every kernel here is a template, also those that need no parameter (`template <int = 0>`): the
 * compiler emits a template's instances behind the translation unit's ordinary functions, so these
 * kernels lie behind the forward kernels' out-of-line callees in the code object and leave the
 * distance between the forward kernels and those callees as it was.
 * Written against psd_platform.h only: the SIMT emulator of tests/emu runs this source. */
#ifndef PSD_JOINT_PATH_H
#define PSD_JOINT_PATH_H

#include "joint_peaks.h"

namespace psd {
namespace joint_path {

using psd::joint::BINS;
using psd::joint::FINAL;
using psd::joint::Groups;
using psd::joint::MAX_CAND;
using psd::joint::REFINE;
using psd::joint::ROW;
using psd::joint::SLAB;
using psd::joint::THREADS;
using psd::joint::WAVES;
using psd::joint::Windows;
using psd::joint::before;
using psd::joint::clamp_into;
using psd::joint::entry_of;
using psd::joint::feasible;
using psd::joint::gain_of;
using psd::joint::position;
using psd::joint::term;
typedef psd::joint::u64 u64;

constexpr int MAX_PENALTIES = 16;
constexpr int PAIRS = 81;                 /* candidates of a later level */
constexpr int ROW_WORDS = SLAB * ROW;     /* words of prefix sums in LDS */

#if defined(PSD_EMU)
#define PSD_PATH_UNROLL
#else
#define PSD_PATH_UNROLL _Pragma("unroll")
#endif

/* the penalties of a call, by value: v[p] for p past the last is +Inf */
struct Penalties {
  double v[MAX_PENALTIES];
};

/* A thread per (penalty, window): joint_peaks.h's setup_kernel, the window's rows repeated for
 * every penalty.  n: windows; rows at p * n + w.  head holds zeros. */
template <int = 0>
__global__ __launch_bounds__(THREADS) void setup_kernel(Groups g, int n_groups, long long n, int n_pen,
                                                        int expand, Windows win,
                                                        psd::joint::Head *head) {
  const long long x = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (x >= n * n_pen) return;
  const long long w = x % n;
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
  win.group[x] = k;
  win.ws[x] = (int)a;
  win.we[x] = (int)z;
  win.b[x] = b;
  win.s[x] = win.e[x] = -1;
  win.levels[x] = win.samples_up[x] = 0;
  win.objective[x] = 0.0;
}

/* A thread per (penalty, entry, slot), slots = REFINE or FINAL: the regions of joint_peaks.h's
 * bins_kernel for the state of (penalty, window), at (p * n_entries + entry) * slots + slot. */
template <int = 0>
__global__ __launch_bounds__(THREADS) void bins_kernel(Groups g, int n_groups, long long n_windows,
                                                       long long n_entries, int n_pen, int slots,
                                                       Windows win, const int *member_contig,
                                                       int *region_start, int *region_end,
                                                       int *region_contig) {
  const long long x = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (x >= n_entries * slots * n_pen) return;
  const long long pe = x / slots;
  const int slot = (int)(x % slots);
  long long w;
  int m;
  entry_of(g, n_groups, pe % n_entries, w, m);
  const long long pw = (pe / n_entries) * n_windows + w;
  const int ws = win.ws[pw], we = win.we[pw], b = win.b[pw], s = win.s[pw], e = win.e[pw];
  int rs = 0, re = 0; /* (an empty region: no bases, sum 0) */
  if (slots == REFINE) {
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

/* pair c of 1 <= i < j <= n - 1, in increasing j, then i (joint_peaks.h's order) */
PSD_D void pair_of(int c, int &i, int &j) {
  int q = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)c)) * 0.5f);
  while (q * (q - 1) / 2 > c) q--;
  while (q * (q + 1) / 2 <= c) q++;
  j = q + 1;
  i = c - q * (q - 1) / 2 + 1;
}

/* Level 0, one workgroup per window w < n_windows.  sum[]: the fold of the BINS slots of every
 * entry; total[]: per entry, the member's sum over the window (written here); carry[]: PT x
 * MAX_CAND doubles per window (touched by groups of more than SLAB members only). */
template <int PT>
__global__ __launch_bounds__(THREADS) void search0_kernel(Groups g, long long n_windows, int n_pen,
                                                          Penalties pen, Windows win,
                                                          const long long *sum, long long *total,
                                                          double *carry) {
  PSD_LDS long long prefix[ROW_WORDS];
  PSD_LDS long long m_total[SLAB];
  PSD_LDS double m_flat[SLAB];
  PSD_LDS double w_g[WAVES * MAX_PENALTIES];
  PSD_LDS int w_s[WAVES * MAX_PENALTIES], w_e[WAVES * MAX_PENALTIES];
  psd_tables_init(); /* exp/log tables -> LDS */
  const long long w = blockIdx.x;
  const int tid = (int)threadIdx.x, lane = lane_id(), wave = wave_id();
  const int b = win.b[w]; /* (the same for every penalty before level 0) */
  if (b == 0) return;     /* (the whole workgroup) */
  const int k = win.group[w];
  const int ws = win.ws[w], we = win.we[w];
  const long long width = (long long)we - ws;
  const int n = (int)((width + b - 1) / b);
  const int member0 = g.member0[k], members = g.member0[k + 1] - member0;
  const long long entry0 = g.entry_off[k] + (w - g.win_off[k]) * members;
  const int n_cand = (n - 1) * (n - 2) / 2;
  double *held = carry + w * (long long)(PT * MAX_CAND);
  double best_g[PT];
  int best_s[PT], best_e[PT];
  PSD_PATH_UNROLL
  for (int p = 0; p < PT; p++) {
    best_g[p] = -1.0;
    best_s[p] = best_e[p] = 0;
  }
  for (int base = 0; base < members; base += SLAB) {
    const int in_slab = members - base < SLAB ? members - base : SLAB;
    const bool last = base + SLAB >= members;
    for (int r = wave; r < in_slab; r += WAVES) {
      const long long entry = entry0 + base + r;
      const long long *from = sum + entry * BINS;
      long long *row = prefix + r * ROW;
      long long inc = lane < n ? from[lane] : 0;
      for (int d = 1; d < WAVE; d <<= 1) {
        const long long o = (long long)psd::stats::shfl_u64((u64)inc, lane >= d ? lane - d : lane);
        if (lane >= d) inc += o;
      }
      row[lane + 1] = inc;
      if (lane == 0) row[0] = 0;
      const long long all = (long long)psd::stats::shfl_u64((u64)inc, WAVE - 1);
      if (lane == 0) {
        total[entry] = all;
        m_total[r] = all;
        m_flat[r] = term(all, width);
      }
    }
    __syncthreads();
    for (int c = tid; c < n_cand; c += THREADS) {
      int i, j;
      pair_of(c, i, j);
      const long long s = (long long)ws + (long long)i * b, e = (long long)ws + (long long)j * b;
      const bool is_candidate = ws < s && s < e && e < we;
      double acc[PT];
      PSD_PATH_UNROLL
      for (int p = 0; p < PT; p++) acc[p] = base == 0 ? 0.0 : held[p * MAX_CAND + c];
      if (is_candidate) {
        const long long l1 = s - ws, l2 = e - s, l3 = we - e;
        for (int r = 0; r < in_slab; r++) {
          const long long *row = prefix + r * ROW;
          const long long p_s = row[i], p_e = row[j];
          const long long s1 = p_s, s2 = p_e - p_s, s3 = m_total[r] - p_e;
          const double gain = gain_of(s1, s2, s3, l1, l2, l3, m_flat[r]);
          const bool ok = feasible(s1, s2, s3, l1, l2, l3);
          PSD_PATH_UNROLL
          for (int p = 0; p < PT; p++) {
            const double more = gain - pen.v[p];
            acc[p] += ok && more > 0.0 ? more : 0.0;
          }
        }
      }
      if (!last) {
        PSD_PATH_UNROLL
        for (int p = 0; p < PT; p++) held[p * MAX_CAND + c] = acc[p];
      } else if (is_candidate) {
        PSD_PATH_UNROLL
        for (int p = 0; p < PT; p++)
          if (best_g[p] < 0.0 || before(acc[p], (int)s, (int)e, best_g[p], best_s[p], best_e[p])) {
            best_g[p] = acc[p];
            best_s[p] = (int)s;
            best_e[p] = (int)e;
          }
      }
    }
    __syncthreads(); /* (the next slab writes the rows again) */
  }
  /* every penalty's best candidate: of this lane, of its wave, of the workgroup */
  PSD_PATH_UNROLL
  for (int p = 0; p < PT; p++) {
    double bg = best_g[p];
    int bs = best_s[p], be = best_e[p];
    for (int d = WAVE / 2; d > 0; d >>= 1) {
      const int src = lane + d < WAVE ? lane + d : lane;
      const double og = shfl_d(bg, src);
      const int os = shfl_i(bs, src), oe = shfl_i(be, src);
      if (og >= 0.0 && (bg < 0.0 || before(og, os, oe, bg, bs, be))) {
        bg = og;
        bs = os;
        be = oe;
      }
    }
    if (lane == 0) {
      w_g[wave * MAX_PENALTIES + p] = bg;
      w_s[wave * MAX_PENALTIES + p] = bs;
      w_e[wave * MAX_PENALTIES + p] = be;
    }
  }
  __syncthreads();
  if (tid < n_pen) {
    double bg = w_g[tid];
    int bs = w_s[tid], be = w_e[tid];
    for (int v = 1; v < WAVES; v++) {
      const int at = v * MAX_PENALTIES + tid;
      if (w_g[at] >= 0.0 && (bg < 0.0 || before(w_g[at], w_s[at], w_e[at], bg, bs, be))) {
        bg = w_g[at];
        bs = w_s[at];
        be = w_e[at];
      }
    }
    const long long pw = (long long)tid * n_windows + w;
    if (!(bg > 0.0)) {
      win.b[pw] = 0; /* no joint peak at this penalty */
    } else {
      win.s[pw] = bs;
      win.e[pw] = be;
      win.objective[pw] = bg;
      win.levels[pw] += 1;
      win.b[pw] = b >> 1; /* (0 after the level of single bases) */
    }
  }
}

/* A later level, one workgroup per window.  sum[]: the fold of the REFINE slots of every (penalty,
 * entry); total[]: per entry, from level 0. */
template <int PT>
__global__ __launch_bounds__(THREADS) void refine_kernel(Groups g, long long n_windows,
                                                         long long n_entries, int n_pen, Penalties pen,
                                                         Windows win, const long long *sum,
                                                         const long long *total) {
  constexpr int MEMBERS = ROW_WORDS / (REFINE * PT) < SLAB ? ROW_WORDS / (REFINE * PT) : SLAB;
  PSD_LDS long long prefix[ROW_WORDS];
  PSD_LDS double g_acc[MAX_PENALTIES * PAIRS];
  PSD_LDS long long m_total[SLAB];
  PSD_LDS double m_flat[SLAB];
  PSD_LDS int p_b[MAX_PENALTIES], p_s[MAX_PENALTIES], p_e[MAX_PENALTIES];
  psd_tables_init();
  const long long w = blockIdx.x;
  const int tid = (int)threadIdx.x;
  if (tid < MAX_PENALTIES) {
    const long long pw = (long long)tid * n_windows + w;
    p_b[tid] = tid < n_pen ? win.b[pw] : 0;
    p_s[tid] = tid < n_pen ? win.s[pw] : -1;
    p_e[tid] = tid < n_pen ? win.e[pw] : -1;
  }
  __syncthreads();
  int busy = 0;
  for (int p = 0; p < n_pen; p++) busy |= p_b[p];
  if (busy == 0) return; /* (the whole workgroup) */
  const int k = win.group[w];
  const int ws = win.ws[w], we = win.we[w];
  const long long width = (long long)we - ws;
  const int member0 = g.member0[k], members = g.member0[k + 1] - member0;
  const long long entry0 = g.entry_off[k] + (w - g.win_off[k]) * members;
  const int n_items = n_pen * PAIRS;
  for (int base = 0; base < members; base += MEMBERS) {
    const int in_slab = members - base < MEMBERS ? members - base : MEMBERS;
    /* the slab's rows: per (penalty, member) the sums below the 18 positions */
    for (int x = tid; x < n_pen * in_slab * REFINE; x += THREADS) {
      const int p = x / (in_slab * REFINE), r = x / REFINE % in_slab, slot = x % REFINE;
      const int b = p_b[p];
      long long v = 0;
      if (b > 0) {
        const long long *from = sum + ((long long)p * n_entries + entry0 + base + r) * REFINE;
        const int a8 = clamp_into(position(8, p_s[p], p_e[p], b), ws, we);
        const int a9 = clamp_into(position(9, p_s[p], p_e[p], b), ws, we);
        v = from[0];
        if (slot >= 9) v += from[8] + (a8 < a9 ? from[9] : -from[9]);
        if (slot != 0 && slot != 9) v += from[slot];
      }
      prefix[(p * MEMBERS + r) * REFINE + slot] = v;
    }
    for (int r = tid; r < in_slab; r += THREADS) {
      const long long all = total[entry0 + base + r];
      m_total[r] = all;
      m_flat[r] = term(all, width);
    }
    __syncthreads();
    for (int x = tid; x < n_items; x += THREADS) {
      const int p = x / PAIRS, c = x % PAIRS;
      const int b = p_b[p];
      if (b == 0) continue;
      const int i = c / 9, j = 9 + c % 9;
      const long long s = position(i, p_s[p], p_e[p], b), e = position(j, p_s[p], p_e[p], b);
      double acc = base == 0 ? 0.0 : g_acc[x];
      if (ws < s && s < e && e < we) {
        const long long l1 = s - ws, l2 = e - s, l3 = we - e;
        const double penalty = pen.v[p];
        for (int r = 0; r < in_slab; r++) {
          const long long *row = prefix + (p * MEMBERS + r) * REFINE;
          const long long q_s = row[i], q_e = row[j];
          const long long s1 = q_s, s2 = q_e - q_s, s3 = m_total[r] - q_e;
          const double gain = gain_of(s1, s2, s3, l1, l2, l3, m_flat[r]);
          const double more = gain - penalty;
          acc += feasible(s1, s2, s3, l1, l2, l3) && more > 0.0 ? more : 0.0;
        }
      } else {
        acc = -1.0; /* no candidate */
      }
      g_acc[x] = acc;
    }
    __syncthreads(); /* (the next slab writes the rows again) */
  }
  /* a lane per penalty: the best of its 81 (exact comparisons: the order does not matter) */
  if (tid < n_pen && p_b[tid] > 0) {
    const int b = p_b[tid], s0 = p_s[tid], e0 = p_e[tid];
    double best_g = -1.0;
    int best_s = 0, best_e = 0;
    for (int c = 0; c < PAIRS; c++) {
      const double v = g_acc[tid * PAIRS + c];
      const int cs = clamp_into(position(c / 9, s0, e0, b), ws, we);
      const int ce = clamp_into(position(9 + c % 9, s0, e0, b), ws, we);
      if (v >= 0.0 && (best_g < 0.0 || before(v, cs, ce, best_g, best_s, best_e))) {
        best_g = v;
        best_s = cs;
        best_e = ce;
      }
    }
    const long long pw = (long long)tid * n_windows + w;
    win.s[pw] = best_s;
    win.e[pw] = best_e;
    win.objective[pw] = best_g;
    win.levels[pw] += 1;
    win.b[pw] = b >> 1;
  }
}

/* A thread per (penalty, entry): the member at the window's peak.  sum[]: the fold of the FINAL
 * slots.  Columns at p * n_entries + entry. */
template <int = 0>
__global__ __launch_bounds__(THREADS) void report_kernel(Groups g, int n_groups, long long n_windows,
                                                         long long n_entries, int n_pen,
                                                         Penalties pen, Windows win,
                                                         const long long *sum, double *m_gain,
                                                         int *m_up, long long *m_sum, int *m_bases) {
  psd_tables_init();
  const long long x = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (x >= n_entries * n_pen) return;
  long long w;
  int m;
  entry_of(g, n_groups, x % n_entries, w, m);
  const int p = (int)(x / n_entries);
  const long long pw = (long long)p * n_windows + w;
  const int s = win.s[pw], e = win.e[pw];
  double gain = 0.0;
  long long s2 = 0;
  int up = 0, bases = 0;
  if (s >= 0) {
    const int ws = win.ws[pw], we = win.we[pw];
    const long long s1 = sum[x * FINAL], s3 = sum[x * FINAL + 2];
    const long long l1 = (long long)s - ws, l2 = (long long)e - s, l3 = (long long)we - e;
    s2 = sum[x * FINAL + 1];
    bases = (int)l2;
    const double v = gain_of(s1, s2, s3, l1, l2, l3, term(s1 + s2 + s3, (long long)we - ws));
    if (feasible(s1, s2, s3, l1, l2, l3)) {
      gain = v;
      up = v - pen.v[p] > 0.0;
    }
  }
  m_gain[x] = gain;
  m_up[x] = up;
  m_sum[x] = s2;
  m_bases[x] = bases;
  if (up) atomic_add_i32(win.samples_up + pw, 1);
}

}  // namespace joint_path
}  // namespace psd
#endif
