/* fpop_kernels.h -- the HIP kernels of the PeakSegFPOP hot path.
 *
 *   fpop_forward_kernel   one workgroup per (penalty, contig) problem: wave 0 carries the "up"
 *                         cost function, wave 1 the "down" one (waves 2 and 3, when
 *                         PSD_HELPER_WAVES is defined, are their helpers, fpop_coop.h), through
 *                         the strictly sequential recurrence of
 *                         /root/reference/src/PeakSegFPOPLog.cpp:258-397 (one __syncthreads
 *                         per data point; the two updates of a step only read the previous
 *                         step's functions).  Live piece lists sit in LDS; each step's
 *                         backtrack record {max_log_mean, data_i, prev_log_mean} per piece --
 *                         what the reference serialises to its DiskVector (drv:12-34) -- is
 *                         appended to the in-HBM arena.
 *                         After its last data point the down wave decodes the segmentation
 *                         from the arena (backtrack_wave; drv:399-442: Minimize result, then
 *                         findMean per segment).
 *   math_probe_kernel     element-wise psd_exp / psd_log / psd_div (tests: host == device bit
 *                         for bit) and the compiler's own fp64 division.
 *
 * Included by peakseg_hip.cpp (hipcc, gfx950) and by tests/emu (g++ + hip_emu.h).
 *
 * NO include guard: peakseg_hip.cpp includes this file once per build variant (PSD_VARIANT =
 * namespace name, PSD_LDS_CAP, PSD_HELPER_WAVES), see fpop_wave.h.
 *
 * This file is the umbrella of the kernel side: it includes the parts in order and holds the
 * decoding (backtrack_wave), the kernel body and the kernels.
 *   fpop_arena.h  arena of backtrack records, rescale + append, Minimize
 *   fpop_step.h   one chain's update for one data point, in LDS and in HBM
 *   fpop_sync.h   workgroup barrier, end-of-data-point barrier, spill slot
 *   fpop_ckpt.h   checkpoint slots, the park slot, the overflow pool */
#include "fpop_wave.h"
#include "fpop_arena.h"
#include "fpop_step.h"
#include "fpop_sync.h"
#include "fpop_ckpt.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace psd {
namespace PSD_VARIANT {

/* list ids: 2*chain + buffer for the two cost functions (chain 0 = up, 1 = down), 4 + chain
 * for the chain's min-less / min-more temporary.  Lists live in LDS (g_sm.list[id]) while
 * every function has at most LDS_CAP pieces; when an operation overflows, the step is redone
 * with all lists in the HBM spill area, and the problem returns to LDS once both functions
 * have shrunk below LDS_CAP/2. */
/* State of the decoding (drv:399-442) between two calls of backtrack_wave. */
struct BtState {
  double best_log_mean, prev_log_mean;
  int prev_seg_end, prev_seg_offset; /* offset 0: the next function is an up one, N: a down one */
  int n_seg, n_eq, status;
};

/* Decode the optimal segmentation (drv:399-442): one wave, right after the forward pass of
 * its problem (the arena records it follows were written by this workgroup; fast problems
 * decode while slower ones are still in their forward pass).  Follows the chain of segment
 * ends while it stays at data points >= t_lo (0: to the end); the record of function
 * (up/down, t) is fn_ref[fn_up/fn_down + t - t_origin].  Returns with bt.prev_seg_end < t_lo. */
PSD_D void backtrack_wave(const DeviceArgs &a, int p, int N, BtState &bt, unsigned long long fn_up,
                          unsigned long long fn_down, int t_origin, int t_lo) {
  const int lane = lane_id();
  int *seg_start = a.seg_start + a.prob_seg_off[p];
  double *seg_mean = a.seg_mean + a.prob_seg_off[p];
  double best_log_mean = bt.best_log_mean;
  double prev_log_mean = bt.prev_log_mean;
  int prev_seg_end = bt.prev_seg_end;
  int prev_seg_offset = bt.prev_seg_offset;
  int n_seg = bt.n_seg, n_eq = bt.n_eq, status = bt.status;
  while (t_lo <= prev_seg_end && status == 0) {
    if (n_seg >= N) { /* more segments than data points: cannot happen for a valid store */
      status = PST_BACKTRACK;
      break;
    }
    unsigned long long ref = a.fn_ref[(prev_seg_offset ? fn_down : fn_up) +
                                      (unsigned long long)(prev_seg_end - t_origin)];
    unsigned long long off = ref >> FN_COUNT_BITS;
    int n = (int)(ref & ((1ull << FN_COUNT_BITS) - 1));
    if (lane == 0) {
      seg_start[n_seg] = prev_seg_end;
      seg_mean[n_seg] = d_exp(best_log_mean);
    }
    n_seg++;
    prev_seg_offset = prev_seg_offset == 0 ? N : 0;
    if (prev_log_mean != PSD_INF) {
      best_log_mean = prev_log_mean; /* equality constraint inactive */
    } else {
      n_eq++;
    }
    /* findMean (fpl:643-653) on the restored function (drv:44-54): piece k spans
     * [max_{k-1}, max_k], the first from -Inf; the first match wins. */
    bool found = false;
    const ArenaPtr rec = arena_at(a, off); /* (a record never straddles a block) */
    for (int base = 0; base < n; base += WAVE) {
      int k = base + lane;
      bool hit = false;
      int di = 0;
      double prv = 0.0;
      if (k < n) {
        double mxk = rec.mx[k];
        double mnk = k == 0 ? -PSD_INF : rec.mx[k - 1];
        di = rec.di[k];
        prv = rec.prv[k];
        hit = mnk <= best_log_mean && best_log_mean <= mxk;
      }
      unsigned long long m = ballot(hit);
      if (m) {
        int src = ctz64(m);
        prev_seg_end = rdlane_i(di, src);
        prev_log_mean = rdlane_d(prv, src);
        found = true;
        break;
      }
    }
    if (!found) {
      status = PST_BACKTRACK;
      break;
    }
  }
  if (status == 0 && prev_seg_end < 0) { /* the first segment (drv:442) */
    if (lane == 0) {
      seg_start[n_seg] = -1;
      seg_mean[n_seg] = d_exp(best_log_mean);
    }
    n_seg++;
  }
  bt.best_log_mean = best_log_mean;
  bt.prev_log_mean = prev_log_mean;
  bt.prev_seg_end = prev_seg_end;
  bt.prev_seg_offset = prev_seg_offset;
  bt.n_seg = n_seg;
  bt.n_eq = n_eq;
  bt.status = status;
}

/* The end of a chain's step: its piece count for the other wave (0 with an error), or the error
 * for both waves, in the slot of the barrier that follows. */
PSD_D void step_publish(int lane, int id_own_new, int n_new, unsigned slot) {
  if (lane == 0) g_sm.n[id_own_new] = n_new < 0 ? 0 : n_new;
  if (n_new < 0) {
    if (lane == 0) {
      g_sm.abort_err[slot] = -n_new;
      g_sm.abort_status[slot] = ((-n_new) & WERR_ARENA)      ? PST_ARENA_FULL
                                : ((-n_new) & WERR_OVERFLOW) ? PST_LDS_OVERFLOW
                                                             : PST_REF_THROW;
    }
  }
}

/* -DPSD_LOOP_STATS (a test build): per chain wave, the data points taken inside the inner loop of
 * the usual data point, those taken by the general code, and the entries into the inner loop */
enum { LOOP_INSIDE = 0, LOOP_GENERAL = 1, LOOP_ENTRIES = 2 };
#undef PSD_LOOP_COUNT
#ifdef PSD_LOOP_STATS
#define PSD_LOOP_COUNT(which)                                   \
  do {                                                          \
    if (lane_id() == 0) g_sm.loop_stats[wave_id() & 1][which]++; \
  } while (0)
#else
#define PSD_LOOP_COUNT(which) \
  do {                        \
  } while (0)
#endif

/* PSD_KERNEL_WAVES_PER_EU (throughput build): keep the kernel's own register use within the
 * budget of that many waves per SIMD, as the out-of-line operations already are */
#undef PSD_KERNEL_OCC
#if defined(PSD_KERNEL_WAVES_PER_EU) && !defined(PSD_EMU)
#define PSD_KERNEL_OCC \
  __attribute__((amdgpu_waves_per_eu(PSD_KERNEL_WAVES_PER_EU, PSD_KERNEL_WAVES_PER_EU)))
#else
#define PSD_KERNEL_OCC
#endif
/* The kernel body.  CKPT = false: the full store, one pass (everything about passes and
 * checkpoints below folds away: the loop is the one the latency numbers were tuned on);
 * CKPT = true: the checkpointed store's passes. */
template <bool CKPT>
PSD_D void forward_body(const DeviceArgs &a) {
  /* What a problem is made of is the same in every lane, but it is read from tables in HBM that
   * the compiler will not read with scalar loads: say that it is uniform, or the number of data
   * points arrives in a vector register, the loop's exit test becomes a vector compare and the
   * data-point counter with everything derived from it (the lane of the data block, fn_index,
   * every test of t) moves to vector registers and lane masks with it. */
  const int p = uniform_i(a.prob_order[blockIdx.x]);
  const int chain = uniform_i(wave_id()) & 1; /* uniform per wave: say so (scalar branches) */
  const int lane = lane_id();
  const int contig = uniform_i(a.prob_contig[p]);
  const int N = uniform_i(a.contig_n[contig]);
  const double penalty = uniform_d(a.prob_penalty[p]);
  const long long contig_off = (long long)uniform_u64((unsigned long long)a.contig_off[contig]);
  const int *count = a.count + contig_off;
  const int *weight = a.weight + contig_off;
  const LdsList mlist = lds_list(4 + chain);
  LdsScratch lsc;
  lsc.w = chain;

  psd_tables_init(); /* exp/log tables -> LDS */
  if (threadIdx.x == 0) {
    if (a.started) atomicAdd_system(a.started, 1);
    g_sm.abort_status[0] = g_sm.abort_status[1] = g_sm.abort_status[2] = 0;
    g_sm.abort_err[0] = g_sm.abort_err[1] = g_sm.abort_err[2] = 0;
    for (int i = 0; i < 6; i++) g_sm.n[i] = 0;
    g_sm.serial[0] = g_sm.serial[1] = 0;
    g_sm.total_up = 0; /* (read by the down wave's result even when the pass stops early) */
    g_sm.max_up = 0;
    g_sm.arrived[0] = g_sm.arrived[1] = 0xffffffffu;
#ifdef PSD_SPIN_STATS
    g_sm.spin_max[0] = g_sm.spin_max[1] = g_sm.spin_max[2] = g_sm.spin_max[3] = 0;
#endif
#ifdef PSD_LOOP_STATS
    for (int i = 0; i < 3; i++) g_sm.loop_stats[0][i] = g_sm.loop_stats[1][i] = 0;
#endif
#ifdef PSD_PROFILE
    for (int i = 0; i < N_PROF; i++)
      g_sm.prof[0][i] = g_sm.prof[1][i] = g_sm.prof[2][i] = g_sm.prof[3][i] = 0;
#endif
#ifdef PSD_HELPER_WAVES
    for (int c = 0; c < 2; c++) {
      g_sm.mail[c].seq_cmd = g_sm.mail[c].seq_done = 0;
      g_sm.mail[c].op = 0;
      g_sm.mail[c].abort = 0;
    }
#endif
  }
  __syncthreads();
#ifdef PSD_HELPER_WAVES
  if (wave_id() >= 2) {
    helper_loop(chain, a);
    return;
  }
#endif

  /* Passes over the data.  Full store (ckpt_interval = 0): one pass, every function recorded,
   * then the decoding.  Checkpointed store: a forward pass that records nothing but a
   * checkpoint every K data points, then, led by the decoding, one pass per block of K data
   * points that holds a segment end, from that block's checkpoint and with the records kept
   * in this wave's region of the arena. */
  const int K = CKPT ? a.ckpt_interval : 0;
  const unsigned long long fn_stride = K > 0 ? (unsigned long long)K + 1ull : (unsigned long long)N;
  const unsigned long long fn_up = uniform_u64((unsigned long long)a.prob_fn_off[p]);
  const unsigned long long fn_down = fn_up + fn_stride;
  const unsigned long long fn_mine = chain == 1 ? fn_down : fn_up;
  ArenaCursor cur;
  cursor_clear(cur, K > 0 ? 0 : 1);
  unsigned long long total_intervals = 0;
  int max_intervals = 0;
  int spill_steps = 0;
  int status = 0;
  double cum_weight_i = 0.0, cum_weight_prev_i = -1.0;
  int cnt_reg = 0, wt_reg = 0;
  int b = 0;        /* buffer holding step t-1 */
  /* (the flags of the loop are integers, not bools: a uniform bool that lives across blocks is
   * kept as a 64-bit lane mask and tested through vcc, an integer is tested with a scalar compare) */
  int in_hbm = 0; /* where the lists of step t-1 live */
  int spill_slot = -1; /* this problem's slot of the HBM spill pool, taken on first overflow */
  int t = 0;
  int t_lo = 0, t_hi = N; /* data points of this pass */
  int t_first = 0;        /* where this pass starts: t_lo, or the data point a parked problem resumes at */
  int t_origin = 0;       /* fn_ref index of data point t: t - t_origin */
  int next_ckpt = K > 0 ? K : -1;
  int forward = 1;        /* the first pass */
  int step_reached = 0;
  int parked = 0;
  BtState bt;
  bt.best_log_mean = bt.prev_log_mean = 0.0;
  bt.prev_seg_end = -1;
  bt.prev_seg_offset = 0;
  bt.n_seg = bt.n_eq = bt.status = 0;
  ProbResult r;
  r.best_cost = 0.0;
  r.best_log_mean = 0.0;
  r.prev_log_mean = 0.0;
  r.prev_seg_end = -1;
  unsigned sync_no = 0; /* parity slot of the abort flags: one per barrier */
  if (lane == 0) g_sm.t_begin[chain] = cycle_now(); /* (in LDS: read once, at the end) */
  int resumed_abort = 0;
  if (!CKPT && a.prob_resume != nullptr) {
    /* A problem parked by an earlier launch (the arena had run out): its two functions, the
     * cumulated weight and its counters come back from the park slot and the pass goes on at
     * the data point it had reached. */
    const int t_resume = uniform_i(a.prob_resume[p]);
    if (t_resume > 0) {
      device_fence();
      in_hbm = (uniform_i(ckpt_count(*a.self, p, 0, 0)) > LDS_CAP ||
                uniform_i(ckpt_count(*a.self, p, 0, 1)) > LDS_CAP) ? 1 : 0;
      if (in_hbm) {
        spill_slot = uniform_i(take_spill_slot(*a.self, chain));
        if (spill_slot < 0) {
          /* (the pool has no slot yet for these long functions: the park slot stays as it is
           * and the problem resumes here again once the host has enlarged the pool) */
          status = PST_SPILL_FULL;
          resumed_abort = 1;
          parked = 1;
          step_reached = t_resume;
        }
      }
      if (!resumed_abort) {
        const int n_ck = uniform_i(ckpt_load(*a.self, p, 0, chain, 2 * chain, in_hbm ? 1 : 0,
                                             spill_slot));
        if (lane == 0) g_sm.n[2 * chain] = n_ck;
        cum_weight_i = uniform_d(ckpt_cum_weight(*a.self, p, 0));
        cum_weight_prev_i = cum_weight_i;
        /* (results of calls arrive in vector registers: the statistics are scalar sums) */
        total_intervals = uniform_u64(park_total_intervals(*a.self, p, chain));
        max_intervals = uniform_i(park_int(*a.self, p, 3 + chain));
        spill_steps = uniform_i(park_int(*a.self, p, 5));
        {
          const int n_serial = park_int(*a.self, p, 6 + chain);
          if (lane == 0) g_sm.serial[chain] = n_serial;
        }
        t_first = t_resume; /* (t_lo stays 0: the decoding goes back to the first data point) */
        block_sync(chain); /* both functions are in place before either chain reads the other's */
      }
    }
  }
  for (;;) { /* passes */
  if (resumed_abort) break;
  int reload = 1; /* cnt_reg / wt_reg do not hold the 64 data points around t */
  for (t = t_first; t < t_hi; t++) {
    int synced = 0; /* the inner loop left this data point after its barrier, with a status */
#ifndef PSD_CALL_LDS_OPS
    /* The usual data point (latency build, full store) in a loop of its own: t >= 2, lists in
     * LDS, functions short enough for chain_step_fast, no error.  It holds what such a data point
     * does and no call of a cold function, so that what the cold paths need lives around it and
     * not in it.  Anything else leaves it: a function that outgrew the fast sizes and a rare
     * argument (-WERR_SERIAL) before anything of the data point is written -- the general code
     * below computes it -- and a status after the barrier (arena full, an overflow seen by the
     * other wave, a helper that never came), which the general code's dispatch takes over as it
     * is.  The pass tries the loop again at the next data point. */
    if (!CKPT && t >= 2 && !in_hbm) {
      int entry = 1; /* first data point of this entry: the data block is read whatever t is */
      cur.store = 1;
      /* (the statistics: sums in vector registers while the loop runs, see PSD_VECTOR_REG;
       * spill_steps cannot change here) */
      unsigned long long total_v = total_intervals;
      int max_v = max_intervals;
      PSD_VECTOR_REG(total_v);
      PSD_VECTOR_REG(max_v);
      for (;;) {
        PSD_PROF_T0();
        const int nb = b ^ 1;
        const int n_own = uniform_i(g_sm.n[2 * chain + b]);
        const int n_other = uniform_i(g_sm.n[2 * (1 - chain) + b]);
        if (n_other > FAST_MAX_OTHER || n_own > FAST_MAX_OWN) break;
        if (entry || (t & 63) == 0) { /* coalesced read of the next 64 data points */
          int tt = (t & ~63) + lane;
          cnt_reg = tt < N ? count[tt] : 0;
          wt_reg = tt < N ? weight[tt] : 0;
          if (entry) PSD_LOOP_COUNT(LOOP_ENTRIES);
          entry = 0;
        }
        const int coverage = rdlane_i(cnt_reg, t & 63);
        const double w = (double)rdlane_i(wt_reg, t & 63);
        const double cum_weight_new = cum_weight_i + w;
        /* (penalty / W_{t-1} belongs to min-less: only the up chain divides) */
        double pen_term = 0.0;
        if (chain == 0) pen_term = penalty / cum_weight_prev_i;
        /* (the count comes out of LDS and lane operations: say that it is uniform before it
         * decides a way out of the loop, or every value the loop carries counts as divergent) */
        const int n_new = uniform_i(chain_step_fast<USE_HELPER>(
            a, cur, fn_mine + (unsigned long long)(t - t_origin), chain, t,
            lds_list(2 * (1 - chain) + b), n_other, lds_list(2 * chain + b), n_own,
            lds_list(2 * chain + nb), mlist, lsc, pen_term, cum_weight_prev_i, w, coverage,
            cum_weight_new));
        if (n_new == -WERR_SERIAL) break; /* nothing written: the general step redoes it */
        synced = 1;
        { /* report, meet the other wave (as in the general code below) */
          PSD_PROF_T0();
          const unsigned slot = sync_no % 3u;
          step_publish(lane, 2 * chain + nb, n_new, slot);
          PSD_PROF_ADD(PROF_ARENA);
          if (!step_sync(chain, sync_no)) {
            status = PST_REF_THROW;
            if (lane == 0) g_sm.abort_err[slot] = WERR_HELPER;
            break;
          }
          PSD_PROF_ADD(PROF_BARRIER);
          status = uniform_i(g_sm.abort_status[slot]);
          if (lane == 0) g_sm.abort_status[(sync_no + 2u) % 3u] = 0;
          sync_no++;
        }
        if (status != 0) break;
        synced = 0;
        PSD_LOOP_COUNT(LOOP_INSIDE);
        total_v += (unsigned long long)n_new;
        if (max_v < n_new) max_v = n_new;
        cum_weight_i = cum_weight_new;
        cum_weight_prev_i = cum_weight_i;
        b = nb;
        t++;
        if (t >= t_hi) break;
      }
      total_intervals = uniform_u64(total_v);
      max_intervals = uniform_i(max_v);
      if (!entry) reload = 1; /* the general code keeps no data block across this loop */
      if (t >= t_hi) break;
    }
#endif
    PSD_PROF_T0();
    if (!CKPT) cur.store = 1; /* known to the compiler even after a cold call returned the cursor */
    if ((t & 63) == 0 || reload) { /* coalesced read of the next 64 data points */
      int tt = (t & ~63) + lane;
      cnt_reg = tt < N ? count[tt] : 0;
      wt_reg = tt < N ? weight[tt] : 0;
      reload = 0;
    }
    const int coverage = rdlane_i(cnt_reg, t & 63);
    const double w = (double)rdlane_i(wt_reg, t & 63);
    const double cum_weight_new = cum_weight_i + w;
    const int nb = b ^ 1;
    const int id_own_prev = 2 * chain + b, id_own_new = 2 * chain + nb;
    const int id_other_prev = 2 * (1 - chain) + b;
    const int n_own = uniform_i(g_sm.n[id_own_prev]);
    const int n_other = uniform_i(g_sm.n[id_other_prev]);
    const unsigned long long fn_index = fn_mine + (unsigned long long)(t - t_origin);
    /* come back from HBM when both functions fit comfortably again */
    if (in_hbm && n_own <= LDS_CAP / 2 && n_other <= LDS_CAP / 2) {
      move_list_hbm(*a.self, spill_slot, id_own_prev, n_own, 0);
      in_hbm = 0;
      block_sync(chain);
    }
    int n_new = 0;
    for (;;) { /* at most two passes: LDS, then HBM after an overflow */
      if (!synced) {
      if (t == 0) {
        ArenaCursor cur0 = cur; /* only this copy has its address taken */
        n_new = uniform_i(first_point(*a.self, cur0, fn_index, chain, contig, coverage, id_own_new));
        cur = cur0;
      } else if (!in_hbm) {
#ifdef PSD_CALL_LDS_OPS /* throughput build: operations out of line (register budget) */
        n_new = chain_step<USE_HELPER>(a, cur, fn_index, chain, t,
                           lds_list(id_other_prev), n_other, lds_list(id_own_prev),
                           n_own, lds_list(id_own_new), mlist, lsc,
                           penalty / cum_weight_prev_i, cum_weight_prev_i, w, coverage,
                           cum_weight_new);
#else
        /* (full store: the usual case has its own loop above and comes here with what that
         * loop would not take) */
        n_new = -WERR_SERIAL;
        if (CKPT && t >= 2 && n_other <= FAST_MAX_OTHER && n_own <= FAST_MAX_OWN) {
          n_new = uniform_i(chain_step_fast<USE_HELPER>(
              a, cur, fn_index, chain, t, lds_list(id_other_prev), n_other,
              lds_list(id_own_prev), n_own, lds_list(id_own_new), mlist, lsc,
              penalty / cum_weight_prev_i, cum_weight_prev_i, w, coverage, cum_weight_new));
        }
        if (n_new == -WERR_SERIAL) { /* not the usual case, or it needs the sequential replay */
          ArenaCursor cur_gen = cur; /* only this copy has its address taken */
          n_new = uniform_i(chain_step_lds<USE_HELPER>(
              *a.self, cur_gen, fn_index, chain, t, id_other_prev, n_other,
              id_own_prev, n_own, id_own_new, penalty / cum_weight_prev_i, cum_weight_prev_i, w,
              coverage, cum_weight_new));
          cur = cur_gen;
        }
#endif
      } else {
        ArenaCursor cur_hbm = cur; /* only this copy has its address taken */
        n_new = uniform_i(chain_step_hbm(*a.self, cur_hbm, fn_index, spill_slot, chain, t,
                               id_other_prev, n_other, id_own_prev, n_own, id_own_new,
                               penalty / cum_weight_prev_i, cum_weight_prev_i, w, coverage,
                               cum_weight_new));
        cur = cur_hbm;
        /* With the lists in HBM the two waves first meet at the workgroup barrier, so that the
         * flag barrier below finds the other wave there already: a wave that polled LDS while
         * the other one worked through lists in HBM with FLAT instructions (issued to the LDS
         * pipeline too) cost half as much again per data point (config 5, 1e5 data points:
         * 7.6 s -> 11.4 s; profiles/r02/ab_step_barrier.log).  The lists are reached with
         * global_* instructions now and polling is harmless; the barrier stays as a guard.
         * in_hbm is the same in both waves. */
        block_sync_cold(chain);
      }
      /* ---- end of pass: report, store the backtrack record, meet the other wave ---- */
      PSD_PROF_T0();
      const unsigned slot = sync_no % 3u;
      step_publish(lane, id_own_new, n_new, slot);
      PSD_PROF_ADD(PROF_ARENA);
      if (!step_sync(chain, sync_no)) {
        status = PST_REF_THROW;
        if (lane == 0) g_sm.abort_err[slot] = WERR_HELPER;
        break;
      }
      PSD_PROF_ADD(PROF_BARRIER);
      status = uniform_i(g_sm.abort_status[slot]);
      /* three rotating slots: the one cleared here is first written two barriers later */
      if (lane == 0) g_sm.abort_status[(sync_no + 2u) % 3u] = 0;
      sync_no++;
      }
      synced = 0;
#ifdef PSD_PARK_ON_LDS_OVERFLOW
      /* the packed build: a function that outgrows its short lists is for the throughput build
       * (the problem is parked below and resumed there), not for the HBM path */
      if (status == PST_LDS_OVERFLOW && !CKPT && a.prob_resume != nullptr && t > 0) break;
#endif
      if (status == PST_LDS_OVERFLOW && !in_hbm && a.spill_cap > LDS_CAP && t > 0) {
        /* redo this data point with the lists in HBM: every wave moves its own t-1 list */
        if (spill_slot < 0) {
          spill_slot = uniform_i(take_spill_slot(*a.self, chain)); /* a call's result: say it is uniform */
          if (spill_slot < 0) {
            status = PST_SPILL_FULL;
            break;
          }
        }
        move_list_hbm(*a.self, spill_slot, id_own_prev, n_own, 1);
        in_hbm = 1;
        status = 0;
        block_sync(chain);
        continue;
      }
      break;
    }
    if (status != 0) {
      /* (no spill slot: this data point's inputs are still in LDS -- the pool was needed for
       * its result -- so the problem parks like one that ran out of arena and goes on at this
       * data point when the host has enlarged the pool, instead of starting over) */
#ifdef PSD_PARK_ON_LDS_OVERFLOW
      const bool park_now = status == PST_ARENA_FULL || status == PST_SPILL_FULL ||
                            status == PST_LDS_OVERFLOW;
#else
      const bool park_now = status == PST_ARENA_FULL || status == PST_SPILL_FULL;
#endif
      if (!CKPT && park_now && a.prob_resume != nullptr && t > 0) {
        /* Out of arena (or of spill slots): park.  The functions of data point t-1 (this step's inputs, untouched)
         * go to the park slot; the host adds arena blocks and resumes the problem at t.  Both
         * waves see the status, so both come here.  (Functions too long for a slot need the
         * overflow pool; without room there the problem is simply rerun from the start.) */
        const int n_up = uniform_i(g_sm.n[b]), n_down = uniform_i(g_sm.n[2 + b]);
        unsigned long long ovf = 0;
        bool can_park = true;
        if (n_up > a.ckpt_cap || n_down > a.ckpt_cap) {
          ovf = psd_d2u(uniform_d(psd_u2d(ckpt_take_overflow(*a.self, chain, n_up, n_down))));
          if (ovf == ~0ull) can_park = false;
          if (can_park && chain == 1 && n_up > a.ckpt_cap) ovf += (unsigned long long)n_up;
        }
        if (can_park) {
          ckpt_save(*a.self, p, 0, chain, 2 * chain + b, chain == 0 ? n_up : n_down, cum_weight_i,
                    in_hbm ? 1 : 0, spill_slot, ovf);
          park_counters_save(*a.self, p, chain, t, total_intervals, max_intervals, spill_steps);
          parked = 1;
        }
      }
      break;
    }
    PSD_LOOP_COUNT(LOOP_GENERAL);
    if (!CKPT || forward) {
      total_intervals += (unsigned long long)n_new;
      if (max_intervals < n_new) max_intervals = n_new;
      if (in_hbm) spill_steps++;
    }
    cum_weight_i = cum_weight_new;
    cum_weight_prev_i = cum_weight_i;
    b = nb;
    if (CKPT && t == next_ckpt) { /* forward pass: keep the two live functions */
      /* both counts are visible to both waves since the barrier of this data point */
      const int n_up = uniform_i(g_sm.n[b]), n_down = uniform_i(g_sm.n[2 + b]);
      unsigned long long ovf = 0;
      if (n_up > a.ckpt_cap || n_down > a.ckpt_cap) { /* beyond a slot: the overflow pool */
        ovf = psd_d2u(uniform_d(psd_u2d(ckpt_take_overflow(*a.self, chain, n_up, n_down))));
        if (ovf == ~0ull) {
          status = PST_CKPT_FULL; /* in both waves */
          break;
        }
        if (chain == 1 && n_up > a.ckpt_cap) ovf += (unsigned long long)n_up;
      }
      ckpt_save(*a.self, p, t / K - 1, chain, 2 * chain + b, n_new, cum_weight_i, in_hbm ? 1 : 0,
                spill_slot, ovf);
      next_ckpt += K;
    }
  }
  if (!CKPT || forward) step_reached = t;
  if (status != 0) break;
  /* ---- after a pass ---- */
  if (forward) {
    /* Minimize the final down function (drv:404-406) */
    if (chain == 0 && lane == 0) {
      g_sm.total_up = total_intervals;
      g_sm.max_up = max_intervals;
    }
  }
  device_fence(); /* the stored functions of both chains are read back by backtrack_wave */
  block_sync(chain);
  if (chain == 1) {
    if (forward) {
      const int id = 2 + b;
      if (in_hbm) {
        minimize_wave(global_list(a, spill_slot, id), g_sm.n[id], &r.best_cost, &r.best_log_mean,
                      &r.prev_seg_end, &r.prev_log_mean);
      } else {
        minimize_wave(lds_list(id), g_sm.n[id], &r.best_cost, &r.best_log_mean, &r.prev_seg_end,
                      &r.prev_log_mean);
      }
      bt.best_log_mean = r.best_log_mean;
      bt.prev_log_mean = r.prev_log_mean;
      bt.prev_seg_end = r.prev_seg_end;
    }
    /* decode as far as the records at hand reach: everything (full store), the segment ends
     * inside the block just recomputed, or -- after the forward pass of the checkpointed store
     * -- nothing but the one-segment model's only row */
    backtrack_wave(a, p, N, bt, fn_up, fn_down, t_origin, (K > 0 && forward) ? N : t_lo);
  }
  if (!CKPT || K == 0) break;
  /* checkpointed store: which block holds the next segment end?  (-1: decoding complete) */
  if (chain == 1 && lane == 0) {
    int c = -1;
    if (bt.status == 0 && bt.prev_seg_end >= 0)
      c = bt.prev_seg_end == 0 ? 0 : (bt.prev_seg_end - 1) / K;
    g_sm.bt_next = c;
  }
  block_sync(chain);
  const int c = uniform_i(g_sm.bt_next);
  if (c < 0) break;
  /* next pass: data points c K + 1 .. (c + 1) K (block 0 also redoes data point 0), from the
   * checkpoint after data point c K, records into this wave's region of the arena */
  forward = 0;
  next_ckpt = -1;
  t_origin = c * K;
  t_lo = c == 0 ? 0 : c * K + 1;
  t_hi = (c + 1) * K + 1 < N ? (c + 1) * K + 1 : N;
  t_first = t_lo;
  {
    /* this wave's region: regions are packed whole into the arena's blocks */
    const unsigned long long per_block = (1ull << a.ar_block_log2) / a.ckpt_region;
    const unsigned long long region = (unsigned long long)p * 2ull + (unsigned long long)chain;
    cursor_point(a, cur, ((region / per_block) << a.ar_block_log2) + (region % per_block) * a.ckpt_region,
                 (int)a.ckpt_region);
    cur.store = 1;
  }
  in_hbm = 0;
  b = 0;
  if (c == 0) {
    cum_weight_i = 0.0;
    cum_weight_prev_i = -1.0;
    if (lane == 0) g_sm.n[2 * chain] = g_sm.n[2 * chain + 1] = 0;
  } else {
    device_fence();
    /* functions that do not fit LDS: the block starts with the lists in the HBM spill area
     * (the same decision in both waves: both counts are in the checkpoint) */
    in_hbm = (uniform_i(ckpt_count(*a.self, p, c - 1, 0)) > LDS_CAP ||
              uniform_i(ckpt_count(*a.self, p, c - 1, 1)) > LDS_CAP) ? 1 : 0;
    if (in_hbm && spill_slot < 0) {
      spill_slot = uniform_i(take_spill_slot(*a.self, chain));
      if (spill_slot < 0) {
        status = PST_SPILL_FULL;
        break;
      }
    }
    const int n_ck = uniform_i(ckpt_load(*a.self, p, c - 1, chain, 2 * chain, in_hbm ? 1 : 0,
                                         spill_slot));
    if (lane == 0) g_sm.n[2 * chain] = n_ck;
    cum_weight_i = uniform_d(ckpt_cum_weight(*a.self, p, c - 1));
    cum_weight_prev_i = cum_weight_i;
  }
  block_sync(chain); /* both functions are in LDS before either chain reads the other's */
  } /* passes */
#ifdef PSD_HELPER_WAVES
  if (mail_wait(chain)) mail_post(chain, HOP_EXIT);
  else if (lane == 0) g_sm.mail[chain].abort = 1;
#endif
#ifdef PSD_PROFILE
  if (lane == 0 && a.prof) {
    long long *dst = a.prof + ((long long)p * 2 + chain) * N_PROF;
    for (int i = 0; i < N_PROF; i++) dst[i] = g_sm.prof[chain][i];
    dst[PROF_TOTAL] = cycle_now() - g_sm.t_begin[chain];
  }
#endif
  if (chain == 1) {
    r.status = status != 0 ? status : bt.status;
    r.wave_err = g_sm.abort_err[0] | g_sm.abort_err[1] | g_sm.abort_err[2];
    r.max_intervals = max_intervals > g_sm.max_up ? max_intervals : g_sm.max_up;
    r.total_intervals = total_intervals + g_sm.total_up;
    r.n_segments = bt.n_seg;
    r.n_equality = bt.n_eq;
    r.n_serial_env = g_sm.serial[0] + g_sm.serial[1];
    r.step_reached = step_reached;
    r.spill_steps = spill_steps;
    r.parked = parked;
    r.max_spin = 0;
#ifdef PSD_SPIN_STATS
    for (int w = 0; w < 4; w++) r.max_spin = g_sm.spin_max[w] > r.max_spin ? g_sm.spin_max[w] : r.max_spin;
#endif
#ifdef PSD_LOOP_STATS
    /* (the up wave's counts are complete: the waves met after the pass) */
    for (int i = 0; i < 6; i++) r.loop_stats[i] = g_sm.loop_stats[i / 3][i % 3];
#endif
    r.cycles = cycle_now() - g_sm.t_begin[chain];
    if (lane == 0) a.result[p] = r;
  }
}

__global__ __launch_bounds__(FORWARD_THREADS) PSD_KERNEL_OCC void fpop_forward_kernel(
    DeviceArgs a) {
  forward_body<false>(a);
}
/* the same for problem sets that use the checkpointed store (a.ckpt_interval > 0) */
__global__ __launch_bounds__(FORWARD_THREADS) PSD_KERNEL_OCC void fpop_forward_ckpt_kernel(
    DeviceArgs a) {
  forward_body<true>(a);
}

__global__ void math_probe_kernel(int op, int n, const double *x, double *y) {
  psd_tables_init();
  int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n) {
    if (op == 2) /* (x holds n numerators, then n denominators) */
      y[i] = psd_div(x[i], x[n + i]);
    else if (op == 3) /* the compiler's division sequence as it is (what psd_div repairs) */
      y[i] = x[i] / x[n + i];
    else
      y[i] = op == 0 ? d_exp(x[i]) : d_log(x[i]);
  }
}

}  // namespace PSD_VARIANT
}  // namespace psd
