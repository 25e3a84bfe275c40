/* fpop_step.h -- one chain's update for one data point.
 *
 * The accessors of a problem's slot of the HBM spill pool, the step in its three forms
 * (chain_step_ops: the skeleton, its three operations supplied by the caller; chain_step:
 * operations out of line, lists in LDS or HBM; chain_step_fast: the usual case inlined;
 * chain_step_hbm: shared with the helper wave), data point 0, and moving a list between LDS
 * and HBM.
 *
 * Reached only through fpop_kernels.h: no include guard, compiled once per build variant into
 * namespace psd::PSD_VARIANT. */
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace psd {
namespace PSD_VARIANT {

/* lists / scratch of spill-pool slot p (a problem's slot, see take_spill_slot) */
PSD_D GlobalList global_list(const DeviceArgs &a, int p, int id) {
  const size_t cap = (size_t)a.spill_cap;
  gdouble *f = (gdouble *)(a.spill_f64 + ((size_t)p * 48 + (size_t)id * 6) * cap);
  GlobalList r;
  r.Lin_ = f;
  r.Log_ = f + cap;
  r.Con_ = f + 2 * cap;
  r.mn_ = f + 3 * cap;
  r.mx_ = f + 4 * cap;
  r.prv_ = f + 5 * cap;
  r.di_ = (gint *)(a.spill_i32 + ((size_t)p * 12 + (size_t)id) * cap);
  return r;
}
PSD_D GlobalScratch global_scratch(const DeviceArgs &a, int p, int wave) {
  const size_t cap = (size_t)a.spill_cap;
  gdouble *f = (gdouble *)(a.spill_f64 + ((size_t)p * 48 + 36 + (size_t)wave * 6) * cap);
  gint *q = (gint *)(a.spill_i32 + ((size_t)p * 12 + 6) * cap);
  GlobalScratch r;
  r.lc_ = f;
  r.rc_ = f + cap;
  r.om_ = f + 2 * cap;
  r.mu_ = f + 3 * cap;
  r.muc_ = f + 4 * cap;
  r.oc2_ = f + 5 * cap;
  r.cls_ = q + (size_t)wave * cap;
  r.iv_ = q + 2 * cap + (size_t)wave * 2 * cap;
  r.iv_cap_ = 2 * a.spill_cap;
  return r;
}

/* The end of every step, whatever computed the envelope: multiply, add the data point, multiply
 * (drv:316-321,365-370) and the backtrack record appended, once the whole function is written.
 * Returns the piece count, or -WERR_ARENA when the arena is full. */
template <class L>
PSD_D int step_tail(const DeviceArgs &a, ArenaCursor &cur, unsigned long long fn_index,
                    const L &own_new, int n_new, double cum_weight_prev, double w, int coverage,
                    double cum_weight) {
  PSD_PROF_T0();
  wave_sync();
  bool ok = scale_add_store_wave(a, cur, own_new, n_new, fn_index, true, cum_weight_prev, w,
                                 (double)(-coverage) * w, 1 / cum_weight);
  wave_sync();
  PSD_PROF_ADD(PROF_SCALE);
  return ok ? n_new : -WERR_ARENA;
}

/* One chain's update for data point t >= 1 (chain 0: up_t, chain 1: down_t):
 *   up_t   = min_env(min_less(down_{t-1}) + penalty/W_{t-1}, up_{t-1})   drv:273-300
 *   down_t = min_env(min_more(up_{t-1}),                    down_{t-1})  drv:324-349
 *   (t == 1: up_1 = the min-less result, down_1 = down_0)
 * then multiply, add the data point, multiply (drv:316-321,365-370).
 * The three operations are the caller's: min_less() / min_more() leave their result in mlist
 * (min-more at its far end) and return its piece count, min_env(nm) writes own_new; each
 * returns -(WERR_* bits) on error.  Returns the new piece count or -(WERR_* bits). */
template <class L, class Less, class More, class Env>
PSD_D int chain_step_ops(const DeviceArgs &a, ArenaCursor &cur, unsigned long long fn_index,
                         int chain, int t, const L &own_prev, int n_own, const L &own_new,
                         const L &mlist, double cum_weight_prev, double w, int coverage,
                         double cum_weight, Less &&min_less, More &&min_more, Env &&min_env) {
  int nm = 0;
  if (chain == 0) {
    nm = min_less();
  } else if (t >= 2) {
    nm = min_more();
  }
  nm = uniform_i(nm); /* return values of out-of-line functions arrive in a VGPR */
  if (nm < 0) return nm;
  int n_new;
  if (t == 1) {
    if (chain == 0) {
      copy_list_wave(mlist, nm, own_new);
      n_new = nm;
    } else {
      copy_list_wave(own_prev, n_own, own_new);
      n_new = n_own;
    }
  } else {
    n_new = uniform_i(min_env(nm));
  }
  if (n_new < 0) return n_new;
  return step_tail(a, cur, fn_index, own_new, n_new, cum_weight_prev, w, coverage, cum_weight);
}

/* The step with its operations out of line, one wave on lists in LDS or HBM. */
template <bool HELP, class L, class S>
PSD_D int chain_step(const DeviceArgs &a, ArenaCursor &cur, unsigned long long fn_index,
                     int chain, int t, const L &other_prev, int n_other, const L &own_prev,
                     int n_own, const L &own_new, const L &mlist, const S &sc, double pen_term,
                     double cum_weight_prev, double w, int coverage, double cum_weight) {
  /* (in LDS a constant here, not a captured value: the out-of-line operations are compiled for
   * the one capacity they are ever called with) */
  const int cap = L::in_lds ? LDS_CAP : a.spill_cap;
  /* in LDS the versions specialised for short functions when they apply */
  /* (the specialised versions answer -WERR_SERIAL when they met a rare exp / log argument:
   * their arithmetic has no branch for those, the general versions do) */
  return chain_step_ops(
      a, cur, fn_index, chain, t, own_prev, n_own, own_new, mlist, cum_weight_prev, w, coverage,
      cum_weight,
      [&]() {
        int nm = -WERR_SERIAL;
        if (L::in_lds && n_other <= WAVE)
          nm = uniform_i(min_less_small_wave(other_prev, n_other, mlist, cap, sc, t - 1, pen_term));
        if (nm == -WERR_SERIAL)
          nm = min_less_wave(other_prev, n_other, mlist, cap, sc, t - 1, pen_term);
        return nm;
      },
      [&]() {
        int nm = -WERR_SERIAL;
        if (L::in_lds && n_other <= WAVE)
          nm = uniform_i(min_more_small_wave(other_prev, n_other, mlist, cap, sc, t - 1));
        if (nm == -WERR_SERIAL) nm = min_more_wave(other_prev, n_other, mlist, cap, sc, t - 1);
        return nm;
      },
      [&](int nm) {
        const L f1 = chain == 0 ? mlist : mlist.shifted(cap - nm);
        int n_new = -WERR_SERIAL;
        if (L::in_lds && nm <= 32 && n_own <= 32)
          n_new = uniform_i(
              min_env_small_wave<HELP>(f1, nm, own_prev, n_own, own_new, cap, sc, chain));
        if (n_new == -WERR_SERIAL)
          n_new = min_env_wave<HELP>(f1, nm, own_prev, n_own, own_new, cap, sc, chain);
        return n_new;
      });
}

/* The same update for the usual case -- data point t >= 2, lists in LDS, n_other <= 16 (so
 * that the min-less / min-more result has at most 32 pieces) and n_own <= 32 -- with the
 * specialised operations inlined and not a single call: what the latency build runs for
 * nearly every data point. */
constexpr int FAST_MAX_OTHER = 16, FAST_MAX_OWN = 32;
template <bool HELP>
PSD_D int chain_step_fast(const DeviceArgs &a, ArenaCursor &cur, unsigned long long fn_index,
                          int chain, int t, const LdsList &other_prev, int n_other,
                          const LdsList &own_prev, int n_own, const LdsList &own_new,
                          const LdsList &mlist, const LdsScratch &sc, double pen_term,
                          double cum_weight_prev, double w, int coverage, double cum_weight) {
  PSD_ASSUME(n_other <= FAST_MAX_OTHER && n_own <= FAST_MAX_OWN);
  int nm;
  MathFast mth; /* exp / log without their rare-argument branches; one test at the end */
  if (chain == 0) {
    nm = min_less_impl<true>(other_prev, n_other, mlist, LDS_CAP, sc, t - 1, pen_term, mth);
  } else {
    nm = min_more_impl<true>(other_prev, n_other, mlist, LDS_CAP, sc, t - 1, mth);
  }
  /* (an error may itself be the consequence of a rare argument's unspecified value: the
   * general path decides) */
  if (nm < 0) return ballot(mth.rare != 0) ? -WERR_SERIAL : nm;
  if (nm > 32) return -WERR_OVERFLOW; /* cannot happen: at most 2 pieces per input piece */
  const LdsList f1 = chain == 0 ? mlist : mlist.shifted(LDS_CAP - nm);
  int n_new = min_env_impl<HELP, true>(f1, nm, own_prev, n_own, own_new, LDS_CAP, sc, chain, mth);
  if (ballot(mth.rare != 0)) return -WERR_SERIAL; /* the general path redoes the data point */
  if (n_new < 0) return n_new;
  return step_tail(a, cur, fn_index, own_new, n_new, cum_weight_prev, w, coverage, cum_weight);
}

/* Move one list between LDS and the problem's slot p of the HBM spill pool (cold: only when a
 * function outgrows LDS or has shrunk again). */
PSD_COLD_DEV void move_list_hbm(const DeviceArgs &a, int p, int id, int n, int to_hbm) {
  p = uniform_i(p);
  id = uniform_i(id);
  n = uniform_i(n);
  if (uniform_i(to_hbm)) {
    copy_list_wave(lds_list(id), n, global_list(a, p, id));
  } else {
    copy_list_wave(global_list(a, p, id), n, lds_list(id));
  }
}

/* The general LDS step as one out-of-line function (latency build: data point 1 and functions
 * longer than chain_step_fast takes). */
template <bool HELP>
PSD_COLD_DEV int chain_step_lds(const DeviceArgs &a, ArenaCursor &cur, unsigned long long fn_index,
                                int chain, int t, int id_other_prev, int n_other, int id_own_prev,
                                int n_own, int id_own_new, double pen_term, double cum_weight_prev,
                                double w, int coverage, double cum_weight) {
  chain = uniform_i(chain);
  t = uniform_i(t);
  LdsScratch lsc;
  lsc.w = chain;
  return chain_step<HELP>(a, cur, fn_index, chain, t, lds_list(uniform_i(id_other_prev)),
                          uniform_i(n_other), lds_list(uniform_i(id_own_prev)), uniform_i(n_own),
                          lds_list(uniform_i(id_own_new)), lds_list(4 + chain), lsc,
                          uniform_d(pen_term), uniform_d(cum_weight_prev), uniform_d(w),
                          uniform_i(coverage), uniform_d(cum_weight));
}

/* Data point 0 (cold, once per problem): C^down_1 = gamma_1 / w_1 (drv:266-270), stored
 * unscaled (drv:391); there is no up function yet.  Returns the piece count of the chain's
 * function or -WERR_ARENA. */
PSD_COLD_DEV int first_point(const DeviceArgs &a, ArenaCursor &cur, unsigned long long fn0,
                             int chain, int contig, int coverage, int id_own_new) {
  chain = uniform_i(chain);
  if (chain != 1) return 0;
  const LdsList own_new = lds_list(uniform_i(id_own_new));
  contig = uniform_i(contig);
  if (lane_id() == 0) {
    Coef c;
    c.Linear = 1.0;
    c.Log = (double)(-uniform_i(coverage));
    c.Constant = 0.0;
    store_piece(own_new, 0, c, a.contig_min_log_mean[contig], a.contig_max_log_mean[contig], -1,
                -5.0);
  }
  wave_sync();
  return arena_store_wave(a, cur, own_new, 1, fn0) ? 1 : -WERR_ARENA;
}

#ifdef PSD_HELPER_WAVES
/* Lists in HBM, latency build: the chain wave and its helper wave share the chunks of the
 * three parallel phases of a step (fpop_lds.h, HOP_HBM_*; fpop_coop.h): functions of adversarial
 * data have hundreds of pieces, i.e. more than one wave's worth of lanes of work per phase
 * (7.33 -> 6.24 s on 1e5 increasing counts,
 * profiles/r03/ab_hbm_cooperative_helper_config5_1e5.log; sending only the larger roots to the
 * helper, as the envelope in LDS does, made it 7.3 -> 10.6 s, profiles/r02/ab_step_barrier.log). */
PSD_COLD_DEV void helper_hbm_op(const DeviceArgs &a, int chain, int op) {
  chain = uniform_i(chain);
  op = uniform_i(op);
  Mail &m = g_sm.mail[chain];
  const int p = uniform_i(m.h_arg[0]);
  const GlobalScratch s = global_scratch(a, p, chain);
  if (op == HOP_HBM_COSTS) {
    LanePiece P;
    lane_piece_clear(P);
    MathFull mth;
    piece_costs_wave(global_list(a, p, uniform_i(m.h_arg[1])), uniform_i(m.h_arg[2]), s, P, mth, 1, 2);
  } else {
    const GlobalList f1 = global_list(a, p, uniform_i(m.h_arg[1])).shifted(uniform_i(m.h_arg[2]));
    const int n1 = uniform_i(m.h_arg[3]);
    const GlobalList f2 = global_list(a, p, uniform_i(m.h_arg[4]));
    const int n2 = uniform_i(m.h_arg[5]);
    if (op == HOP_HBM_TABLE) {
      const ldouble *staged = nullptr;
      if (n1 + n2 <= COOP_STAGE_DOUBLES) { /* the ends of f1 behind the chain wave's copy of f2's */
        ldouble *dst = coop_stage(chain) + n2;
        coop_stage_ends(f1, n1, dst);
        staged = dst;
      }
      env_table_second(f1, n1, f2, n2, s, staged);
    } else if (op == HOP_HBM_CLASSIFY) {
      env_coop_helper(f1, n1, f2, n2, s, uniform_i(m.h_arg[6]), chain);
    }
  }
}
PSD_NOINLINE int min_less_coop_wave(GlobalList in, int n, GlobalList out, int cap, GlobalScratch s,
                                    int data_i_out, double add_const, int chain, int p, int id) {
  MathFull mth;
  return min_less_impl<false, true>(in, n, out, cap, s, data_i_out, add_const, mth, chain, p, id);
}
PSD_NOINLINE int min_more_coop_wave(GlobalList in, int n, GlobalList out, int cap, GlobalScratch s,
                                    int data_i_out, int chain, int p, int id) {
  MathFull mth;
  return min_more_impl<false, true>(in, n, out, cap, s, data_i_out, mth, chain, p, id);
}
PSD_NOINLINE int min_env_coop_wave(GlobalList f1, int n1, GlobalList f2, int n2, GlobalList out,
                                   int cap, GlobalScratch s, int chain, int p, int id1, int off1,
                                   int id2) {
  return min_env_coop(f1, n1, f2, n2, out, cap, s, chain, p, id1, off1, id2);
}
PSD_COLD_DEV int chain_step_hbm(const DeviceArgs &a, ArenaCursor &cur,
                                unsigned long long fn_index, int p, int chain, int t,
                                int id_other_prev, int n_other, int id_own_prev, int n_own,
                                int id_own_new, double pen_term, double cum_weight_prev, double w,
                                int coverage, double cum_weight) {
  p = uniform_i(p);
  chain = uniform_i(chain);
  t = uniform_i(t);
  id_other_prev = uniform_i(id_other_prev);
  id_own_prev = uniform_i(id_own_prev);
  n_other = uniform_i(n_other);
  n_own = uniform_i(n_own);
  pen_term = uniform_d(pen_term);
  const int cap = a.spill_cap;
  const GlobalList other_prev = global_list(a, p, id_other_prev);
  const GlobalList own_prev = global_list(a, p, id_own_prev);
  const GlobalList own_new = global_list(a, p, uniform_i(id_own_new));
  const GlobalList mlist = global_list(a, p, 4 + chain);
  const GlobalScratch sc = global_scratch(a, p, chain);
  return chain_step_ops(
      a, cur, fn_index, chain, t, own_prev, n_own, own_new, mlist, uniform_d(cum_weight_prev),
      uniform_d(w), uniform_i(coverage), uniform_d(cum_weight),
      [&]() {
        return min_less_coop_wave(other_prev, n_other, mlist, cap, sc, t - 1, pen_term, chain, p,
                                  id_other_prev);
      },
      [&]() {
        return min_more_coop_wave(other_prev, n_other, mlist, cap, sc, t - 1, chain, p,
                                  id_other_prev);
      },
      [&](int nm) {
        const int off1 = chain == 0 ? 0 : cap - nm;
        return min_env_coop_wave(mlist.shifted(off1), nm, own_prev, n_own, own_new, cap, sc, chain,
                                 p, 4 + chain, off1, id_own_prev);
      });
}
#else
/* The same step with every list in the HBM spill area (functions that outgrew LDS): a cold,
 * out-of-line function, so that its addressing does not hold registers in the kernel's loop. */
PSD_COLD_DEV int chain_step_hbm(const DeviceArgs &a, ArenaCursor &cur,
                                unsigned long long fn_index, int p, int chain, int t,
                                int id_other_prev, int n_other, int id_own_prev, int n_own,
                                int id_own_new, double pen_term, double cum_weight_prev, double w,
                                int coverage, double cum_weight) {
  p = uniform_i(p);
  chain = uniform_i(chain);
  t = uniform_i(t);
  return chain_step<false>(a, cur, fn_index, chain, t,
                           global_list(a, p, uniform_i(id_other_prev)), uniform_i(n_other),
                           global_list(a, p, uniform_i(id_own_prev)), uniform_i(n_own),
                           global_list(a, p, uniform_i(id_own_new)), global_list(a, p, 4 + chain),
                           global_scratch(a, p, chain), uniform_d(pen_term),
                           uniform_d(cum_weight_prev), uniform_d(w), uniform_i(coverage),
                           uniform_d(cum_weight));
}
#endif

}  // namespace PSD_VARIANT
}  // namespace psd
