/* fpop_coop.h -- the helper wave's side, and two waves on one function in HBM.
 *
 * What a helper wave runs (helper_loop: the larger roots of an envelope in LDS, its share of an
 * operation on lists in HBM) and the cooperative envelope of two functions in HBM, min_env_coop:
 * who takes which chunk and how the results cross; the parts are those of fpop_envelope.h.
 * Everything here exists only in builds with PSD_HELPER_WAVES.
 *
 * Reached only through fpop_wave.h: no include guard, compiled once per build variant into
 * namespace psd::PSD_VARIANT. */
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace psd {
namespace PSD_VARIANT {

#ifdef PSD_HELPER_WAVES
/* HOP_ROOT: the larger roots of the lanes flagged by the chain wave.  Returns nonzero in a lane
 * that met a rare exp / log argument (NB only). */
template <bool NB>
PSD_D int helper_root_lanes(Mail &m, int lane) {
  StepMath<NB> mth;
  if (m.flags[lane] & 1) {
    const Coef d = {m.d_lin[lane], m.d_log[lane], m.d_con[lane]};
    /* the optimum of the difference piece exactly as env_classify_lanes derives it */
    PieceOpt o;
    o.mean = psd_div(-d.Log, d.Linear); /* (as env_classify_lanes: the same quotient) */
    o.log_mean = mth.log(o.mean);
    o.cost = mth.cost(d, o.log_mean);
    double loss_without_log_term = d.Linear * o.mean + d.Constant;
    o.cost2 = loss_without_log_term + o.log_mean * d.Log;
    const double b = m.b[lane];
    double root = PSD_INF;
    /* NaN as the right-end cost disables the early exit: the main wave applies it */
    if (has_two_roots(d, o, 0.0))
      root = get_larger_root(d, o, b, __builtin_nan(""), 0.0, nullptr, mth.rare_out());
    m.res_large[lane] = root;
  }
  return mth.rare;
}

/* the helper's share of an operation on lists in HBM (fpop_step.h) */
PSD_COLD_DEV void helper_hbm_op(const DeviceArgs &a, int chain, int op);
/* Body of a helper wave: serve the main wave of `chain` until HOP_EXIT. */
PSD_D void helper_loop(int chain, const DeviceArgs &a) {
  Mail &m = g_sm.mail[chain];
  const int lane = lane_id();
  int seen = 0;
  for (;;) {
    int cmd = seen;
    for (int spin = 0;; spin++) {
      cmd = flag_load(&m.seq_cmd);
      if (cmd != seen) break; /* (not a wait FOR a wave at work: the helper idles here) */
      if (spin > MAIL_SPIN_LIMIT || flag_load(&m.abort)) return;
      spin_pause();
    }
    seen = cmd;
    const int op = uniform_i(m.op);
    if (op == HOP_EXIT) return;
    if (op == HOP_BARRIER) {
      __syncthreads();
    } else if (op == HOP_ROOT) {
      /* without the rare-argument branches first; the complete functions if one was met */
      if (ballot(helper_root_lanes<true>(m, lane) != 0)) (void)helper_root_lanes<false>(m, lane);
    } else if (op >= HOP_HBM_COSTS) {
      helper_hbm_op(*a.self, chain, op);
    }
    wave_sync();
    if (lane == 0) flag_store(&m.seq_done, seen);
    }
}

/* ---- the envelope of two functions in HBM, by the chain wave and its helper ----------------
 * Functions of hundreds of pieces (adversarial data) are processed in chunks of 64 merged
 * intervals; the chunks are independent up to the compaction, which needs the number of
 * pieces emitted so far.  The helper wave classifies the odd chunks and leaves its results
 * (shape, first source, the two crossings, error bits) in HBM; the chain wave classifies the
 * even chunks and compacts all chunks in order, reading the helper's results as they come.
 * Table, classification and compaction are the code of min_env_impl (fpop_envelope.h): same
 * lists, bit for bit. */

/* With the lists in HBM the LDS-resident lists are dead storage: the ends (max_log_mean) of
 * the function a wave ranks against are staged there, so that the binary search of every lane
 * (ten to fifteen dependent reads) runs at LDS instead of L2 latency.  Chain c owns the storage
 * of lists 3c..3c+2, the chain wave the first part (the ends of f2), its helper the rest (the
 * ends of f1); functions too long for it are searched in HBM as before. */
constexpr int COOP_STAGE_DOUBLES = 3 * (int)(sizeof(ListStore) / sizeof(double));
PSD_D ldouble *coop_stage(int chain) { return (ldouble *)&g_sm.list[3 * chain]; }
template <class L>
PSD_D void coop_stage_ends(const L &f, int n, ldouble *dst) {
  for (int i = lane_id(); i < n; i += WAVE) dst[i] = f.mx(i);
  wave_sync();
}
/* one chunk of merged intervals, by either wave: everything up to the candidates */
template <class L, class S>
PSD_D void env_coop_classify(const L &f1, int n1, const L &f2, int n2, const S &s, int K, int base,
                             int chain, EnvLane &e) {
  const int k = base + lane_id();
  const bool valid = k < K;
  env_lane_load(f1, n1, f2, n2, s, k, valid, e);
  bool sl = false, sr = false;
  env_neighbour_flags(f1, f2, s, k, K, valid, valid && same_funs(e.c1, e.c2), sl, sr);
  MathFull mth;
  env_classify_lanes<false>(valid && e.err == 0, e.c1, e.c2, e.ia, e.ib, sl, sr, e.cd, chain, e.err,
                            mth);
}

/* Which chunks of merged intervals the helper classifies: all but every PSD_COOP_PERIOD-th.
 * The chain wave also compacts every chunk (and re-reads the pieces of the helper's chunks for
 * that); measured shares from 3/5 to all: profiles/r03/ab_hbm_helper_share_and_stealing.log. */
#ifndef PSD_COOP_PERIOD
#define PSD_COOP_PERIOD 4
#endif
PSD_D bool coop_helper_owns(int chunk) { return chunk % PSD_COOP_PERIOD != 0; }
/* helper-owned chunks among chunks 0..chunk */
PSD_D int coop_helper_chunks_upto(int chunk) {
  return (chunk / PSD_COOP_PERIOD) * (PSD_COOP_PERIOD - 1) + chunk % PSD_COOP_PERIOD;
}
/* the helper's share: its chunks, results to HBM, progress published chunk by chunk */
template <class L, class S>
PSD_D void env_coop_helper(const L &f1, int n1, const L &f2, int n2, const S &s, int K, int chain) {
  Mail &m = g_sm.mail[chain];
  int done = 0;
  for (int base = 0, chunk = 0; base < K; base += WAVE, chunk++) {
    if (!coop_helper_owns(chunk)) continue;
    EnvLane e;
    env_coop_classify(f1, n1, f2, n2, s, K, base, chain, e);
    const int k = base + lane_id();
    if (k < K) {
      s.coop_x1(k) = e.cd.x1;
      s.coop_x2(k) = e.cd.x2;
      s.coop_code(k) = (double)(e.cd.n | (e.cd.first << 2) | (e.err << 3));
    }
    done++;
    wave_sync();
    if (lane_id() == 0) flag_store(&m.h_progress, done);
  }
}

/* the chain wave: table (with the helper), its own chunks, and the compaction of all */
template <class L, class S>
PSD_D int min_env_coop(L f1_, int n1_, L f2_, int n2_, L out_, int cap_, S s_, int chain_, int p_,
                       int id1_, int off1_, int id2_) {
  const int chain = uniform_i(chain_);
  const L f1 = f1_.uniformed(), f2 = f2_.uniformed(), out = out_.uniformed();
  const S s = s_.uniformed();
  const int n1 = uniform_i(n1_), n2 = uniform_i(n2_), cap = uniform_i(cap_);
  const int lane = lane_id();
  const int iv_cap = s.iv_cap();
  Mail &m = g_sm.mail[chain];
  PSD_PROF_T0();
  if (lane == 0) {
    m.h_arg[0] = p_;
    m.h_arg[1] = id1_;
    m.h_arg[2] = off1_;
    m.h_arg[3] = n1;
    m.h_arg[4] = id2_;
    m.h_arg[5] = n2;
  }
  mail_post(chain, HOP_HBM_TABLE);
  const ldouble *staged = nullptr;
  if (n1 + n2 <= COOP_STAGE_DOUBLES) { /* (the helper makes the same test) */
    ldouble *dst = coop_stage(chain);
    coop_stage_ends(f2, n2, dst);
    staged = dst;
  }
  const int dup_total = env_table_first(f1, n1, f2, n2, s, staged);
  if (!mail_wait(chain)) return -WERR_HELPER;
  const int K = n1 + n2 - dup_total;
  if (K > iv_cap || n1 > SPILL_CAP_MAX || n2 > SPILL_CAP_MAX) return -WERR_OVERFLOW;
  wave_sync();
  PSD_PROF_ADD(PROF_TABLE);
  if (lane == 0) {
    m.h_arg[6] = K;
    flag_store(&m.h_progress, 0);
  }
  mail_post(chain, HOP_HBM_CLASSIFY);

  int n_out = 0, last_id = -1;
  int status = 0;
  for (int base = 0, chunk = 0; base < K; base += WAVE, chunk++) {
    const int k = base + lane;
    const bool valid = k < K;
    EnvLane e;
    PSD_PROF_T0();
    if (!coop_helper_owns(chunk)) {
      env_coop_classify(f1, n1, f2, n2, s, K, base, chain, e);
    } else {
      /* the helper's chunk: wait for it, then fetch its results and the pieces they refer to */
      const int want = coop_helper_chunks_upto(chunk);
      bool there = false;
      for (int spin = 0; spin < MAIL_SPIN_LIMIT; spin++) {
        if (rdlane_i(flag_load(&m.h_progress), 0) >= want) {
          there = true;
          PSD_SPIN_NOTE(spin);
          break;
        }
        spin_pause();
      }
      if (!there) {
        status = -WERR_HELPER;
        break;
      }
      env_lane_load(f1, n1, f2, n2, s, k, valid, e);
      if (valid) {
        const int code = (int)s.coop_code(k);
        e.cd.n = code & 3;
        e.cd.first = (code >> 2) & 1;
        e.err |= code >> 3;
        e.cd.x1 = s.coop_x1(k);
        e.cd.x2 = s.coop_x2(k);
      }
    }
    PSD_PROF_ADD(PROF_CLASSIFY);
    status = env_compact_chunk(f1, f2, out, cap, valid, e, n_out, last_id);
    PSD_PROF_ADD(PROF_COMPACT);
    /* (where min_env_impl may return, this wave goes on to wait for its helper) */
    if (status < 0) break;
  }
  /* the helper finishes its chunks whatever happened here (they are bounded work) */
  if (!mail_wait(chain)) return -WERR_HELPER;
  if (status < 0 && status != -WERR_SERIAL) return status;
#ifdef PSD_FORCE_SERIAL_ENV
  status = -WERR_SERIAL;
#endif
  if (status == -WERR_SERIAL) {
    if (lane == 0) g_sm.serial[wave_id()]++;
    n_out = min_env_serial(f1, n1, f2, n2, out, cap, s, K);
  }
  return n_out;
}
#endif /* PSD_HELPER_WAVES */

}  // namespace PSD_VARIANT
}  // namespace psd
