/* fpop_coop.h -- the helper wave's side, and two waves on one function in HBM.
 *
 * What a helper wave runs (helper_loop: the larger roots of an envelope in LDS, its share of an
 * operation on lists in HBM) and the cooperative envelope of two functions in HBM, min_env_coop.
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
 * The arithmetic per interval is that of min_env_impl: same lists, bit for bit. */

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
/* number of entries of the sorted array a[0..n) below x */
PSD_D int rank_staged(const ldouble *a, int n, double x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (a[mid] < x) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo;
}

/* merged-interval table, the entries owned by f1 (every end of f1); returns how many ends of
 * f1 are also ends of f2.  staged: the ends of f2 in LDS (or nullptr) */
template <class L, class S>
PSD_D int env_table_first(const L &f1, int n1, const L &f2, int n2, const S &s,
                          const ldouble *staged) {
  const int lane = lane_id();
  const int iv_cap = s.iv_cap();
  int dup_before = 0;
  for (int base = 0; base < n1; base += WAVE) {
    int i = base + lane;
    bool valid = i < n1;
    int p = 0;
    bool dup = false;
    if (valid) {
      double x = f1.mx(i);
      if (staged) {
        p = rank_staged(staged, n2, x);
        dup = p < n2 && staged[p] == x;
      } else {
        p = rank_mx(f2, n2, x);
        dup = p < n2 && f2.mx(p) == x;
      }
    }
    unsigned long long md = ballot(dup);
    if (valid) {
      int k = i + p - (dup_before + popc64(md & lanes_below(lane)));
      if (k < iv_cap) s.iv(k) = (i << 16) | p;
    }
    dup_before += popc64(md);
  }
  return dup_before;
}
/* ... and the entries owned by f2 (its ends that are not ends of f1); staged: the ends of f1 */
template <class L, class S>
PSD_D void env_table_second(const L &f1, int n1, const L &f2, int n2, const S &s,
                            const ldouble *staged) {
  const int lane = lane_id();
  const int iv_cap = s.iv_cap();
  int dup_before = 0;
  for (int base = 0; base < n2; base += WAVE) {
    int j = base + lane;
    bool valid = j < n2;
    int q = 0;
    bool dup = false;
    if (valid) {
      double x = f2.mx(j);
      if (staged) {
        q = rank_staged(staged, n1, x);
        dup = q < n1 && staged[q] == x;
      } else {
        q = rank_mx(f1, n1, x);
        dup = q < n1 && f1.mx(q) == x;
      }
    }
    unsigned long long md = ballot(dup);
    if (valid && !dup) {
      int k = j + q - (dup_before + popc64(md & lanes_below(lane)));
      if (k < iv_cap) s.iv(k) = (q << 16) | j;
    }
    dup_before += popc64(md);
  }
}

/* one chunk of merged intervals: everything up to the candidates (the first half of the chunk
 * loop of min_env_impl) */
struct EnvLane {
  Cands cd;
  double ia, ib;
  Coef c1, c2;
  double prv1, prv2;
  int di1, di2, i1, i2;
  int err;
};
template <class L, class S>
PSD_D void env_coop_load(const L &f1, int n1, const L &f2, int n2, const S &s, int k, bool valid,
                         EnvLane &e) {
  e.cd.n = 0;
  e.cd.first = 0;
  e.cd.x1 = e.cd.x2 = 0.0;
  e.ia = e.ib = 0.0;
  e.c1.Linear = e.c1.Log = e.c1.Constant = 0.0;
  e.c2 = e.c1;
  e.prv1 = e.prv2 = 0.0;
  e.di1 = e.di2 = e.i1 = e.i2 = 0;
  e.err = 0;
  if (valid) {
    int en = s.iv(k);
    e.i1 = en >> 16;
    e.i2 = en & 0xffff;
    env_load_interval(f1, n1, f2, n2, e.i1, e.i2, e.c1, e.c2, e.ia, e.ib, e.err);
    e.prv1 = f1.prv(e.i1);
    e.di1 = f1.di(e.i1);
    e.prv2 = f2.prv(e.i2);
    e.di2 = f2.di(e.i2);
  }
}
template <class L, class S>
PSD_D void env_coop_classify(const L &f1, int n1, const L &f2, int n2, const S &s, int K, int base,
                             int chain, EnvLane &e) {
  const int k = base + lane_id();
  const bool valid = k < K;
  env_coop_load(f1, n1, f2, n2, s, k, valid, e);
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

  int n_out = 0;
  int err = 0;
  bool need_serial = false, overflow = false, helper_lost = false;
  int last_id = -1;
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
        helper_lost = true;
        break;
      }
      env_coop_load(f1, n1, f2, n2, s, k, valid, e);
      if (valid) {
        const int code = (int)s.coop_code(k);
        e.cd.n = code & 3;
        e.cd.first = (code >> 2) & 1;
        e.err |= code >> 3;
        e.cd.x1 = s.coop_x1(k);
        e.cd.x2 = s.coop_x2(k);
      }
    }
    err = e.err;
    PSD_PROF_ADD(PROF_CLASSIFY);
    /* ---- compaction: as in min_env_impl ---- */
    const Cands &cd = e.cd;
    const int src0 = cd.first, src1 = cd.first ^ 1;
    Coef fc = src0 ? e.c2 : e.c1;
    double fprv = src0 ? e.prv2 : e.prv1;
    int fdi = src0 ? e.di2 : e.di1;
    int lsrc = cd.n == 2 ? src1 : src0;
    const double hi0 = cd.n == 1 ? e.ib : cd.x1;
    const double hi1 = cd.n == 2 ? e.ib : cd.x2;
    bool has = valid && cd.n > 0;
    unsigned long long m_has = ballot(has);
    unsigned long long m_err = ballot(err != 0);
    if (m_err) {
      int eb = 0;
      for (int l = 0; l < WAVE; l++) eb |= shfl_i(err, l);
      err = eb;
      break;
    }
    unsigned long long lb = lanes_below(lane);
    unsigned long long below = m_has & lb;
    const int my_last_id = (lsrc << 20) | (lsrc ? e.i2 : e.i1);
    int pid = shfl_i(my_last_id, below ? msb64(below) : 0);
    if (!below) pid = last_id;
    const bool have_pred = pid >= 0;
    Coef pc = {0.0, 0.0, 0.0};
    double pprv = 0.0;
    int pdi = 0;
    if (has && have_pred) {
      const L &pl = (pid >> 20) ? f2 : f1;
      const int pi = pid & 0xfffff;
      pc = load_coef(pl, pi);
      pprv = pl.prv(pi);
      pdi = pl.di(pi);
    }
    bool head0 = true;
    bool fuzzy = false;
    if (has && have_pred) {
      bool co = coalesces(pc, pprv, pdi, fc, fprv, fdi);
      bool bi = bit_identical(pc, pprv, pdi, fc, fprv, fdi);
      head0 = !co;
      fuzzy = co && !bi;
    }
    if (ballot(fuzzy)) {
      need_serial = true;
      break;
    }
    int heads = has ? ((head0 ? 1 : 0) + (cd.n - 1)) : 0;
    unsigned long long hb0 = ballot((heads & 1) != 0);
    unsigned long long hb1 = ballot((heads & 2) != 0);
    int heads_before = popc64(hb0 & lb) + 2 * popc64(hb1 & lb);
    int heads_total = popc64(hb0) + 2 * popc64(hb1);
    if (n_out + heads_total > cap) {
      overflow = true;
      break;
    }
    int slot = n_out + heads_before - (head0 ? 0 : 1);
    if (has) {
      if (head0) store_piece(out, slot, fc, e.ia, hi0, fdi, fprv);
      if (cd.n >= 2) {
        Coef c = src1 ? e.c2 : e.c1;
        store_piece(out, slot + 1, c, cd.x1, hi1, src1 ? e.di2 : e.di1, src1 ? e.prv2 : e.prv1);
      }
      if (cd.n >= 3) store_piece(out, slot + 2, fc, cd.x2, e.ib, fdi, fprv);
    }
    wave_sync();
    {
      unsigned long long m_head0 = ballot(has && head0);
      if (has && !head0) {
        unsigned long long above = m_has & ~lb & ~(1ull << lane);
        bool next_is_head = true;
        if (above) next_is_head = ((m_head0 >> ctz64(above)) & 1ull) != 0;
        if (cd.n >= 2 || next_is_head) out.mx(slot) = hi0;
      }
    }
    wave_sync();
    n_out += heads_total;
    if (m_has) last_id = rdlane_i(my_last_id, msb64(m_has));
    PSD_PROF_ADD(PROF_COMPACT);
  }
  /* the helper finishes its chunks whatever happened here (they are bounded work) */
  if (!mail_wait(chain) || helper_lost) return -WERR_HELPER;
  if (err) return -err;
  if (overflow) return -WERR_OVERFLOW;
#ifdef PSD_FORCE_SERIAL_ENV
  need_serial = true;
#endif
  if (need_serial) {
    if (lane == 0) g_sm.serial[wave_id()]++;
    n_out = min_env_serial(f1, n1, f2, n2, out, cap, s, K);
  }
  return n_out;
}
#endif /* PSD_HELPER_WAVES */

}  // namespace PSD_VARIANT
}  // namespace psd
