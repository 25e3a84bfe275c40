/* fpop_walks.h -- min-less and min-more: the two walks over one function's pieces.
 *
 * The classes and error bits, the speculation window, the first pass (per piece: end costs,
 * optimum, what the walk does with it) and the two walks themselves, min_less_impl and
 * min_more_impl (fpop_wave.h describes the design).
 *
 * Reached only through fpop_wave.h: no include guard, compiled once per build variant into
 * namespace psd::PSD_VARIANT. */
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace psd {
namespace PSD_VARIANT {

enum { CLS_STORE = 0, CLS_CONST_EDGE = 1, CLS_CONST_MU = 2 };

/* how many pieces after (before) a constant's start the all-pairs speculation of min_less
 * (min_more) covers; the rest is scanned only if no crossing was found among them */
#ifndef PSD_SPEC_WINDOW
#define PSD_SPEC_WINDOW 5
#endif
constexpr int SPEC_WINDOW = PSD_SPEC_WINDOW;
/* ... and for functions of 13 to 16 pieces (whose starts times SPEC_WINDOW no longer fit the 64
 * lanes): one piece fewer per start keeps the direct lane -> (start, piece) mapping instead of a
 * loop over the starts, which cost the min-more wave of the large-penalty problems -- the
 * slowest of a grid -- 3 % of its data point (2124 -> 2101 ms on 200 k bins x 64,
 * profiles/r04/ab_adaptive_speculation_window.log).  Speculation only decides what is solved
 * ahead of the walk, never a result. */
constexpr int SPEC_WINDOW_NARROW = 4;

/* error bits (the reference would throw / loop / read a sentinel) */
enum {
  WERR_OVERFLOW = 1,      /* output does not fit `cap` */
  WERR_REF_THROW = 2,     /* fpl:380 decreasing degenerate linear piece */
  WERR_SENTINEL = 4,      /* push_min_pieces neighbour outside the list */
  WERR_ZERO_INTERVAL = 8, /* fpl:933 zero-size merged interval */
  WERR_ARENA = 16,        /* the in-HBM store is full */
  WERR_HELPER = 32,       /* a helper wave did not answer (never expected) */
  WERR_SERIAL = 64,       /* specialised min_env only: the step needs the sequential replay */
};

/* A lane's own copy of piece `lane` and of what the first pass computed for it (functions of
 * at most 64 pieces): the walk's state machine then reads other pieces with v_readlane
 * instead of dependent LDS round trips. */
struct LanePiece {
  Coef c;
  double mn, mx;
  double lc, rc;   /* getCost at the left / right end */
  double om, mu;   /* argmin_mean(), argmin() */
  double muc, oc2; /* getCost(argmin()), PoissonLoss(argmin_mean()) */
  int cls;
};
PSD_D void lane_piece_clear(LanePiece &P) {
  P.c.Linear = P.c.Log = P.c.Constant = 0.0;
  P.mn = P.mx = P.lc = P.rc = P.om = P.mu = P.muc = P.oc2 = 0.0;
  P.cls = CLS_STORE;
}

/* Shared first half of min-less / min-more: per piece, the costs at both ends and the
 * optimum (fpl:245-246,310-311 / 469-470,483-485); kept in scratch for every piece and in
 * registers for piece `lane`. */
template <class L, class S, class M>
PSD_D void piece_costs_wave(const L &in, int n, const S &s, LanePiece &P, M &mth, int chunk0 = 0,
                            int stride = 1) {
  const int lane = lane_id();
  /* chunks chunk0, chunk0 + stride, ...: two waves share a long function (HOP_HBM_COSTS) */
  for (int base = chunk0 * WAVE; base < n; base += stride * WAVE) {
    int i = base + lane;
    if (i < n) {
      Coef c = load_coef(in, i);
      double mn = in.mn(i), mx = in.mx(i);
      /* exp(mn), exp(mx) and log(argmin_mean) do not depend on one another: one interleaved
       * evaluation (peakseg_detmath_core.h, psd_exp2_log) instead of three in a row; the values
       * are those of get_cost() and piece_opt() (paired against single evaluations: 1172 ->
       * 1163 ms on 100 k bins x 64, profiles/r02/ab_paired_transcendentals.log) */
      const bool has_opt = c.Log != 0;
      PieceOpt o = {0.0, 0.0, 0.0, 0.0};
      if (has_opt) o.mean = argmin_mean(c);
      double e_mn, e_mx, l_om;
      mth.exp2_log(mn == -PSD_INF ? 0.0 : mn, mx == -PSD_INF ? 0.0 : mx, has_opt ? o.mean : 1.0,
                   e_mn, e_mx, l_om);
      double lc = get_cost_e(c, mn, e_mn);
      double rc = get_cost_e(c, mx, e_mx);
      if (has_opt) {
        o.log_mean = l_om;
        o.cost = mth.cost(c, o.log_mean);
        double loss_without_log_term = c.Linear * o.mean + c.Constant; /* fpl:52-61 */
        o.cost2 = loss_without_log_term + o.log_mean * c.Log;
      }
      s.lc(i) = lc;
      s.rc(i) = rc;
      s.om(i) = o.mean;
      s.mu(i) = o.log_mean;
      s.muc(i) = o.cost;
      s.oc2(i) = o.cost2;
      if (base == 0) {
        P.c = c;
        P.mn = mn;
        P.mx = mx;
        P.lc = lc;
        P.rc = rc;
        P.om = o.mean;
        P.mu = o.log_mean;
        P.muc = o.cost;
        P.oc2 = o.cost2;
      }
    }
  }
  wave_sync();
}

/* First pass of min-less: per piece the end costs and optimum (piece_costs_wave) and what the
 * walk does with the piece when it reaches it in search mode. */
#ifdef PSD_HELPER_WAVES
/* The costs of a function in HBM by two waves: the helper takes the odd chunks. */
template <class L, class S>
PSD_D bool coop_piece_costs(const L &in, int n, const S &s, LanePiece &P, int chain, int p, int id) {
  Mail &m = g_sm.mail[chain];
  if (lane_id() == 0) {
    m.h_arg[0] = p;
    m.h_arg[1] = id;
    m.h_arg[2] = n;
  }
  mail_post(chain, HOP_HBM_COSTS);
  MathFull mth;
  piece_costs_wave(in, n, s, P, mth, 0, 2);
  return mail_wait(chain);
}
#endif
/* COOP: the function is list coop_id of spill slot coop_p and the chain's helper wave takes
 * half of the chunks (latency build, lists in HBM). */
template <bool COOP = false, class L, class S, class M>
PSD_D bool min_less_pre(const L &in, int n, const S &s, LanePiece &P, M &mth, int coop_chain = 0,
                        int coop_p = 0, int coop_id = 0) {
  const int lane = lane_id();
  bool ok = true;
#ifdef PSD_HELPER_WAVES
  if (COOP) {
    ok = coop_piece_costs(in, n, s, P, coop_chain, coop_p, coop_id);
  } else
#endif
  {
    piece_costs_wave(in, n, s, P, mth);
  }
  /* what the walk does with piece i when it reaches it in search mode */
  for (int base = 0; base < n; base += WAVE) {
    int i = base + lane;
    if (i < n) {
      double Log_i = in.Log(i);
      double lc = s.lc(i), rc = s.rc(i);
      bool has_next = i + 1 < n;
      double next_left_cost = has_next ? s.lc(i + 1) : PSD_INF;
      /* both kinds of piece are classified and one result selected: all reads in one LDS
       * round trip and no exec-masked region per test (a degenerate piece's optimum is stored
       * as zeros) */
      const double mu = s.mu(i), mu_cost = s.muc(i), mn_i = in.mn(i), mx_i = in.mx(i);
      /* fpl:256-308 */
      const bool right_left_equal = rc - lc < NEWTON_EPSILON;
      const bool next_cost_more_than_left = !has_next | (NEWTON_EPSILON < next_left_cost - lc);
      const int cls_flat = (next_cost_more_than_left & !right_left_equal) ? CLS_CONST_EDGE : CLS_STORE;
      /* fpl:309-366 */
      const bool next_ok = !has_next | (NEWTON_EPSILON < next_left_cost - mu_cost);
      const bool cost_ok = (NEWTON_EPSILON < rc - mu_cost) & next_ok;
      int cls_convex = ((mu < mx_i) & cost_ok) ? CLS_CONST_MU : CLS_STORE;
      cls_convex = ((mu <= mn_i) & cost_ok) ? CLS_CONST_EDGE : cls_convex;
      const int cls = (Log_i == 0) ? cls_flat : cls_convex;
      s.cls(i) = cls;
      if (base == 0) P.cls = cls;
    }
  }
  wave_sync();
  return ok;
}

/* First pass of min-more, as min_less_pre. */
template <bool COOP = false, class L, class S, class M>
PSD_D bool min_more_pre(const L &in, int n, const S &s, LanePiece &P, M &mth, int coop_chain = 0,
                        int coop_p = 0, int coop_id = 0) {
  const int lane = lane_id();
  bool ok = true;
#ifdef PSD_HELPER_WAVES
  if (COOP) {
    ok = coop_piece_costs(in, n, s, P, coop_chain, coop_p, coop_id);
  } else
#endif
  {
    piece_costs_wave(in, n, s, P, mth);
  }
  for (int base = 0; base < n; base += WAVE) {
    int i = base + lane;
    if (i < n) {
      /* (selects, all reads in one LDS round trip: as in min_less_pre) */
      const double Log_i = in.Log(i), mu = s.mu(i), mu_cost = s.muc(i);
      const double mn_i = in.mn(i), mx_i = in.mx(i);
      const double this_cost_left = s.lc(i), this_cost_right = s.rc(i);
      const double prev_cost_right = s.rc(i > 0 ? i - 1 : 0);
      /* fpl:468-548 */
      const bool prev_ok = (i <= 0) | (NEWTON_EPSILON < prev_cost_right - mu_cost);
      const int cls_edge = (NEWTON_EPSILON < this_cost_left - this_cost_right) ? CLS_CONST_EDGE : CLS_STORE;
      const bool at_mu = (mn_i < mu) & (NEWTON_EPSILON < this_cost_left - mu_cost) & prev_ok;
      const int cls_convex = (mx_i <= mu) ? cls_edge : (at_mu ? CLS_CONST_MU : CLS_STORE);
      const int cls = (Log_i == 0) ? CLS_STORE : cls_convex; /* fpl:458-467 */
      s.cls(i) = cls;
      if (base == 0) P.cls = cls;
    }
  }
  wave_sync();
  return ok;
}

/* ------------------------------------------------------------------------------------- */
/* min-less: out(x) = min_{y<=x} in(y).  All output pieces get data_i = data_i_out (the
 * driver's set_prev_seg_end) and Constant += add_const (its add(0,0,penalty/cum_weight_prev),
 * PeakSegFPOPLog.cpp:290-296). */
template <bool SMALL, bool COOP = false, class L, class S, class M>
PSD_D int min_less_impl(L in_, int n_, L out_, int cap_, S s_, int data_i_out_,
                        double add_const_, M &mth, int coop_chain = 0, int coop_p = 0,
                        int coop_id = 0) {
  const L in = in_.uniformed(), out = out_.uniformed();
  const S s = s_.uniformed();
  const int n = uniform_i(n_), cap = uniform_i(cap_), data_i_out = uniform_i(data_i_out_);
  const double add_const = uniform_d(add_const_);
  const int lane = lane_id();
  /* lane i holds piece i; SMALL: the caller guarantees n <= WAVE (the other code drops out) */
  if (SMALL) PSD_ASSUME(n <= WAVE);
  const bool small = SMALL || n <= WAVE;
  LanePiece P;
  lane_piece_clear(P);
  PSD_PROF_T0();
  if (!min_less_pre<COOP>(in, n, s, P, mth, coop_chain, coop_p, coop_id)) return -WERR_HELPER;
  PSD_PROF_ADD(PROF_PRE);
  /* uniform reads of piece j: registers of lane j when the function fits one wave */
  auto cls_at = [&](int j) -> int { return small ? rdlane_i(P.cls, j) : s.cls(j); };
  auto mu_at = [&](int j) -> double { return small ? rdlane_d(P.mu, j) : s.mu(j); };
  auto muc_at = [&](int j) -> double { return small ? rdlane_d(P.muc, j) : s.muc(j); };
  auto lc_at = [&](int j) -> double { return small ? rdlane_d(P.lc, j) : s.lc(j); };
  auto mn_at = [&](int j) -> double { return small ? rdlane_d(P.mn, j) : in.mn(j); };
  auto mx_at = [&](int j) -> double { return small ? rdlane_d(P.mx, j) : in.mx(j); };

  int err = 0;
  /* ---- all-pairs speculation ------------------------------------------------------------
   * Where the constant started at piece j ends depends only on j (its level c_j is known from
   * the first pass) and on the pieces after it, not on how the walk got to j.  When all
   * (start j, later piece k) pairs fit in one wave, every pair tests its crossing NOW, in one
   * round of Newton solves, and the walk below only looks results up.  Otherwise each
   * constant scans its remaining pieces when the walk reaches it (one round per constant). */
  bool spec = false;
  unsigned long long sp_ev = 0, sp_inside = 0, sp_bad = 0;
  double sp_mu = PSD_INF;
  int my_base = 0; /* lane j: first task lane of start j */
  int win = SPEC_WINDOW; /* pieces after a start that the speculation covers */
  if (small) {
    unsigned long long m_start = ballot(lane < n && P.cls != CLS_STORE);
    int tj = -1, tk = 0;
    /* the window a start gets: SPEC_WINDOW pieces while n starts of that many fit a wave, one
     * fewer for up to 16 pieces (64 / 4 starts): still a direct lane -> task mapping, no loop
     * over the starts */
    win = (n * SPEC_WINDOW <= WAVE) ? SPEC_WINDOW : ((n * SPEC_WINDOW_NARROW <= WAVE) ? SPEC_WINDOW_NARROW : 0);
    if (win > 0) {
      /* few pieces (the usual case): task lane = start * window + offset, no loop */
      if (m_start) {
        spec = true;
        const int cj = win == SPEC_WINDOW ? lane / SPEC_WINDOW : lane / SPEC_WINDOW_NARROW;
        const int off = lane - cj * win;
        if (cj < n && ((m_start >> cj) & 1ull) && cj + 1 + off < n) {
          tj = cj;
          tk = cj + 1 + off;
        }
        my_base = lane * win;
      }
    } else {
      win = SPEC_WINDOW;
      int total = 0;
      for (unsigned long long m = m_start; m; m &= m - 1) {
        int c = n - 1 - ctz64(m);
        total += c < SPEC_WINDOW ? c : SPEC_WINDOW;
      }
      if (total > 0 && total <= WAVE) {
        spec = true;
        int base = 0;
        for (unsigned long long m = m_start; m; m &= m - 1) {
          int j = ctz64(m), cnt = n - 1 - j;
          if (cnt > SPEC_WINDOW) cnt = SPEC_WINDOW;
          if (lane == j) my_base = base;
          if (lane >= base && lane < base + cnt) {
            tj = j;
            tk = j + 1 + (lane - base);
          }
          base += cnt;
        }
      }
    }
    if (spec) {
      bool inside = false, at_right = false, bad = false;
      int sp_steps = 0;
      /* every lane loads (a lane without a task reads piece 0: harmless), so that all reads
       * share one LDS round trip and the only exec-masked region is the Newton solve */
      const bool task = tj >= 0;
      const int sj = task ? tj : 0;
      const double level = (s.cls(sj) == CLS_CONST_MU) ? s.muc(sj) : s.lc(sj);
      const Coef c = load_coef(in, tk);
      const PieceOpt o = {s.om(tk), s.mu(tk), s.muc(tk), s.oc2(tk)};
      const double t_mn = in.mn(tk), t_mx = in.mx(tk), t_lc = s.lc(tk), t_rc = s.rc(tk);
      const bool convex = task & (c.Log != 0);
      bad = task & (c.Log == 0) & (c.Linear < 0); /* fpl:378-380 */
      if (convex & has_two_roots(c, o, level)) {
        sp_mu = get_smaller_root(c, o, t_mn, t_lc, level, &sp_steps);
        inside = (t_mn < sp_mu) & (sp_mu < t_mx);
      }
      at_right = convex & !inside & (t_rc <= level + NEWTON_EPSILON);
      PSD_PROF_ITERS(PROF_IT_SPEC, sp_steps);
      sp_ev = ballot(inside || at_right);
      sp_inside = ballot(inside);
      sp_bad = ballot(bad);
    }
  }
  PSD_PROF_ADD(PROF_SERIAL); /* diagnostic builds: the speculation round */
  int n_out = 0;
  int i0 = 0;
  double prev_min_log_mean = mn_at(0);
  /* Functions of at most 64 pieces: the walk only RECORDS, in the lane of each input piece,
   * what that piece contributes (first its own kept or partial convex piece, then the
   * constant that starts at it); everything is written in one parallel pass after the
   * walk.  Longer functions write as they go. */
  bool e1 = false, e2 = false;          /* this lane's piece emits a convex / a constant piece */
  double e1_lo = 0.0, e1_hi = 0.0;      /* convex piece: own coefficients on [e1_lo, e1_hi] */
  double e2_lo = 0.0, e2_hi = 0.0, e2_level = 0.0, e2_best = 0.0;
  for (;;) {
    PSD_PROF_COUNT(PROF_IT_ROUNDS);
    /* ---- search mode: first piece j >= i0 that starts a constant ---- */
    int j = n;
    for (int base = i0 & ~(WAVE - 1); base < n; base += WAVE) {
      int i = base + lane;
      int cls_i = small ? P.cls : ((i < n) ? s.cls(i) : CLS_STORE);
      bool hit = i >= i0 && i < n && cls_i != CLS_STORE;
      unsigned long long m = ballot(hit);
      if (m) {
        j = base + ctz64(m);
        break;
      }
    }
    /* pieces i0..j-1 are kept as they are (fpl:303-307,361-364) */
    int cnt = j - i0;
    if (small) {
      if (lane >= i0 && lane < j) {
        e1 = true;
        e1_lo = (lane == i0) ? prev_min_log_mean : P.mn;
        e1_hi = P.mx;
      }
    } else {
      if (n_out + cnt + 2 > cap) return -WERR_OVERFLOW;
      for (int base = i0; base < j; base += WAVE) {
        int i = base + lane;
        if (i < j) {
          Coef c = load_coef(in, i);
          c.Constant = c.Constant + add_const;
          c.Linear = c.Linear + 0.0;
          c.Log = c.Log + 0.0;
          double lo = (i == i0) ? prev_min_log_mean : in.mn(i);
          store_piece(out, n_out + (i - i0), c, lo, in.mx(i), data_i_out, PSD_INF);
        }
      }
      n_out += cnt;
    }
    if (cnt > 0) prev_min_log_mean = mx_at(j - 1);
    if (j == n) break;
    /* ---- piece j starts a constant piece ---- */
    double prev_min_cost, prev_best_log_mean;
    if (cls_at(j) == CLS_CONST_MU) { /* fpl:337-355 */
      double mu = mu_at(j);
      if (prev_min_log_mean < mu) {
        if (small) {
          if (lane == j) {
            e1 = true;
            e1_lo = prev_min_log_mean;
            e1_hi = mu;
          }
        } else {
          if (lane == 0) {
            Coef c = load_coef(in, j);
            c.Constant = c.Constant + add_const;
            c.Linear = c.Linear + 0.0;
            c.Log = c.Log + 0.0;
            store_piece(out, n_out, c, prev_min_log_mean, mu, data_i_out, PSD_INF);
          }
          n_out++;
        }
      }
      prev_min_log_mean = mu;
      prev_best_log_mean = mu;
      prev_min_cost = muc_at(j);
    } else { /* fpl:288-292,328-336 */
      prev_min_cost = lc_at(j);
      prev_best_log_mean = mn_at(j);
    }
    /* ---- constant mode: first piece k > j where the constant ends (fpl:367-422) ---- */
    int k_ev = -1;
    bool ev_inside = false;
    double ev_mu = 0.0;
    int scan_from = j + 1; /* first piece not covered by the speculation */
    if (spec) {
      int cntj = n - 1 - j;
      if (cntj > win) cntj = win;
      scan_from = j + 1 + cntj;
      if (cntj > 0) {
        int base = rdlane_i(my_base, j);
        unsigned long long range = ((1ull << cntj) - 1ull) << base;
        unsigned long long ev = sp_ev & range;
        unsigned long long visited = ev ? (range & lanes_below(ctz64(ev))) : range;
        if (sp_bad & visited) err |= WERR_REF_THROW;
        if (ev) {
          int src = ctz64(ev);
          k_ev = j + 1 + (src - base);
          ev_inside = ((sp_inside >> src) & 1ull) != 0;
          ev_mu = rdlane_d(sp_mu, src);
        }
      }
    }
    if (k_ev < 0) { /* pieces beyond the speculation window: scan them now */
      for (int base = scan_from; base < n; base += WAVE) {
        int k = base + lane;
        bool inside = false, at_right = false, bad = false;
        double mu = PSD_INF;
        if (k < n) {
          Coef c = load_coef(in, k);
          if (c.Log == 0) {
            if (c.Linear < 0) bad = true; /* fpl:378-380 */
          } else {
            /* optimum and end costs of piece k were computed in the first pass */
            PieceOpt o = {s.om(k), s.mu(k), s.muc(k), s.oc2(k)};
            if (has_two_roots(c, o, prev_min_cost)) {
              mu = get_smaller_root(c, o, in.mn(k), s.lc(k), prev_min_cost);
              inside = in.mn(k) < mu && mu < in.mx(k);
            }
            if (!inside) at_right = s.rc(k) <= prev_min_cost + NEWTON_EPSILON;
          }
        }
        unsigned long long m_ev = ballot(inside || at_right);
        unsigned long long m_in = ballot(inside);
        unsigned long long m_bad = ballot(bad);
        unsigned long long visited = m_ev ? lanes_below(ctz64(m_ev)) : ~0ull;
        if (m_bad & visited) err |= WERR_REF_THROW;
        if (m_ev) {
          int src = ctz64(m_ev);
          k_ev = base + src;
          ev_inside = ((m_in >> src) & 1ull) != 0;
          ev_mu = rdlane_d(mu, src);
          break;
        }
      }
    }
    Coef cc;
    cc.Linear = 0.0 + 0.0;
    cc.Log = 0.0 + 0.0;
    cc.Constant = prev_min_cost + add_const;
    /* where the constant ends: the end of the function (fpl:429-436), a crossing inside piece
     * k, which is then revisited in search mode (fpl:397-408), or the right end of piece k
     * (fpl:410-420) */
    double c_hi;
    bool last_round = false;
    if (k_ev < 0) {
      c_hi = mx_at(n - 1);
      last_round = true;
    } else if (ev_inside) {
      c_hi = ev_mu;
      i0 = k_ev;
    } else {
      c_hi = mx_at(k_ev);
      i0 = k_ev + 1;
      if (i0 == n) last_round = true;
    }
    if (small) {
      if (lane == j) {
        e2 = true;
        e2_lo = prev_min_log_mean;
        e2_hi = c_hi;
        e2_level = cc.Constant;
        e2_best = prev_best_log_mean;
      }
    } else {
      if (lane == 0)
        store_piece(out, n_out, cc, prev_min_log_mean, c_hi, data_i_out, prev_best_log_mean);
      n_out++;
    }
    prev_min_log_mean = c_hi;
    if (last_round) break;
  }
  if (small) {
    /* one parallel pass: lane i writes its convex piece, then its constant piece */
    unsigned long long m1 = ballot(e1), m2 = ballot(e2);
    unsigned long long lb = lanes_below(lane);
    n_out = popc64(m1) + popc64(m2);
    if (n_out + 2 > cap) return -WERR_OVERFLOW;
    int pos = popc64(m1 & lb) + popc64(m2 & lb);
    if (e1) {
      Coef c = P.c;
      c.Constant = c.Constant + add_const;
      c.Linear = c.Linear + 0.0;
      c.Log = c.Log + 0.0;
      store_piece(out, pos, c, e1_lo, e1_hi, data_i_out, PSD_INF);
      pos++;
    }
    if (e2) {
      Coef cc;
      cc.Linear = 0.0 + 0.0;
      cc.Log = 0.0 + 0.0;
      cc.Constant = e2_level;
      store_piece(out, pos, cc, e2_lo, e2_hi, data_i_out, e2_best);
    }
  }
  wave_sync();
  PSD_PROF_ADD(PROF_WALK);
  return err ? -err : n_out;
}

/* ------------------------------------------------------------------------------------- */
/* min-more: out(x) = min_{y>=x} in(y).  The reference builds the list with emplace_front;
 * here pieces are written downwards from out[cap-1]: the result is out[cap-n .. cap). */
template <bool SMALL, bool COOP = false, class L, class S, class M>
PSD_D int min_more_impl(L in_, int n_, L out_, int cap_, S s_, int data_i_out_, M &mth,
                        int coop_chain = 0, int coop_p = 0, int coop_id = 0) {
  const L in = in_.uniformed(), out = out_.uniformed();
  const S s = s_.uniformed();
  const int n = uniform_i(n_), cap = uniform_i(cap_), data_i_out = uniform_i(data_i_out_);
  const int lane = lane_id();
  if (SMALL) PSD_ASSUME(n <= WAVE);
  const bool small = SMALL || n <= WAVE;
  LanePiece P;
  lane_piece_clear(P);
  PSD_PROF_T0();
  if (!min_more_pre<COOP>(in, n, s, P, mth, coop_chain, coop_p, coop_id)) return -WERR_HELPER;
  PSD_PROF_ADD(PROF_PRE);
  auto cls_at = [&](int j) -> int { return small ? rdlane_i(P.cls, j) : s.cls(j); };
  auto mu_at = [&](int j) -> double { return small ? rdlane_d(P.mu, j) : s.mu(j); };
  auto muc_at = [&](int j) -> double { return small ? rdlane_d(P.muc, j) : s.muc(j); };
  auto rc_at = [&](int j) -> double { return small ? rdlane_d(P.rc, j) : s.rc(j); };
  auto mn_at = [&](int j) -> double { return small ? rdlane_d(P.mn, j) : in.mn(j); };
  auto mx_at = [&](int j) -> double { return small ? rdlane_d(P.mx, j) : in.mx(j); };

  /* all-pairs speculation, mirror image of min_less_wave: pairs (start j, earlier piece k),
   * tasks of one start ordered by decreasing k */
  bool spec = false;
  unsigned long long sp_ev = 0, sp_inside = 0;
  double sp_mu = PSD_INF;
  int my_base = 0;
  int win = SPEC_WINDOW;
  PSD_PROF_SUB0();
  if (small) {
    unsigned long long m_start = ballot(lane < n && P.cls != CLS_STORE);
    int tj = -1, tk = 0;
    win = (n * SPEC_WINDOW <= WAVE) ? SPEC_WINDOW : ((n * SPEC_WINDOW_NARROW <= WAVE) ? SPEC_WINDOW_NARROW : 0);
    if (win > 0) {
      /* few pieces (the usual case): task lane = start * window + offset, no loop */
      if (m_start & ~1ull) { /* piece 0 has no earlier piece */
        spec = true;
        const int cj = win == SPEC_WINDOW ? lane / SPEC_WINDOW : lane / SPEC_WINDOW_NARROW;
        const int off = lane - cj * win;
        if (cj < n && ((m_start >> cj) & 1ull) && off < cj) {
          tj = cj;
          tk = cj - 1 - off;
        }
        my_base = lane * win;
      }
    } else {
      win = SPEC_WINDOW;
      int total = 0;
      for (unsigned long long m = m_start; m; m &= m - 1) {
        int c = ctz64(m);
        total += c < SPEC_WINDOW ? c : SPEC_WINDOW;
      }
      if (total > 0 && total <= WAVE) {
        spec = true;
        int base = 0;
        for (unsigned long long m = m_start; m; m &= m - 1) {
          int j = ctz64(m), cnt = j;
          if (cnt > SPEC_WINDOW) cnt = SPEC_WINDOW;
          if (lane == j) my_base = base;
          if (lane >= base && lane < base + cnt) {
            tj = j;
            tk = j - 1 - (lane - base);
          }
          base += cnt;
        }
      }
    }
    if (spec) {
      bool inside = false, at_left = false;
      int sp_steps = 0;
      PSD_PROF_SUB(PROF_S_ASSIGN);
      double level = 0.0, t_mx = 0.0, t_rc = 0.0, t_mn = 0.0, t_lc = 0.0;
      Coef c = {0.0, 0.0, 0.0};
      PieceOpt o = {0.0, 0.0, 0.0, 0.0};
      if (tj >= 0) {
        level = (s.cls(tj) == CLS_CONST_MU) ? s.muc(tj) : s.rc(tj);
        c = load_coef(in, tk);
        o.mean = s.om(tk);
        o.log_mean = s.mu(tk);
        o.cost = s.muc(tk);
        o.cost2 = s.oc2(tk);
        t_mx = in.mx(tk);
        t_rc = s.rc(tk);
        t_mn = in.mn(tk);
        t_lc = s.lc(tk);
      }
      PSD_PROF_SUB(PROF_S_LOAD);
      if (tj >= 0) {
        if (c.Log == 0) {
          sp_mu = mth.log_wild(psd_div(level - c.Constant, c.Linear)); /* fpl:563 */
        } else {
          if (has_two_roots(c, o, level)) {
            sp_mu = get_larger_root(c, o, t_mx, t_rc, level, &sp_steps, mth.rare_out());
          }
        }
        inside = t_mn < sp_mu && sp_mu < t_mx;
        if (!inside) at_left = t_lc <= level + NEWTON_EPSILON;
      }
      PSD_PROF_SUB(PROF_S_NEWTON);
      PSD_PROF_ITERS(PROF_IT_SPEC, sp_steps);
      sp_ev = ballot(inside || at_left);
      sp_inside = ballot(inside);
    }
  }
  PSD_PROF_ADD(PROF_SERIAL); /* diagnostic builds: the speculation round */
  int n_out = 0; /* pieces written so far; piece p lives at out[cap-1-p] */
  int i0 = n - 1;
  double prev_max_log_mean = mx_at(n - 1);
  /* deferred emission for functions of at most 64 pieces, as in min_less_wave; in ascending
   * order a piece contributes first the constant that starts at it (it extends downwards),
   * then its own kept or partial convex piece */
  bool e1 = false, e2 = false;
  double e1_lo = 0.0, e1_hi = 0.0;
  double e2_lo = 0.0, e2_hi = 0.0, e2_level = 0.0, e2_best = 0.0;
  for (;;) {
    PSD_PROF_COUNT(PROF_IT_ROUNDS);
    /* ---- search mode, walking down from i0: first piece j <= i0 starting a constant ---- */
    int j = -1;
    if (small) {
      unsigned long long m = ballot(lane <= i0 && P.cls != CLS_STORE);
      if (m) j = msb64(m);
    } else {
      for (int base = i0 | (WAVE - 1); base >= 0; base -= WAVE) { /* base = top of a chunk */
        int i = base - lane;
        bool hit = i <= i0 && i >= 0 && s.cls(i) != CLS_STORE;
        unsigned long long m = ballot(hit);
        if (m) {
          j = base - ctz64(m);
          break;
        }
      }
    }
    int cnt = i0 - j;
    if (small) {
      if (lane > j && lane <= i0) {
        e1 = true;
        e1_lo = P.mn;
        e1_hi = (lane == i0) ? prev_max_log_mean : P.mx;
      }
    } else {
      if (n_out + cnt + 2 > cap) return -WERR_OVERFLOW;
      for (int base = i0; base > j; base -= WAVE) {
        int i = base - lane;
        if (i > j) {
          Coef c = load_coef(in, i);
          double hi = (i == i0) ? prev_max_log_mean : in.mx(i);
          store_piece(out, cap - 1 - (n_out + (i0 - i)), c, in.mn(i), hi, data_i_out, PSD_INF);
        }
      }
      n_out += cnt;
    }
    if (cnt > 0) prev_max_log_mean = mn_at(j + 1);
    if (j < 0) break;
    double prev_min_cost, prev_best_log_mean;
    if (cls_at(j) == CLS_CONST_MU) { /* fpl:524-537 */
      double mu = mu_at(j);
      if (mu < prev_max_log_mean) {
        if (small) {
          if (lane == j) {
            e1 = true;
            e1_lo = mu;
            e1_hi = prev_max_log_mean;
          }
        } else {
          if (lane == 0)
            store_piece(out, cap - 1 - n_out, load_coef(in, j), mu, prev_max_log_mean,
                        data_i_out, PSD_INF);
          n_out++;
        }
      }
      prev_max_log_mean = mu;
      prev_best_log_mean = mu;
      prev_min_cost = muc_at(j);
    } else { /* fpl:500-510 */
      prev_min_cost = rc_at(j);
      prev_best_log_mean = mx_at(j);
    }
    /* ---- constant mode: highest piece k < j where the constant ends (fpl:549-602) ---- */
    int k_ev = -1;
    bool ev_inside = false;
    double ev_mu = 0.0;
    int scan_from = j - 1; /* first piece (walking down) not covered by the speculation */
    if (spec) {
      int cntj = j < win ? j : win;
      scan_from = j - 1 - cntj;
      if (cntj > 0) {
        int base = rdlane_i(my_base, j);
        unsigned long long range = ((1ull << cntj) - 1ull) << base;
        unsigned long long ev = sp_ev & range;
        if (ev) {
          int src = ctz64(ev);
          k_ev = j - 1 - (src - base);
          ev_inside = ((sp_inside >> src) & 1ull) != 0;
          ev_mu = rdlane_d(sp_mu, src);
        }
      }
    }
    if (k_ev < 0) { /* pieces beyond the speculation window: scan them now */
      for (int base = scan_from; base >= 0; base -= WAVE) {
        int k = base - lane;
        bool inside = false, at_left = false;
        double mu = PSD_INF;
        if (k >= 0) {
          Coef c = load_coef(in, k);
          if (c.Log == 0) {
            mu = d_log(psd_div(prev_min_cost - c.Constant, c.Linear)); /* fpl:563 */
          } else {
            PieceOpt o = {s.om(k), s.mu(k), s.muc(k), s.oc2(k)};
            if (has_two_roots(c, o, prev_min_cost)) {
              mu = get_larger_root(c, o, in.mx(k), s.rc(k), prev_min_cost);
            }
          }
          inside = in.mn(k) < mu && mu < in.mx(k);
          if (!inside) at_left = s.lc(k) <= prev_min_cost + NEWTON_EPSILON;
        }
        unsigned long long m_ev = ballot(inside || at_left);
        unsigned long long m_in = ballot(inside);
        if (m_ev) {
          int src = ctz64(m_ev);
          k_ev = base - src;
          ev_inside = ((m_in >> src) & 1ull) != 0;
          ev_mu = rdlane_d(mu, src);
          break;
        }
      }
    }
    Coef cc;
    cc.Linear = 0.0;
    cc.Log = 0.0;
    cc.Constant = prev_min_cost;
    /* where the constant ends (walking down): the start of the function (fpl:608-615), a
     * crossing inside piece k, then revisited (fpl:578-590), or the left end of piece k
     * (fpl:591-601) */
    double c_lo;
    bool last_round = false;
    if (k_ev < 0) {
      c_lo = mn_at(0);
      last_round = true;
    } else if (ev_inside) {
      c_lo = ev_mu;
      i0 = k_ev;
    } else {
      c_lo = mn_at(k_ev);
      i0 = k_ev - 1;
      if (i0 < 0) last_round = true;
    }
    if (small) {
      if (lane == j) {
        e2 = true;
        e2_lo = c_lo;
        e2_hi = prev_max_log_mean;
        e2_level = prev_min_cost;
        e2_best = prev_best_log_mean;
      }
    } else {
      if (lane == 0)
        store_piece(out, cap - 1 - n_out, cc, c_lo, prev_max_log_mean, data_i_out,
                    prev_best_log_mean);
      n_out++;
    }
    prev_max_log_mean = c_lo;
    if (last_round) break;
  }
  if (small) {
    /* one parallel pass; the result occupies out[cap-n_out .. cap) in ascending order */
    unsigned long long m1 = ballot(e1), m2 = ballot(e2);
    unsigned long long lb = lanes_below(lane);
    n_out = popc64(m1) + popc64(m2);
    if (n_out + 2 > cap) return -WERR_OVERFLOW;
    int pos = cap - n_out + popc64(m1 & lb) + popc64(m2 & lb);
    if (e2) {
      Coef cc;
      cc.Linear = 0.0;
      cc.Log = 0.0;
      cc.Constant = e2_level;
      store_piece(out, pos, cc, e2_lo, e2_hi, data_i_out, e2_best);
      pos++;
    }
    if (e1) store_piece(out, pos, P.c, e1_lo, e1_hi, data_i_out, PSD_INF);
  }
  wave_sync();
  PSD_PROF_ADD(PROF_WALK);
  return n_out;
}

}  // namespace PSD_VARIANT
}  // namespace psd
