/* fpop_envelope.h -- the min-envelope of two functions.
 *
 * Its parts, each once for every envelope: the candidates of a merged interval, the interval
 * table, a lane's load of its interval (EnvLane), the classification by lanes, the compaction of
 * a chunk (env_compact_chunk) and the sequential replay (min_env_serial).  min_env_impl is the
 * envelope by one wave, lists in LDS or HBM; fpop_coop.h has the one by two waves on lists in
 * HBM (fpop_wave.h describes the design).
 *
 * Reached only through fpop_wave.h: no include guard, compiled once per build variant into
 * namespace psd::PSD_VARIANT. */
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace psd {
namespace PSD_VARIANT {

/* Candidates emitted for one merged interval [a,b].  Every path of push_min_pieces emits
 * one of three shapes, with the source alternating between the two input pieces:
 *   n=1: [a,b]            n=2: [a,x1] [x1,b]            n=3: [a,x1] [x1,x2] [x2,b]
 * `first` is the source of the first piece (0: piece of fun1, 1: piece of fun2).  All split
 * points are strictly inside (a,b) and ordered (the reference tests that before pushing), so
 * push_piece's zero-width guard (fpl:1261-1267) can only ever drop the n=1 shape; it is
 * applied there.  Plain scalars: nothing here is indexed at run time (an indexed struct was
 * placed in scratch memory by the compiler). */
struct Cands {
  int n, first;
  double x1, x2;
};
PSD_D void cand_one(Cands &c, int src, double a, double b) {
  c.n = (b <= a) ? 0 : 1;
  c.first = src;
}
PSD_D void cand_two(Cands &c, int first, double x) {
  c.n = 2;
  c.first = first;
  c.x1 = x;
}
PSD_D void cand_three(Cands &c, int first, double x1, double x2) {
  c.n = 3;
  c.first = first;
  c.x1 = x1;
  c.x2 = x2;
}

/* push_min_pieces (fpl:870-1259) for one merged interval [a, b] =
 * [last_min_log_mean, first_max_log_mean] of it1 = c1, it2 = c2.
 * exp(a), exp(b), the optimum of the difference piece and its end costs are each needed by
 * several of the reference's helper calls (getCost / has_two_roots / get_*_root / argmin on
 * the same diff_piece); they are evaluated once here -- identical values, fewer serial
 * transcendentals. */
PSD_D void env_interval(const Coef &c1, const Coef &c2, double a, double b, bool same_at_left,
                        bool same_at_right, Cands &out) {
  if (same_funs(c1, c2)) { /* fpl:945-951 */
    cand_one(out, 0, a, b);
    return;
  }
  Coef d;
  d.Linear = c1.Linear - c2.Linear;
  d.Log = c1.Log - c2.Log;
  d.Constant = c1.Constant - c2.Constant;
  const double ea = d_exp(a), eb = d_exp(b);
  double mid_mean = (eb + ea) / 2; /* fpl:960 */
  double cost_diff_mid = get_cost(d, d_log(mid_mean));
  if (same_at_left && same_at_right) { /* fpl:963-971 */
    cand_one(out, cost_diff_mid < 0 ? 0 : 1, a, b);
    return;
  }
  if (d.Log == 0) { /* fpl:973-1019 */
    if (d.Linear == 0) {
      cand_one(out, d.Constant < 0 ? 0 : 1, a, b);
      return;
    }
    if (d.Constant == 0) {
      cand_one(out, d.Linear < 0 ? 0 : 1, a, b);
      return;
    }
    double x = d_log(psd_div(-d.Constant, d.Linear));
    if (a < x && x < b) {
      int first = (0 < d.Linear) ? 0 : 1;
      cand_two(out, first, x);
      return;
    }
    cand_one(out, cost_diff_mid < 0 ? 0 : 1, a, b);
    return;
  }
  double cost_diff_left = get_cost_e(d, a, ea);
  double cost_diff_right = get_cost_e(d, b, eb);
  const PieceOpt o = piece_opt(d);
  bool two_roots = has_two_roots(d, o, 0.0);
  double smaller_log_mean = PSD_INF, larger_log_mean = PSD_INF;
  if (two_roots) {
    smaller_log_mean = get_smaller_root(d, o, a, cost_diff_left, 0.0);
    larger_log_mean = get_larger_root(d, o, b, cost_diff_right, 0.0);
  }
  if (same_at_right) { /* fpl:1029-1093 */
    if (two_roots) {
      double x = smaller_log_mean;
      double opt = o.log_mean; /* diff_piece.argmin() */
      if (a < x && x < opt && opt < b) {
        int first = (cost_diff_left < 0) ? 0 : 1;
        cand_two(out, first, x);
        return;
      }
      bool it1_smaller_at_mean0 = 0 < d.Log;
      if (x < a) {
        cand_one(out, it1_smaller_at_mean0 ? 1 : 0, a, b);
      } else {
        cand_one(out, it1_smaller_at_mean0 ? 0 : 1, a, b);
      }
      return;
    }
    cand_one(out, cost_diff_mid < 0 ? 0 : 1, a, b);
    return;
  }
  if (same_at_left) { /* fpl:1094-1123 */
    if (two_roots) {
      double x = larger_log_mean;
      double opt = o.log_mean;
      if (a < opt && opt < x && x < b) {
        int first = (cost_diff_right < 0) ? 1 : 0;
        cand_two(out, first, x);
        return;
      }
    }
    cand_one(out, cost_diff_mid < 0 ? 0 : 1, a, b);
    return;
  }
  /* equal on neither side (fpl:1124-1258) */
  double first_log_mean = PSD_INF, second_log_mean = PSD_INF;
  double e_smaller = 0.0;
  if (two_roots) {
    bool larger_inside = a < larger_log_mean && larger_log_mean < b;
    e_smaller = d_exp(smaller_log_mean);
    bool smaller_inside = a < smaller_log_mean && 0 < e_smaller && smaller_log_mean < b;
    if (larger_inside) {
      if (smaller_inside && smaller_log_mean < larger_log_mean) {
        first_log_mean = smaller_log_mean;
        second_log_mean = larger_log_mean;
      } else {
        first_log_mean = larger_log_mean;
      }
    } else {
      if (smaller_inside) {
        first_log_mean = smaller_log_mean;
      }
    }
  }
  if (first_log_mean == PSD_INF) { /* no crossing inside (fpl:1238-1258) */
    double cost_diff;
    if (absd(cost_diff_mid) < NEWTON_EPSILON) {
      cost_diff = cost_diff_right;
    } else {
      cost_diff = cost_diff_mid;
    }
    cand_one(out, cost_diff < 0 ? 0 : 1, a, b);
    return;
  }
  /* one or two crossings: both cases may test the sign of the difference at the mean-space
   * midpoint of [a, first crossing] (fpl:1178-1179,1211-1212) */
  const bool two = second_log_mean != PSD_INF;
  const bool need_before = !two || (second_log_mean - first_log_mean < first_log_mean - a);
  double cost_diff_before = 0.0;
  if (need_before) {
    double e_first = (first_log_mean == smaller_log_mean) ? e_smaller : d_exp(first_log_mean);
    double before_mean = (ea + e_first) / 2;
    cost_diff_before = get_cost(d, d_log(before_mean));
  }
  if (two) {
    bool it1_larger_before;
    if (need_before) {
      it1_larger_before = cost_diff_before < 0;
    } else {
      double log_mean_between = (first_log_mean + second_log_mean) / 2;
      double cost_diff_between = get_cost(d, log_mean_between);
      it1_larger_before = !(cost_diff_between < 0);
    }
    int first = it1_larger_before ? 0 : 1;
    cand_three(out, first, first_log_mean, second_log_mean);
  } else {
    double after_mean = (b + first_log_mean) / 2; /* a log-mean, fpl:1216 */
    double cost_diff_after = get_cost(d, after_mean);
    if (cost_diff_before < 0) {
      if (cost_diff_after < 0) {
        cand_one(out, 0, a, b);
      } else {
        cand_two(out, 0, first_log_mean);
      }
    } else {
      if (cost_diff_after < 0) {
        cand_two(out, 1, first_log_mean);
      } else {
        cand_one(out, 1, a, b);
      }
    }
  }
}

/* number of pieces of f (sorted by max_log_mean) with max_log_mean < x */
template <class L>
PSD_D int rank_mx(const L &f, int n, double x) {
  if (n <= 32) { /* independent broadcast reads beat a dependent binary search */
    int r = 0;
    for (int j = 0; j < n; j++) r += f.mx(j) < x ? 1 : 0;
    return r;
  }
  int lo = 0, hi = n;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (f.mx(mid) < x) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo;
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

/* Merged-interval table of functions too long for the 32+32 table of min_env_impl: interval k
 * ends at the k-th distinct max_log_mean.  First the entries owned by f1 (every end of f1);
 * returns how many ends of f1 are also ends of f2.  staged: the ends of f2 in LDS (fpop_coop.h),
 * or nullptr to rank in the list itself */
template <class L, class S>
PSD_D int env_table_first(const L &f1, int n1, const L &f2, int n2, const S &s,
                          const ldouble *staged) {
  const int lane = lane_id();
  const int iv_cap = s.iv_cap();
  int dup_before = 0; /* ends of f1 that are also ends of f2, among earlier chunks */
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

/* Everything push_min_pieces needs for merged interval (i1,i2): loads the two pieces and
 * the neighbours it inspects (fpl:876-932), classifies, returns candidates. */
template <class L>
PSD_D void env_interval_at(const L &f1, int n1, const L &f2, int n2, int i1, int i2, Cands &cands,
                           double &a_out, double &b_out, Coef &c1, Coef &c2, int &err) {
  c1 = load_coef(f1, i1);
  c2 = load_coef(f2, i2);
  double mn1 = f1.mn(i1), mx1 = f1.mx(i1), mn2 = f2.mn(i2), mx2 = f2.mx(i2);
  bool same_at_left, same_at_right;
  double last_min_log_mean, first_max_log_mean;
  bool sentinel = false;
  if (mn1 < mn2) {
    if (i2 == 0) sentinel = true;
    same_at_left = !sentinel && same_funs(load_coef(f2, i2 - 1), c1);
    last_min_log_mean = mn2;
  } else {
    last_min_log_mean = mn1;
    if (mn2 < mn1) {
      if (i1 == 0) sentinel = true;
      same_at_left = !sentinel && same_funs(load_coef(f1, i1 - 1), c2);
    } else {
      if (i1 == 0 && i2 == 0) {
        same_at_left = false;
      } else {
        if (i1 == 0 || i2 == 0) sentinel = true;
        same_at_left = !sentinel && same_funs(load_coef(f1, i1 - 1), load_coef(f2, i2 - 1));
      }
    }
  }
  if (mx1 < mx2) {
    if (i1 + 1 >= n1) sentinel = true;
    same_at_right = !sentinel && same_funs(load_coef(f1, i1 + 1), c2);
    first_max_log_mean = mx1;
  } else {
    first_max_log_mean = mx2;
    if (mx2 < mx1) {
      if (i2 + 1 >= n2) sentinel = true;
      same_at_right = !sentinel && same_funs(c1, load_coef(f2, i2 + 1));
    } else {
      if (i1 + 1 == n1 && i2 + 1 == n2) {
        same_at_right = false;
      } else {
        if (i1 + 1 >= n1 || i2 + 1 >= n2) sentinel = true;
        same_at_right = !sentinel && same_funs(load_coef(f1, i1 + 1), load_coef(f2, i2 + 1));
      }
    }
  }
  cands.n = 0;
  cands.first = 0;
  cands.x1 = cands.x2 = 0.0;
  a_out = last_min_log_mean;
  b_out = first_max_log_mean;
  if (sentinel) {
    err |= WERR_SENTINEL;
    return;
  }
  if (last_min_log_mean == first_max_log_mean) { /* fpl:933-944 */
    err |= WERR_ZERO_INTERVAL;
    return;
  }
  env_interval(c1, c2, last_min_log_mean, first_max_log_mean, same_at_left, same_at_right,
               cands);
}

/* The same classification as env_interval(), written for SIMT execution: one lane per merged
 * interval, and every transcendental evaluation site is reached by all lanes that need it at
 * the same time (predicated phases) instead of each lane walking its own branch of
 * push_min_pieces -- a wave otherwise executes the union of all branches one after another.
 * The arithmetic per lane is identical to env_interval(). */
template <bool HELP, class M>
PSD_D void env_classify_lanes(bool valid, const Coef &c1, const Coef &c2, double a, double b,
                              bool same_at_left, bool same_at_right, Cands &out, int chain,
                              int &err, M &mth) {
  out.n = 0;
  out.first = 0;
  out.x1 = out.x2 = 0.0;
  Coef d;
  d.Linear = c1.Linear - c2.Linear;
  d.Log = c1.Log - c2.Log;
  d.Constant = c1.Constant - c2.Constant;
  const bool triv = same_funs(c1, c2);  /* fpl:945-951 */
  const bool act = valid && !triv;
  PSD_PROF_T0();
  const bool both = same_at_left && same_at_right;
  const bool hard = act && !both;
  const bool degen = hard && d.Log == 0;                              /* fpl:973-1019 */
  const bool degen_root = degen && d.Linear != 0 && d.Constant != 0;  /* fpl:996 */
  const bool rootp = hard && d.Log != 0;
  bool root_posted = false;
#ifdef PSD_HELPER_WAVES
  if (HELP) {
    /* The helper wave starts on the larger roots (fpl:1027) right away: it derives the
     * optimum of the difference piece and has_two_roots itself -- same code, same bits --
     * while this wave evaluates the end costs, the midpoint and the smaller roots. */
    if (ballot(rootp)) {
      Mail &m = g_sm.mail[chain];
      const int l = lane_id();
      m.flags[l] = rootp ? 1 : 0;
      m.d_lin[l] = d.Linear;
      m.d_log[l] = d.Log;
      m.d_con[l] = d.Constant;
      m.b[l] = b;
      mail_post(chain, HOP_ROOT);
      root_posted = true;
    }
  }
#endif
  /* phases A-D: exp(a), exp(b); the cost at the mean-space midpoint (fpl:960-961); the one log
   * site for the degenerate crossing and for argmin() of the difference; the optimum of the
   * difference piece, its end costs, has_two_roots (fpl:1020-1022).  Six transcendentals per
   * interval, evaluated in three interleaved pairs (the values are those of the single calls):
   * exp(a) | exp(b), log(midpoint) | log(argmin_mean), exp for the cost at each of the two. */
  double ea = 0.0, eb = 0.0, cost_diff_mid = 0.0;
  /* (psd_div: against a constant piece the difference has the function piece's own Linear,
   * which may be 1 - k ulp; peakseg_detmath.h) */
  const double larg = degen ? psd_div(-d.Constant, d.Linear) : psd_div(-d.Log, d.Linear);
  const bool need_l = degen_root || rootp;
  double lres = 0.0;
  PieceOpt o = {0.0, 0.0, 0.0, 0.0};
  double cost_diff_left = 0.0, cost_diff_right = 0.0;
  bool two_roots = false;
  if (ballot(act)) {
    mth.exp2((act && a != -PSD_INF) ? a : 0.0, act ? b : 0.0, ea, eb);
    if (a == -PSD_INF) ea = 0.0; /* exp(-Inf) */
    double log_mid;
    mth.log2(act ? (eb + ea) / 2 : 1.0, need_l ? larg : 1.0, log_mid, lres);
    if (!need_l) lres = 0.0;
    double e_mid, e_opt;
    mth.exp2(log_mid == -PSD_INF ? 0.0 : log_mid, (rootp && lres != -PSD_INF) ? lres : 0.0, e_mid,
           e_opt);
    if (act) cost_diff_mid = get_cost_e(d, log_mid, e_mid);
    if (!act) ea = eb = 0.0;
    if (rootp) o.cost = get_cost_e(d, lres, e_opt);
  }
  PSD_PROF_ADD(PROF_C_MID);
  if (rootp) {
    cost_diff_left = get_cost_e(d, a, ea);
    cost_diff_right = get_cost_e(d, b, eb);
    o.mean = larg;
    o.log_mean = lres;
    double loss_without_log_term = d.Linear * o.mean + d.Constant;
    o.cost2 = loss_without_log_term + o.log_mean * d.Log;
    two_roots = has_two_roots(d, o, 0.0);
  }
  PSD_PROF_ADD(PROF_C_OPT);
  /* phases E, F: the two Newton solves (fpl:1023-1028) */
  double smaller_log_mean = PSD_INF, larger_log_mean = PSD_INF;
  int it_small = 0, it_large = 0;
  if (two_roots) smaller_log_mean = get_smaller_root(d, o, a, cost_diff_left, 0.0, &it_small);
  PSD_PROF_ADD(PROF_C_SMALL);
  /* Phase G needs more evaluations for intervals equal on neither side (fpl:1124-1258).  What
   * depends on the smaller root alone is evaluated here, while the helper may still be at the
   * larger roots: exp(smaller root), and the cost before the first crossing as if the smaller
   * root were it (the usual case; replaced below when the larger root comes first). */
  const bool neither = rootp && !same_at_left && !same_at_right;
  double e_smaller = 0.0, cost_before_smaller = 0.0;
  /* (before the wait against after it: 1148 -> 1141 ms on 100 k bins x 64; without a helper
   * there is no wait to fill, and the throughput build lost 3 to 9 % with it:
   * profiles/r02/ab_step_barrier.log, s0/s1 and w0/v0) */
  constexpr bool EARLY_TAIL = HELP;
  if (EARLY_TAIL && ballot(neither && two_roots)) {
    const bool on = neither && two_roots;
    e_smaller = mth.exp(on ? smaller_log_mean : 0.0);
    cost_before_smaller = mth.cost(d, mth.log(on ? (ea + e_smaller) / 2 : 1.0));
    if (!on) e_smaller = 0.0;
  }
#ifdef PSD_HELPER_WAVES
  if (HELP) {
    if (root_posted) {
      if (!mail_wait(chain)) err |= WERR_HELPER;
      if (two_roots) {
        /* the early exit of get_larger_root (fpl:75-79), which the helper leaves to us */
        const bool beyond = (o.cost2 < cost_diff_right && cost_diff_right < 0.0) ||
                            (o.cost2 > cost_diff_right && cost_diff_right > 0.0);
        larger_log_mean = beyond ? b + 1 : g_sm.mail[chain].res_large[lane_id()];
      }
    }
  } else
#endif
  {
    if (two_roots) larger_log_mean = get_larger_root(d, o, b, cost_diff_right, 0.0, &it_large, mth.rare_out());
  }
  (void)root_posted;
  PSD_PROF_ADD(PROF_C_LARGE);
  PSD_PROF_ITERS(PROF_IT_SMALL, it_small);
  PSD_PROF_ITERS(PROF_IT_LARGE, it_large);
  /* phase G, the part that needs both roots */
  if (!EARLY_TAIL && neither && two_roots) e_smaller = mth.exp(smaller_log_mean);
  double first_log_mean = PSD_INF, second_log_mean = PSD_INF;
  { /* which roots are crossings inside (a, b), in order: selects, no region per case */
    const bool on = neither & two_roots;
    const bool larger_inside = on & (a < larger_log_mean) & (larger_log_mean < b);
    const bool smaller_inside =
        on & (a < smaller_log_mean) & (0 < e_smaller) & (smaller_log_mean < b);
    const bool both_inside = larger_inside & smaller_inside & (smaller_log_mean < larger_log_mean);
    first_log_mean = smaller_inside ? smaller_log_mean : first_log_mean;
    first_log_mean = larger_inside ? larger_log_mean : first_log_mean;
    first_log_mean = both_inside ? smaller_log_mean : first_log_mean;
    second_log_mean = both_inside ? larger_log_mean : second_log_mean;
  }
  const bool crossing = neither && first_log_mean != PSD_INF;
  const bool two = crossing && second_log_mean != PSD_INF;
  const bool need_before =
      crossing && (!two || (second_log_mean - first_log_mean < first_log_mean - a));
  const bool need_other = crossing && !(two && need_before);
  /* between the crossings (two) or after the crossing (one): both are log-means */
  const double x_other =
      two ? (first_log_mean + second_log_mean) / 2 : (b + first_log_mean) / 2;
  double cost_diff_other = 0.0;
  if (need_other) cost_diff_other = mth.cost(d, x_other);
  double cost_diff_before = 0.0;
  if (EARLY_TAIL) {
    if (need_before) cost_diff_before = cost_before_smaller;
    /* the larger root is the first crossing: exp(first crossing) and the cost before it anew */
    const bool redo = need_before && first_log_mean != smaller_log_mean;
    if (ballot(redo)) {
      const double e_first = mth.exp(redo ? first_log_mean : 0.0);
      const double c_before = mth.cost(d, mth.log(redo ? (ea + e_first) / 2 : 1.0));
      if (redo) cost_diff_before = c_before;
    }
  } else {
    /* exp(first crossing) unless it is the value already computed */
    double e_first = e_smaller;
    if (need_before && first_log_mean != smaller_log_mean) e_first = mth.exp(first_log_mean);
    if (need_before) cost_diff_before = mth.cost(d, mth.log((ea + e_first) / 2));
  }

  PSD_PROF_ADD(PROF_C_TAIL);
  /* ---- decisions (no more transcendentals) ----
   * The decision tree of push_min_pieces as values: every case's shape (1-3 pieces), first
   * source and crossing is computed by comparisons of values that all lanes hold, and the tree
   * only selects among them, innermost case first -- no exec-masked region per case.  A
   * one-piece shape is dropped when the interval is empty (cand_one). */
  const int by_mid = cost_diff_mid < 0 ? 0 : 1;
  const int one = (b <= a) ? 0 : 1; /* cand_one's n */
  /* fpl:1238-1258: no crossing inside */
  const int by_ends = ((absd(cost_diff_mid) < NEWTON_EPSILON) ? cost_diff_right : cost_diff_mid) < 0 ? 0 : 1;
  int n = one, first = by_ends;
  double x1 = 0.0, x2 = 0.0;
  { /* fpl:1206-1237: one crossing */
    const bool before = cost_diff_before < 0, other = cost_diff_other < 0;
    const bool split = before != other;
    n = crossing ? (split ? 2 : one) : n;
    first = crossing ? (before ? 0 : 1) : first;
    x1 = (crossing & split) ? first_log_mean : x1;
  }
  { /* fpl:1171-1205: two crossings */
    const bool it1_larger_before = need_before ? (cost_diff_before < 0) : !(cost_diff_other < 0);
    n = two ? 3 : n;
    first = two ? (it1_larger_before ? 0 : 1) : first;
    x1 = two ? first_log_mean : x1;
    x2 = two ? second_log_mean : x2;
  }
  { /* fpl:1094-1123 */
    const double x = larger_log_mean, opt = o.log_mean;
    const bool cut = two_roots & (a < opt) & (opt < x) & (x < b);
    n = same_at_left ? (cut ? 2 : one) : n;
    first = same_at_left ? (cut ? ((cost_diff_right < 0) ? 1 : 0) : by_mid) : first;
    x1 = same_at_left ? (cut ? x : 0.0) : x1;
    x2 = same_at_left ? 0.0 : x2;
  }
  { /* fpl:1029-1093 */
    const double x = smaller_log_mean, opt = o.log_mean;
    const bool cut = two_roots & (a < x) & (x < opt) & (opt < b);
    const bool it1_smaller_at_mean0 = 0 < d.Log;
    const int side = ((x < a) == it1_smaller_at_mean0) ? 1 : 0;
    const int f_cut = !(cost_diff_left < 0), f_whole = two_roots ? side : by_mid;
    const int f = cut ? f_cut : f_whole;
    n = same_at_right ? (cut ? 2 : one) : n;
    first = same_at_right ? f : first;
    x1 = same_at_right ? (cut ? x : 0.0) : x1;
    x2 = same_at_right ? 0.0 : x2;
  }
  { /* fpl:973-1019 */
    const bool cut = (d.Linear != 0) & (d.Constant != 0) & (a < lres) & (lres < b);
    const int f_lin0 = !(d.Constant < 0), f_con0 = !(d.Linear < 0), f_cut = !(0 < d.Linear);
    int f = cut ? f_cut : by_mid;
    f = (d.Constant == 0) ? f_con0 : f;
    f = (d.Linear == 0) ? f_lin0 : f;
    n = degen ? (cut ? 2 : one) : n;
    first = degen ? f : first;
    x1 = degen ? (cut ? lres : 0.0) : x1;
    x2 = degen ? 0.0 : x2;
  }
  /* fpl:963-971, fpl:945-951 */
  const bool flat = triv | both;
  n = flat ? one : n;
  first = triv ? 0 : (both ? by_mid : first);
  x1 = flat ? 0.0 : x1;
  x2 = flat ? 0.0 : x2;
  out.n = valid ? n : 0;
  out.first = valid ? first : 0;
  out.x1 = valid ? x1 : 0.0;
  out.x2 = valid ? x2 : 0.0;
}

/* Loads merged interval (i1,i2): the two pieces and the interval [a,b] (fpl:876-932 without
 * the neighbour tests, see env_neighbour_flags). */
template <class L>
PSD_D void env_load_interval(const L &f1, int n1, const L &f2, int n2, int i1, int i2, Coef &c1,
                             Coef &c2, double &a, double &b, int &err) {
  c1 = load_coef(f1, i1);
  c2 = load_coef(f2, i2);
  double mn1 = f1.mn(i1), mx1 = f1.mx(i1), mn2 = f2.mn(i2), mx2 = f2.mx(i2);
  /* the piece that started earlier / ends later must have a neighbour on that side; the
   * reference would read a std::list sentinel otherwise */
  /* ('&' and '|': every term is a comparison of values already loaded, and short-circuit
   * evaluation made each an exec-masked region) */
  bool sentinel = ((mn1 < mn2) & (i2 == 0)) | ((mn2 < mn1) & (i1 == 0)) |
                  ((mn1 == mn2) & ((i1 == 0) != (i2 == 0))) | ((mx1 < mx2) & (i1 + 1 >= n1)) |
                  ((mx2 < mx1) & (i2 + 1 >= n2)) |
                  ((mx1 == mx2) & ((i1 + 1 == n1) != (i2 + 1 == n2)));
  a = mn1 < mn2 ? mn2 : mn1;
  b = mx1 < mx2 ? mx1 : mx2;
  if (sentinel) err |= WERR_SENTINEL;
  if (a == b) err |= WERR_ZERO_INTERVAL; /* fpl:933-944 */
}

/* same_at_left / same_at_right of push_min_pieces (fpl:876-932) compare the pieces next to
 * (it1, it2) in the two input lists.  Those neighbours are exactly the pair of pieces of the
 * previous / next merged interval: if it1 starts before it2 the previous interval is
 * (it1, prev2), if it2 starts first it is (prev1, it2), if both start together (prev1, prev2)
 * -- and the test made is sameFuns of that pair in each case; symmetrically on the right.
 * So same_at_left(k) = sameFuns of interval k-1, same_at_right(k) = sameFuns of interval k+1
 * (false at the two ends of the function, fpl:894-896,919-922). */
template <class L, class S>
PSD_D void env_neighbour_flags(const L &f1, const L &f2, const S &s, int k, int K, bool valid,
                               bool triv, bool &same_at_left, bool &same_at_right) {
  const int lane = lane_id();
  unsigned long long m_triv = ballot(valid && triv);
  same_at_left = lane > 0 && ((m_triv >> (lane - 1)) & 1ull) != 0;
  same_at_right = lane < WAVE - 1 && ((m_triv >> (lane + 1)) & 1ull) != 0;
  /* chunk edges (functions with more than 64 merged intervals): look the neighbour up */
  if (valid && lane == 0 && k > 0) {
    int e = s.iv(k - 1);
    same_at_left = same_funs(load_coef(f1, e >> 16), load_coef(f2, e & 0xffff));
  }
  if (valid && lane == WAVE - 1 && k + 1 < K) {
    int e = s.iv(k + 1);
    same_at_right = same_funs(load_coef(f1, e >> 16), load_coef(f2, e & 0xffff));
  }
}

/* push_piece's "same as last" test (fpl:1270-1273) */
PSD_D bool coalesces(const Coef &last, double last_prv, int last_di, const Coef &c, double prv,
                     int di) {
  return same_funs(last, c) & (prv == last_prv) & (di == last_di);
}
PSD_D bool bit_identical(const Coef &last, double last_prv, int last_di, const Coef &c,
                         double prv, int di) {
  return (psd_d2u(last.Linear) == psd_d2u(c.Linear)) & (psd_d2u(last.Log) == psd_d2u(c.Log)) &
         (psd_d2u(last.Constant) == psd_d2u(c.Constant)) & (psd_d2u(last_prv) == psd_d2u(prv)) &
         (last_di == di);
}

/* What one lane holds of its merged interval: the two pieces, the interval, the candidates */
struct EnvLane {
  Cands cd;
  double ia, ib;
  Coef c1, c2;
  double prv1, prv2;
  int di1, di2, i1, i2;
  int err;
};
template <class L, class S>
PSD_D void env_lane_load(const L &f1, int n1, const L &f2, int n2, const S &s, int k, bool valid,
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
/* push_piece over one chunk of 64 merged intervals, one lane per interval, by ballots and prefix
 * scans: lane `lane` holds interval k's candidates in `e` (valid: k < K).  n_out, the number of
 * pieces in `out`, and last_id, the source piece of the last candidate emitted so far as
 * (list << 20) | index (-1: none), carry from chunk to chunk.  Returns 0, or -(WERR_* bits) and
 * then nothing usable is in `out`; -WERR_SERIAL: the caller replays the intervals sequentially
 * (min_env_serial). */
template <class L>
PSD_D int env_compact_chunk(const L &f1, const L &f2, const L &out, int cap, bool valid,
                            const EnvLane &e, int &n_out, int &last_id) {
  const int lane = lane_id();
  const Cands &cd = e.cd;
  /* first / last candidate of this lane */
  const int src0 = cd.first, src1 = cd.first ^ 1; /* the third piece has source src0 again */
  Coef fc = src0 ? e.c2 : e.c1;
  double fprv = src0 ? e.prv2 : e.prv1;
  int fdi = src0 ? e.di2 : e.di1;
  int lsrc = cd.n == 2 ? src1 : src0;
  /* piece q of this interval spans [lo_q, hi_q] */
  const double hi0 = cd.n == 1 ? e.ib : cd.x1;
  const double hi1 = cd.n == 2 ? e.ib : cd.x2;
  bool has = valid && cd.n > 0;
  unsigned long long m_has = ballot(has);
  unsigned long long m_err = ballot(e.err != 0);
  if (m_err) {
    int eb = 0;
    for (int l = 0; l < WAVE; l++) eb |= shfl_i(e.err, l);
    return -eb;
  }
  /* predecessor = last candidate of the nearest lower lane that has one, else the carry.
   * Only its identity crosses lanes; its fields are re-read from the input list. */
  unsigned long long lb = lanes_below(lane);
  unsigned long long below = m_has & lb;
  const int my_last_id = (lsrc << 20) | (lsrc ? e.i2 : e.i1);
  int pid = shfl_i(my_last_id, below ? msb64(below) : 0); /* per-lane source */
  if (!below) pid = last_id;
  const bool have_pred = pid >= 0;
  /* (every lane reads a predecessor -- piece 0 where it has none -- and the tests are masked
   * afterwards: one LDS round trip, no exec-masked region) */
  const L &pl = (have_pred && (pid >> 20)) ? f2 : f1;
  const int pi = have_pred ? (pid & 0xfffff) : 0;
  const Coef pc = load_coef(pl, pi);
  const double pprv = pl.prv(pi);
  const int pdi = pl.di(pi);
  const bool follows = has & have_pred;
  const bool co = follows & coalesces(pc, pprv, pdi, fc, fprv, fdi);
  const bool bi = bit_identical(pc, pprv, pdi, fc, fprv, fdi);
  const bool head0 = !co; /* does the first candidate start a new output piece? */
  const bool fuzzy = co & !bi;
  /* candidates 2 and 3 of a lane alternate it1/it2 with same_funs(it1,it2) false, so
   * they always start a new piece -- provided the run they follow is bit-identical to
   * its head, which `fuzzy` checks. */
  if (ballot(fuzzy)) return -WERR_SERIAL;
  int heads = has ? ((head0 ? 1 : 0) + (cd.n - 1)) : 0;
  unsigned long long hb0 = ballot((heads & 1) != 0);
  unsigned long long hb1 = ballot((heads & 2) != 0);
  int heads_before = popc64(hb0 & lb) + 2 * popc64(hb1 & lb);
  int heads_total = popc64(hb0) + 2 * popc64(hb1);
  if (n_out + heads_total > cap) return -WERR_OVERFLOW;
  int slot = n_out + heads_before - (head0 ? 0 : 1); /* piece candidate 0 belongs to */
  if (has & head0) store_piece(out, slot, fc, e.ia, hi0, fdi, fprv);
  if (has & (cd.n >= 2)) {
    Coef c = src1 ? e.c2 : e.c1;
    store_piece(out, slot + 1, c, cd.x1, hi1, src1 ? e.di2 : e.di1, src1 ? e.prv2 : e.prv1);
  }
  if (has & (cd.n >= 3)) store_piece(out, slot + 2, fc, cd.x2, e.ib, fdi, fprv);
  wave_sync();
  /* a candidate that extends the previous piece only moves that piece's right end; of
   * the members of a run only the last one (in this chunk) writes, after the heads. */
  {
    const unsigned long long m_head0 = ballot(has & head0);
    const unsigned long long above = m_has & ~lb & ~(1ull << lane);
    /* (bit 63 keeps ctz64 defined for the top lane of the run; it never is the lowest bit
     * of a non-empty `above`) */
    const bool next_is_head = !above | (((m_head0 >> ctz64(above | (1ull << 63))) & 1ull) != 0);
    if (has & !head0 & ((cd.n >= 2) | next_is_head)) out.mx(slot) = hi0;
  }
  wave_sync();
  n_out += heads_total;
  if (m_has) last_id = rdlane_i(my_last_id, msb64(m_has));
  return 0;
}

/* exact sequential replay of fpl:832-860 + push_piece on lane 0 (cold path) */
template <class L, class S>
PSD_NOINLINE int min_env_serial(L f1_, int n1_, L f2_, int n2_, L out_, int cap_, S s_, int K_) {
  const L f1 = f1_.uniformed(), f2 = f2_.uniformed(), out = out_.uniformed();
  const S s = s_.uniformed();
  const int n1 = uniform_i(n1_), n2 = uniform_i(n2_), cap = uniform_i(cap_), K = uniform_i(K_);
  const int lane = lane_id();
  int count = 0;
  int err = 0;
  if (lane == 0) {
    for (int k = 0; k < K && !err; k++) {
      int e = s.iv(k);
      int i1 = e >> 16, i2 = e & 0xffff;
      Cands cd;
      Coef c1, c2;
      double ia, ib;
      env_interval_at(f1, n1, f2, n2, i1, i2, cd, ia, ib, c1, c2, err);
      for (int q = 0; q < cd.n; q++) {
        int src = cd.first ^ (q & 1);
        double lo = q == 0 ? ia : (q == 1 ? cd.x1 : cd.x2);
        double hi = q == cd.n - 1 ? ib : (q == 0 ? cd.x1 : cd.x2);
        Coef c = src ? c2 : c1;
        double prv = src ? f2.prv(i2) : f1.prv(i1);
        int di = src ? f2.di(i2) : f1.di(i1);
        if (count > 0 && coalesces(load_coef(out, count - 1), out.prv(count - 1),
                                   out.di(count - 1), c, prv, di)) {
          out.mx(count - 1) = hi;
        } else {
          if (count >= cap) {
            err |= WERR_OVERFLOW;
            break;
          }
          store_piece(out, count, c, lo, hi, di, prv);
          count++;
        }
      }
    }
  }
  wave_sync();
  err = shfl_i(err, 0);
  count = shfl_i(count, 0);
  return err ? -err : count;
}

/* min-envelope: out = pointwise min(f1, f2). */
template <bool HELP, bool SMALL, class L, class S, class M>
PSD_D int min_env_impl(L f1_, int n1_, L f2_, int n2_, L out_, int cap_, S s_, int chain_,
                       M &mth) {
  const int chain = uniform_i(chain_);
  const L f1 = f1_.uniformed(), f2 = f2_.uniformed(), out = out_.uniformed();
  const S s = s_.uniformed();
  const int n1 = uniform_i(n1_), n2 = uniform_i(n2_), cap = uniform_i(cap_);
  const int lane = lane_id();
  const int iv_cap = s.iv_cap();
  if (SMALL) PSD_ASSUME(n1 <= 32 && n2 <= 32);
  PSD_PROF_T0();
  /* ---- merged-interval table: interval k ends at the k-th distinct max_log_mean ---- */
  int K;
  if (SMALL || (n1 <= 32 && n2 <= 32)) { /* SMALL: guaranteed by the caller */
    /* both lists in one pass: lanes 0-31 rank the ends of f1 in f2, lanes 32-63 those of f2
     * in f1 (the usual case: one ballot, one pass of broadcast reads) */
    const int side = lane >> 5, idx = lane & 31;
    const int n_own = side ? n2 : n1, n_oth = side ? n1 : n2;
    const L &own = side ? f2 : f1;
    const L &oth = side ? f1 : f2;
    const bool valid = idx < n_own;
    double x = PSD_INF; /* lanes without an end never count as "less than" anything */
    int p = 0;
    bool dup = false;
    if (valid) x = own.mx(idx);
    /* Every end is in a register of its lane (f1's in lanes 0-31, f2's in lanes 32-63), so the
     * other list's ends are broadcast with v_readlane instead of read from LDS: four
     * instructions per end and no address arithmetic.  Both halves count against every
     * broadcast end; each keeps the count it needs.  (Against eight independent LDS reads per
     * round trip: 1180 -> 1177 ms on 100 k bins x 64, profiles/r02/ab_rank_by_readlane.log.) */
    int p_vs_f2 = 0, p_vs_f1 = 0;
    /* four ends per trip (a loop with cross-lane reads is not unrolled by the compiler); the
     * lanes read beyond the list hold +Inf */
    for (int j = 0; j < n2; j += 4) {
      p_vs_f2 += rdlane_d(x, 32 + j) < x ? 1 : 0;
      p_vs_f2 += rdlane_d(x, 33 + j) < x ? 1 : 0;
      p_vs_f2 += rdlane_d(x, 34 + j) < x ? 1 : 0;
      p_vs_f2 += rdlane_d(x, 35 + j) < x ? 1 : 0;
    }
    for (int j = 0; j < n1; j += 4) {
      p_vs_f1 += rdlane_d(x, j) < x ? 1 : 0;
      p_vs_f1 += rdlane_d(x, j + 1) < x ? 1 : 0;
      p_vs_f1 += rdlane_d(x, j + 2) < x ? 1 : 0;
      p_vs_f1 += rdlane_d(x, j + 3) < x ? 1 : 0;
    }
    p = side ? p_vs_f1 : p_vs_f2;
    /* both lists are sorted and free of repeats: an end also present in the other list is the
     * other list's end number p */
    if (valid && p < n_oth) dup = oth.mx(p) == x;
    unsigned long long md = ballot(dup);
    const unsigned long long half = side ? (md >> 32) : (md & 0xffffffffull);
    if (valid && !(side && dup)) {
      int k = idx + p - popc64(half & lanes_below(idx));
      if (k < iv_cap) s.iv(k) = side ? ((p << 16) | idx) : ((idx << 16) | p);
    }
    K = n1 + n2 - popc64(md & 0xffffffffull);
  } else {
    const int dup_total = env_table_first(f1, n1, f2, n2, s, nullptr);
    env_table_second(f1, n1, f2, n2, s, nullptr);
    K = n1 + n2 - dup_total;
  }
  /* (i1 << 16) | i2 in a signed int: both indices stay below 32768 (SPILL_CAP_MAX) */
  if (K > iv_cap || n1 > SPILL_CAP_MAX || n2 > SPILL_CAP_MAX) return -WERR_OVERFLOW;
  wave_sync();
  PSD_PROF_ADD(PROF_TABLE);

  /* ---- one lane per interval; ballot/prefix-scan compaction ---- */
  int n_out = 0, last_id = -1;
  int status = 0;
  for (int base = 0; base < K; base += WAVE) {
    const int k = base + lane;
    const bool valid = k < K;
    EnvLane e;
    bool sl = false, sr = false;
    PSD_PROF_T0();
    env_lane_load(f1, n1, f2, n2, s, k, valid, e);
    env_neighbour_flags(f1, f2, s, k, K, valid, valid && same_funs(e.c1, e.c2), sl, sr);
    PSD_PROF_ADD(PROF_C_LOAD);
    env_classify_lanes<HELP>(valid && e.err == 0, e.c1, e.c2, e.ia, e.ib, sl, sr, e.cd, chain, e.err,
                             mth);
    PSD_PROF_ADD(PROF_CLASSIFY);
    status = env_compact_chunk(f1, f2, out, cap, valid, e, n_out, last_id);
    PSD_PROF_ADD(PROF_COMPACT);
    if (status < 0 || SMALL) break; /* SMALL: K <= 64, one chunk */
  }
  if (status < 0 && status != -WERR_SERIAL) return status;
#ifdef PSD_FORCE_SERIAL_ENV /* tests only: every envelope takes the sequential replay */
  status = -WERR_SERIAL;
#endif
  if (status == -WERR_SERIAL) {
    /* the specialised version leaves the replay (and the call it takes) to the general one */
    if (SMALL) return -WERR_SERIAL;
    if (lane == 0) g_sm.serial[wave_id()]++;
    n_out = min_env_serial(f1, n1, f2, n2, out, cap, s, K);
    PSD_PROF_ADD(PROF_SERIAL);
  }
  return n_out;
}

}  // namespace PSD_VARIANT
}  // namespace psd
