/* fpop_lds.h -- where a workgroup's piece lists live and how they are reached.
 *
 * The LDS layout (ListStore, ScratchStore, SharedBlock, g_sm), the helper waves' mailbox with its
 * bounded waits, the profiling macros, the four accessors (a list / a wave's scratch arrays, in
 * LDS / in HBM) that every wave operation is a template over, and copying a list.
 *
 * Reached only through fpop_wave.h: no include guard, compiled once per build variant into
 * namespace psd::PSD_VARIANT. */
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace psd {
namespace PSD_VARIANT {

constexpr int LDS_CAP = PSD_LDS_CAP; /* pieces per LDS-resident list */

/* one piece list, struct-of-arrays (fields of funPieceListLog.h:11-34) */
struct ListStore {
  double Lin[LDS_CAP], Log[LDS_CAP], Con[LDS_CAP], mn[LDS_CAP], mx[LDS_CAP], prv[LDS_CAP];
  int di[LDS_CAP];
};
/* per-wave temporaries, one slot per input piece / merged interval */
struct ScratchStore {
  double lc[LDS_CAP], rc[LDS_CAP];   /* getCost at the piece's left / right end */
  double om[LDS_CAP], mu[LDS_CAP];   /* argmin_mean(), argmin() */
  double muc[LDS_CAP], oc2[LDS_CAP]; /* getCost(argmin()), PoissonLoss(argmin_mean()) */
  int cls[LDS_CAP];
  int iv[2 * LDS_CAP];
};
/* Helper waves (PSD_HELPER_WAVES): every chain's main wave has a second wave that runs the
 * longest dependent chain of the envelope classification concurrently: given the difference
 * piece of every interval (HOP_ROOT, posted as soon as it is formed), it derives the optimum
 * and has_two_roots itself and does the larger-root Newton solves, while the main wave
 * evaluates end costs, midpoint and the smaller-root solves.  Lane k of the helper works on
 * lane k's interval; arguments and results cross through this LDS mailbox.  HOP_BARRIER makes
 * the helper join a workgroup barrier, HOP_EXIT ends it. */
enum {
  HOP_BARRIER = 1, HOP_EXIT = 2, HOP_ROOT = 3,
  /* lists in HBM (functions that outgrew LDS: adversarial data): the helper takes every
   * second chunk of 64 pieces / merged intervals of the chain wave's operation */
  HOP_HBM_COSTS = 4,    /* first pass of min-less / min-more: the odd chunks */
  HOP_HBM_TABLE = 5,    /* merged-interval table: the entries owned by the second function */
  HOP_HBM_CLASSIFY = 6, /* envelope classification: the odd chunks, results left in HBM */
};
struct Mail {
  int seq_cmd, seq_done, op, abort;
  int h_arg[8];   /* arguments of the HBM operations */
  int h_progress; /* HOP_HBM_CLASSIFY: chunks the helper has finished (a flag) */
  int flags[64];
  double d_lin[64], d_log[64], d_con[64], b[64]; /* HOP_ROOT: difference piece, right end */
  double res_large[64];
};

/* the workgroup's LDS: lists 0,1 = up (double-buffered), 2,3 = down, 4,5 = per-wave
 * min-less / min-more result */
struct SharedBlock {
  ListStore list[6];
  ScratchStore sc[2];
  unsigned arrived[2]; /* number of the last end-of-data-point barrier the chain wave reached */
  int n[6];
  int abort_status[3];
  int abort_err[3];
  unsigned long long total_up;
  int max_up;
  int serial[2];
  int spill_slot; /* slot of the HBM spill pool taken by this problem (take_spill_slot) */
  int bt_next;    /* checkpointed store: block the decoding needs next, -1 = done */
  unsigned long long ckpt_ovf; /* checkpointed store: room taken in the overflow pool */
#ifdef PSD_HELPER_WAVES
  Mail mail[2];
#endif
#ifdef PSD_PROFILE
  long long prof[4][N_PROF];
#endif
#ifdef PSD_SPIN_STATS
  int spin_max[4];
#endif
#ifdef PSD_LOOP_STATS
  int loop_stats[2][3]; /* per chain: data points inside the inner loop, general, entries */
#endif
  long long t_begin[2];             /* cycle counter at the start of each chain wave */
  unsigned long long cur_ptr[2][3]; /* where each chain's current arena run lives (ArenaCursor) */
};

PSD_LDS SharedBlock g_sm;

/* Waits between the waves of a workgroup (the flag barrier of a data point, the helper
 * mailboxes, the progress word of a shared envelope) poll an LDS word at most this many times:
 * a wave that never comes turns into an error status instead of a hang.  A poll with its pause
 * is ~100 cycles, so the bound is seconds; the slowest legitimate wait is four orders of
 * magnitude shorter (tests/test_gpu_round4.py measures it with -DPSD_SPIN_STATS). */
constexpr int WAIT_SPIN_LIMIT = 1 << 26;
#ifdef PSD_SPIN_STATS
#define PSD_SPIN_NOTE(spin)                                                           \
  do {                                                                                \
    if (lane_id() == 0 && (spin) > g_sm.spin_max[wave_id()]) g_sm.spin_max[wave_id()] = (spin); \
  } while (0)
#else
#define PSD_SPIN_NOTE(spin) \
  do {                      \
  } while (0)
#endif
#ifdef PSD_HELPER_WAVES
constexpr int MAIL_SPIN_LIMIT = WAIT_SPIN_LIMIT;
/* main wave: wait until the helper has finished the last posted command */
PSD_D bool mail_wait(int chain) {
  Mail &m = g_sm.mail[chain];
  const int want = flag_load(&m.seq_cmd);
  for (int spin = 0; spin < MAIL_SPIN_LIMIT; spin++) {
    if (flag_load(&m.seq_done) == want) {
      PSD_SPIN_NOTE(spin);
      return true;
    }
    spin_pause();
  }
  return false;
}
/* main wave: hand the next command over (arguments already written by the lanes) */
PSD_D void mail_post(int chain, int op) {
  Mail &m = g_sm.mail[chain];
  wave_sync();
  if (lane_id() == 0) {
    m.op = op;
    flag_store(&m.seq_cmd, flag_load(&m.seq_cmd) + 1);
  }
  wave_sync(); /* no lane reads seq_cmd (mail_wait) before lane 0 has advanced it */
}
#endif

#ifdef PSD_PROFILE
#define PSD_PROF_T0()                \
  long long prof_t0_ = cycle_now(); \
  long long prof_sub_ = prof_t0_;   \
  (void)prof_sub_
#define PSD_PROF_ADD(slot)                                             \
  do {                                                                 \
    long long now_ = cycle_now();                                      \
    if (lane_id() == 0) g_sm.prof[wave_id()][slot] += now_ - prof_t0_; \
    prof_t0_ = now_;                                                   \
  } while (0)
#define PSD_PROF_SUB0() prof_sub_ = cycle_now()
#define PSD_PROF_SUB(slot)                                              \
  do {                                                                  \
    long long now_ = cycle_now();                                       \
    if (lane_id() == 0) g_sm.prof[wave_id()][slot] += now_ - prof_sub_; \
    prof_sub_ = now_;                                                   \
  } while (0)
#else
#define PSD_PROF_SUB0() \
  do {                  \
  } while (0)
#define PSD_PROF_SUB(slot) \
  do {                     \
  } while (0)
#define PSD_PROF_T0() \
  do {                \
  } while (0)
#define PSD_PROF_ADD(slot) \
  do {                     \
  } while (0)
#endif
enum {
  PROF_PRE = 0, PROF_WALK = 1, PROF_TABLE = 2, PROF_CLASSIFY = 3, PROF_COMPACT = 4,
  PROF_SCALE = 5, PROF_ARENA = 6, PROF_BARRIER = 7, PROF_SERIAL = 8, PROF_TOTAL = 9,
  PROF_C_LOAD = 10, PROF_C_MID = 11, PROF_C_OPT = 12, PROF_C_SMALL = 13, PROF_C_LARGE = 14,
  PROF_C_TAIL = 15,
  PROF_IT_SPEC = 16, PROF_IT_SMALL = 17, PROF_IT_LARGE = 18, /* wave-level Newton trip counts */
  PROF_IT_ROUNDS = 19, /* walk state-machine rounds */
  PROF_S_ASSIGN = 20, PROF_S_LOAD = 21, PROF_S_NEWTON = 22 /* inside the speculation round */
};
#ifdef PSD_PROFILE
#define PSD_PROF_ITERS(slot, steps)                                 \
  do {                                                              \
    int m_ = 0;                                                     \
    while (ballot((steps) > m_)) m_++;                              \
    if (lane_id() == 0) g_sm.prof[wave_id()][slot] += m_;           \
  } while (0)
#else
#define PSD_PROF_ITERS(slot, steps) \
  do {                             \
  } while (0)
#endif
#ifdef PSD_PROFILE
#define PSD_PROF_COUNT(slot)                                       \
  do {                                                             \
    if (lane_id() == 0) g_sm.prof[wave_id()][slot] += 1;           \
  } while (0)
#else
#define PSD_PROF_COUNT(slot) \
  do {                       \
  } while (0)
#endif

/* accessor of an LDS-resident list: g_sm.list[id], elements off.. */
struct LdsList {
  static constexpr bool in_lds = true;
  int id, off;
  PSD_M double &Lin(int i) const { return g_sm.list[id].Lin[off + i]; }
  PSD_M double &Log(int i) const { return g_sm.list[id].Log[off + i]; }
  PSD_M double &Con(int i) const { return g_sm.list[id].Con[off + i]; }
  PSD_M double &mn(int i) const { return g_sm.list[id].mn[off + i]; }
  PSD_M double &mx(int i) const { return g_sm.list[id].mx[off + i]; }
  PSD_M double &prv(int i) const { return g_sm.list[id].prv[off + i]; }
  PSD_M int &di(int i) const { return g_sm.list[id].di[off + i]; }
  PSD_M LdsList shifted(int d) const {
    LdsList r;
    r.id = id;
    r.off = off + d;
    return r;
  }
  /* Arguments of out-of-line device functions arrive in VGPRs and the compiler must assume
   * they differ between lanes: every loop and branch on them becomes an exec-mask loop.  They
   * are wave-uniform by construction; readfirstlane says so. */
  PSD_M LdsList uniformed() const {
    LdsList r;
    r.id = uniform_i(id);
    r.off = uniform_i(off);
    return r;
  }
};
/* accessor of a wave's LDS scratch arrays */
struct LdsScratch {
  int w;
  PSD_M double &lc(int i) const { return g_sm.sc[w].lc[i]; }
  PSD_M double &rc(int i) const { return g_sm.sc[w].rc[i]; }
  PSD_M double &om(int i) const { return g_sm.sc[w].om[i]; }
  PSD_M double &mu(int i) const { return g_sm.sc[w].mu[i]; }
  PSD_M double &muc(int i) const { return g_sm.sc[w].muc[i]; }
  PSD_M double &oc2(int i) const { return g_sm.sc[w].oc2[i]; }
  PSD_M int &cls(int i) const { return g_sm.sc[w].cls[i]; }
  PSD_M int &iv(int i) const { return g_sm.sc[w].iv[i]; }
  PSD_M int iv_cap() const { return 2 * LDS_CAP; }
  PSD_M LdsScratch uniformed() const {
    LdsScratch r;
    r.w = uniform_i(w);
    return r;
  }
};

/* The same two accessors over HBM: the spill path for functions with more than LDS_CAP
 * pieces (adversarial data, vignettes/Worst_case.Rmd).  `cap` pieces per list. */
struct GlobalList {
  static constexpr bool in_lds = false;
  gdouble *Lin_, *Log_, *Con_, *mn_, *mx_, *prv_;
  gint *di_;
  PSD_M gdouble &Lin(int i) const { return Lin_[i]; }
  PSD_M gdouble &Log(int i) const { return Log_[i]; }
  PSD_M gdouble &Con(int i) const { return Con_[i]; }
  PSD_M gdouble &mn(int i) const { return mn_[i]; }
  PSD_M gdouble &mx(int i) const { return mx_[i]; }
  PSD_M gdouble &prv(int i) const { return prv_[i]; }
  PSD_M gint &di(int i) const { return di_[i]; }
  PSD_M GlobalList shifted(int d) const {
    GlobalList r;
    r.Lin_ = Lin_ + d;
    r.Log_ = Log_ + d;
    r.Con_ = Con_ + d;
    r.mn_ = mn_ + d;
    r.mx_ = mx_ + d;
    r.prv_ = prv_ + d;
    r.di_ = di_ + d;
    return r;
  }
  PSD_M GlobalList uniformed() const {
    GlobalList r;
    r.Lin_ = uniform_p(Lin_);
    r.Log_ = uniform_p(Log_);
    r.Con_ = uniform_p(Con_);
    r.mn_ = uniform_p(mn_);
    r.mx_ = uniform_p(mx_);
    r.prv_ = uniform_p(prv_);
    r.di_ = uniform_p(di_);
    return r;
  }
};
struct GlobalScratch {
  gdouble *lc_, *rc_, *om_, *mu_, *muc_, *oc2_;
  gint *cls_, *iv_;
  int iv_cap_;
  PSD_M gdouble &lc(int i) const { return lc_[i]; }
  PSD_M gdouble &rc(int i) const { return rc_[i]; }
  PSD_M gdouble &om(int i) const { return om_[i]; }
  PSD_M gdouble &mu(int i) const { return mu_[i]; }
  PSD_M gdouble &muc(int i) const { return muc_[i]; }
  PSD_M gdouble &oc2(int i) const { return oc2_[i]; }
  PSD_M gint &cls(int i) const { return cls_[i]; }
  PSD_M gint &iv(int i) const { return iv_[i]; }
  PSD_M int iv_cap() const { return iv_cap_; }
  /* Results of merged intervals classified by the helper wave (HOP_HBM_CLASSIFY), one slot per
   * interval (up to 2 cap of them): the six cost arrays are contiguous in pairs (lc|rc, om|mu,
   * muc|oc2, fpop_step.h global_scratch) and dead once the walk is over. */
  PSD_M gdouble &coop_x1(int k) const { return lc_[k]; }
  PSD_M gdouble &coop_x2(int k) const { return om_[k]; }
  PSD_M gdouble &coop_code(int k) const { return muc_[k]; }
  PSD_M GlobalScratch uniformed() const {
    GlobalScratch r;
    r.lc_ = uniform_p(lc_);
    r.rc_ = uniform_p(rc_);
    r.om_ = uniform_p(om_);
    r.mu_ = uniform_p(mu_);
    r.muc_ = uniform_p(muc_);
    r.oc2_ = uniform_p(oc2_);
    r.cls_ = uniform_p(cls_);
    r.iv_ = uniform_p(iv_);
    r.iv_cap_ = uniform_i(iv_cap_);
    return r;
  }
};

PSD_D LdsList lds_list(int id) {
  LdsList r;
  r.id = id;
  r.off = 0;
  return r;
}

template <class L>
PSD_D Coef load_coef(const L &f, int i) {
  Coef c;
  c.Linear = f.Lin(i);
  c.Log = f.Log(i);
  c.Constant = f.Con(i);
  return c;
}

template <class L>
PSD_D void store_piece(const L &f, int i, const Coef &c, double mn, double mx, int di,
                       double prv) {
  f.Lin(i) = c.Linear;
  f.Log(i) = c.Log;
  f.Con(i) = c.Constant;
  f.mn(i) = mn;
  f.mx(i) = mx;
  f.di(i) = di;
  f.prv(i) = prv;
}

/* n pieces from one list to another, in LDS or in HBM each */
template <class LS, class LD>
PSD_D void copy_list_wave(const LS &src, int n, const LD &dst) {
  const int lane = lane_id();
  for (int base = 0; base < n; base += WAVE) {
    int i = base + lane;
    if (i < n)
      store_piece(dst, i, load_coef(src, i), src.mn(i), src.mx(i), src.di(i), src.prv(i));
  }
}

}  // namespace PSD_VARIANT
}  // namespace psd
