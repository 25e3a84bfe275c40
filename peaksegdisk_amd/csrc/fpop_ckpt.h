/* fpop_ckpt.h -- checkpoint slots and the park slot.
 *
 * The slot layout, the overflow pool for functions longer than a slot, saving and loading a
 * chain's function, and the counters of a parked problem.
 *
 * Reached only through fpop_kernels.h: no include guard, compiled once per build variant into
 * namespace psd::PSD_VARIANT. */
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace psd {
namespace PSD_VARIANT {

/* ---- checkpointed store ----------------------------------------
 * Checkpoint slot k of a problem holds the two live functions after data point (k+1) K: per
 * slot 6 + 12 cap doubles {cum_weight, -, overflow offsets of the two chains, interval totals
 * of the two chains (bit patterns), then per chain Lin, Log, Con, mn, mx, prv} and 8 + 2 cap
 * ints {n_up, n_down, data point, max intervals of the two chains, spill steps, sequential
 * envelope replays of the two chains, then per chain data_i}.  The full store keeps ONE such slot per problem: the park slot, written when
 * the arena runs out (park_state) and read back when the problem is resumed.  A function with more than cap pieces lives in the overflow pool (6 n doubles from
 * 6 off, n ints from off) and the slot only holds its offset. */
constexpr int CKPT_HDR_F64 = 6, CKPT_HDR_I32 = 8;
PSD_D size_t ckpt_f64_at(const DeviceArgs &a, long long slot) {
  return (size_t)slot * (CKPT_HDR_F64 + 12 * (size_t)a.ckpt_cap);
}
PSD_D size_t ckpt_i32_at(const DeviceArgs &a, long long slot) {
  return (size_t)slot * (CKPT_HDR_I32 + 2 * (size_t)a.ckpt_cap);
}
PSD_D GlobalList ckpt_list(const DeviceArgs &a, long long slot, int chain) {
  const size_t cap = (size_t)a.ckpt_cap;
  gdouble *f = (gdouble *)(a.ckpt_f64 + ckpt_f64_at(a, slot) + CKPT_HDR_F64 + (size_t)chain * 6 * cap);
  GlobalList r;
  r.Lin_ = f;
  r.Log_ = f + cap;
  r.Con_ = f + 2 * cap;
  r.mn_ = f + 3 * cap;
  r.mx_ = f + 4 * cap;
  r.prv_ = f + 5 * cap;
  r.di_ = (gint *)(a.ckpt_i32 + ckpt_i32_at(a, slot) + CKPT_HDR_I32 + (size_t)chain * cap);
  return r;
}
/* n pieces of the overflow pool from piece offset off */
PSD_D GlobalList ckpt_overflow_list(const DeviceArgs &a, unsigned long long off, int n) {
  gdouble *f = (gdouble *)(a.ckpt_ovf_f64 + (size_t)off * 6);
  const size_t m = (size_t)n;
  GlobalList r;
  r.Lin_ = f;
  r.Log_ = f + m;
  r.Con_ = f + 2 * m;
  r.mn_ = f + 3 * m;
  r.mx_ = f + 4 * m;
  r.prv_ = f + 5 * m;
  r.di_ = (gint *)(a.ckpt_ovf_i32 + (size_t)off);
  return r;
}
/* Room in the overflow pool for the functions of this checkpoint that exceed ckpt_cap (cold:
 * adversarial data only).  Both chain waves call it with the same counts; chain 0 takes the
 * room with one atomic and publishes it.  Returns the offset of the first such function (the
 * up function's if it is one), ~0 when the pool is exhausted -- in both waves alike. */
PSD_COLD_DEV unsigned long long ckpt_take_overflow(const DeviceArgs &a, int chain, int n_up,
                                                   int n_down) {
  chain = uniform_i(chain);
  n_up = uniform_i(n_up);
  n_down = uniform_i(n_down);
  const unsigned long long want = (unsigned long long)(n_up > a.ckpt_cap ? n_up : 0) +
                                  (unsigned long long)(n_down > a.ckpt_cap ? n_down : 0);
  if (chain == 0 && lane_id() == 0) {
    unsigned long long off = atomicAdd(a.ckpt_ovf_next, want);
    g_sm.ckpt_ovf = off + want <= a.ckpt_ovf_cap ? off : ~0ull;
  }
  block_sync(chain);
  const unsigned long long off = psd_d2u(uniform_d(psd_u2d(g_sm.ckpt_ovf)));
  block_sync(chain); /* the word is free again before anyone can come back here */
  return off;
}
/* this chain's function (list `id`, n pieces, in LDS or in the problem's slot of the HBM spill
 * pool) and the cumulated weight -> checkpoint k; ovf: this chain's room in the overflow pool
 * when n > ckpt_cap */
PSD_COLD_DEV void ckpt_save(const DeviceArgs &a, int p, int k, int chain, int id, int n,
                            double cum_weight, int in_hbm, int spill_slot, unsigned long long ovf) {
  p = uniform_i(p);
  k = uniform_i(k);
  chain = uniform_i(chain);
  n = uniform_i(n);
  id = uniform_i(id);
  spill_slot = uniform_i(spill_slot);
  ovf = psd_d2u(uniform_d(psd_u2d(ovf)));
  const long long slot = a.prob_ckpt_off[p] + k;
  const GlobalList dst = n > a.ckpt_cap ? ckpt_overflow_list(a, ovf, n) : ckpt_list(a, slot, chain);
  if (uniform_i(in_hbm)) {
    copy_list_wave(global_list(a, spill_slot, id), n, dst);
  } else {
    copy_list_wave(lds_list(id), n, dst);
  }
  if (lane_id() == 0) {
    a.ckpt_i32[ckpt_i32_at(a, slot) + (size_t)chain] = n;
    a.ckpt_f64[ckpt_f64_at(a, slot) + 2 + (size_t)chain] = psd_u2d(ovf);
    if (chain == 0) a.ckpt_f64[ckpt_f64_at(a, slot)] = uniform_d(cum_weight);
  }
}
/* piece count of a chain's function in checkpoint k */
PSD_COLD_DEV int ckpt_count(const DeviceArgs &a, int p, int k, int chain) {
  const long long slot = a.prob_ckpt_off[uniform_i(p)] + uniform_i(k);
  return uniform_i(a.ckpt_i32[ckpt_i32_at(a, slot) + (size_t)uniform_i(chain)]);
}
/* checkpoint k -> list `id` (LDS, or the problem's spill slot when to_hbm); returns the piece
 * count */
PSD_COLD_DEV int ckpt_load(const DeviceArgs &a, int p, int k, int chain, int id, int to_hbm,
                           int spill_slot) {
  p = uniform_i(p);
  k = uniform_i(k);
  chain = uniform_i(chain);
  id = uniform_i(id);
  spill_slot = uniform_i(spill_slot);
  const long long slot = a.prob_ckpt_off[p] + k;
  const int n = uniform_i(a.ckpt_i32[ckpt_i32_at(a, slot) + (size_t)chain]);
  const unsigned long long ovf =
      psd_d2u(uniform_d(a.ckpt_f64[ckpt_f64_at(a, slot) + 2 + (size_t)chain]));
  const GlobalList src = n > a.ckpt_cap ? ckpt_overflow_list(a, ovf, n) : ckpt_list(a, slot, chain);
  if (uniform_i(to_hbm)) {
    copy_list_wave(src, n, global_list(a, spill_slot, id));
  } else {
    copy_list_wave(src, n, lds_list(id));
  }
  return n;
}
PSD_COLD_DEV double ckpt_cum_weight(const DeviceArgs &a, int p, int k) {
  const long long slot = a.prob_ckpt_off[uniform_i(p)] + uniform_i(k);
  return a.ckpt_f64[ckpt_f64_at(a, slot)];
}
/* what a parked problem needs besides its two functions (slot 0 of the problem) */
PSD_COLD_DEV void park_counters_save(const DeviceArgs &a, int p, int chain, int t,
                                     unsigned long long total_intervals, int max_intervals,
                                     int spill_steps) {
  const long long slot = a.prob_ckpt_off[uniform_i(p)];
  chain = uniform_i(chain);
  if (lane_id() == 0) {
    a.ckpt_f64[ckpt_f64_at(a, slot) + 4 + (size_t)chain] = psd_u2d(total_intervals);
    a.ckpt_i32[ckpt_i32_at(a, slot) + 3 + (size_t)chain] = max_intervals;
    a.ckpt_i32[ckpt_i32_at(a, slot) + 6 + (size_t)chain] = g_sm.serial[chain];
    if (chain == 1) {
      a.ckpt_i32[ckpt_i32_at(a, slot) + 2] = t;
      a.ckpt_i32[ckpt_i32_at(a, slot) + 5] = spill_steps;
    }
  }
}
PSD_COLD_DEV unsigned long long park_total_intervals(const DeviceArgs &a, int p, int chain) {
  const long long slot = a.prob_ckpt_off[uniform_i(p)];
  return psd_d2u(uniform_d(a.ckpt_f64[ckpt_f64_at(a, slot) + 4 + (size_t)uniform_i(chain)]));
}
PSD_COLD_DEV int park_int(const DeviceArgs &a, int p, int which) {
  const long long slot = a.prob_ckpt_off[uniform_i(p)];
  return uniform_i(a.ckpt_i32[ckpt_i32_at(a, slot) + (size_t)uniform_i(which)]);
}

}  // namespace PSD_VARIANT
}  // namespace psd
