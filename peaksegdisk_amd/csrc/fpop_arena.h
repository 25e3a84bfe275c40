/* fpop_arena.h -- the in-HBM arena of backtrack records, and what touches a whole function
 * once per data point.
 *
 * Where a record lives (ArenaPtr), a wave's current run of chunks (ArenaCursor), taking the
 * next run, appending a function's record, the fused rescale + append that ends every step
 * (scale_add_store_wave) and Minimize.
 *
 * Reached only through fpop_kernels.h: no include guard, compiled once per build variant into
 * namespace psd::PSD_VARIANT. */
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace psd {
namespace PSD_VARIANT {

/* where piece offset `off` of the arena lives (a.ar_block[] must hold the block already) */
struct ArenaPtr {
  gdouble *mx, *prv;
  gint *di;
};
PSD_D ArenaPtr arena_ptr(char *block_base, int block_log2, unsigned long long within) {
  ArenaPtr r;
  r.mx = (gdouble *)block_base + within;
  r.prv = (gdouble *)(block_base + (8ull << block_log2)) + within;
  r.di = (gint *)(block_base + (16ull << block_log2)) + within;
  return r;
}
PSD_D ArenaPtr arena_at(const DeviceArgs &a, unsigned long long off) {
  const int blg = a.ar_block_log2;
  /* (every lane loads the same entry: the address is wave-uniform, say so) */
  return arena_ptr(uniform_p(agent_load_ptr(&a.ar_block[off >> blg])), blg,
                   off & ((1ull << blg) - 1ull));
}

/* The three addresses of the current chunk run are needed once per data point, by the lanes
 * that store the record: they live in LDS (g_sm.cur_ptr: one broadcast read next to the reads of
 * the record itself), not in six scalar registers that the whole loop would carry -- the latency
 * build spills scalar registers as it is (cursor in registers: 2172 ms, in LDS: 2120 ms on
 * 200 k bins x 64, profiles/r04/ab_cursor_in_lds_packed_flag_newton_trim.log). */
struct ArenaCursor {
  unsigned long long base; /* first piece of the current chunk run */
  int used, room;
  int store; /* 0: the forward pass of the checkpointed store keeps no per-step records */
};
PSD_D void cursor_clear(ArenaCursor &cur, int store) {
  cur.base = 0;
  cur.used = 0;
  cur.room = 0;
  cur.store = store;
}
PSD_D void cursor_point(const DeviceArgs &a, ArenaCursor &cur, unsigned long long base, int room) {
  const ArenaPtr q = arena_at(a, base);
  wave_sync();
  if (lane_id() == 0) {
    g_sm.cur_ptr[wave_id() & 1][0] = (unsigned long long)q.mx;
    g_sm.cur_ptr[wave_id() & 1][1] = (unsigned long long)q.prv;
    g_sm.cur_ptr[wave_id() & 1][2] = (unsigned long long)q.di;
  }
  wave_sync();
  cur.base = base;
  cur.used = 0;
  cur.room = room;
}
PSD_D gdouble *cursor_mx() { return (gdouble *)g_sm.cur_ptr[wave_id() & 1][0]; }
PSD_D gdouble *cursor_prv() { return (gdouble *)g_sm.cur_ptr[wave_id() & 1][1]; }
PSD_D gint *cursor_di() { return (gint *)g_sm.cur_ptr[wave_id() & 1][2]; }

/* Reserve arena room for a function of n pieces: the next run of whole chunks for this wave
 * (cold: once per chunk of 2^ar_chunk_log2 pieces), inside ONE block.  Returns the first piece
 * index of the run; ~0 when the arena is exhausted.  A run beyond what was mapped at launch
 * waits for the host, which maps ahead of ar_used while the kernel runs; the arena is exhausted
 * when the host says that no more will come (or never answers). */
PSD_COLD_DEV unsigned long long arena_take(const DeviceArgs &a, int n) {
  if (a.ckpt_interval > 0) return ~0ull; /* checkpointed store: the wave's region is all it has */
  const int lg = a.ar_chunk_log2, blg = a.ar_block_log2;
  const unsigned long long chunks = ((unsigned long long)uniform_i(n) + (1ull << lg) - 1ull) >> lg;
  if ((chunks << lg) > (1ull << blg)) return ~0ull; /* (a function is never longer than a block) */
  /* How long a wave waits for the host to map a block: a block is 10-340 MB at 13-35 ms per GB,
   * so a fifth of a second is generous -- and it must stay far below the bound on the waits
   * BETWEEN waves (WAIT_SPIN_LIMIT, seconds): the other chain's wave sits at the data point's
   * barrier meanwhile.  Past it the problem is parked, which costs a relaunch, not a result. */
  constexpr long long LIVE_WAIT_CYCLES = 480000000ll; /* 0.2 s at 2.4 GHz */
  constexpr int LIVE_SPIN_LIMIT = 1 << 22; /* (the emulator has no clock: polls) */
  for (;;) {
    unsigned long long first = 0;
    if (lane_id() == 0) {
      first = atomicAdd(a.ar_next_chunk, chunks);
      if (a.ar_used) sys_add_u64(a.ar_used, chunks << lg);
    }
    first = psd_d2u(rdlane_d(psd_u2d(first), 0));
    const unsigned long long lo = first << lg, hi = (first + chunks) << lg;
    if ((lo >> blg) != ((hi - 1ull) >> blg)) continue; /* straddles two blocks: the next run */
    if (hi > a.ar_cap) {
      if (a.ar_live == nullptr) return ~0ull;
      bool mapped = false;
      const long long t_wait = cycle_now();
      for (int spin = 0; spin < LIVE_SPIN_LIMIT; spin++) {
        /* (the flag first: a capacity published before it is final) */
        const unsigned long long final_now = psd_d2u(uniform_d(psd_u2d(sys_load_u64(&a.ar_live[1]))));
        const unsigned long long cap_now = psd_d2u(uniform_d(psd_u2d(sys_load_u64(&a.ar_live[0]))));
        if (hi <= cap_now) {
          mapped = true;
          break;
        }
        if (final_now || cycle_now() - t_wait > LIVE_WAIT_CYCLES) break;
        host_pause();
      }
      if (!mapped) return ~0ull;
      /* a block the host added during this launch: its address goes into the device table */
      const unsigned long long blk = lo >> blg;
      if (lane_id() == 0)
        agent_store_ptr(&a.ar_block[blk], (char *)sys_load_u64(&a.ar_live[2ull + blk]));
      wave_sync();
    }
    return lo;
  }
}
PSD_D int arena_room_for(const DeviceArgs &a, int n) {
  const int lg = a.ar_chunk_log2;
  return (int)((((unsigned)n + (1u << lg) - 1u) >> lg) << lg);
}
/* the next run of chunks for a function of n pieces -> cursor; false when the arena is full */
PSD_D bool cursor_take(const DeviceArgs &a, ArenaCursor &cur, int n) {
  unsigned long long base = psd_d2u(uniform_d(psd_u2d(arena_take(*a.self, n))));
  if (base == ~0ull) return false;
  cursor_point(a, cur, base, arena_room_for(a, n));
  return true;
}

/* Append one function's backtrack record to the arena; returns false when it is full. */
template <class L>
PSD_D bool arena_store_wave(const DeviceArgs &a, ArenaCursor &cur, const L &f, int n,
                            unsigned long long fn_index) {
  const int lane = lane_id();
  if (!cur.store) return true;
  if (n > cur.room - cur.used && !cursor_take(a, cur, n)) return false;
  const int at = cur.used;
  for (int base = 0; base < n; base += WAVE) {
    int i = base + lane;
    if (i < n) {
      cursor_mx()[at + i] = f.mx(i);
      cursor_prv()[at + i] = f.prv(i);
      cursor_di()[at + i] = f.di(i);
    }
  }
  if (lane == 0)
    ((gull *)a.fn_ref)[fn_index] =
        ((cur.base + (unsigned long long)at) << FN_COUNT_BITS) | (unsigned long long)n;
  cur.used += n;
  return true;
}

/* Last phase of a step, fused: f <- (f * W_{t-1} + (w, -z w, 0)) * (1/W_t)  (drv:316-321 /
 * 365-370: multiply, add, multiply, no contraction) and the function's backtrack record
 * {max_log_mean, data_i, prev_log_mean} appended to the arena, each piece touched once.
 * Returns false when the arena is full. */
template <class L>
PSD_D bool scale_add_store_wave(const DeviceArgs &a, ArenaCursor &cur, const L &f, int n,
                                unsigned long long fn_index, bool store, double cum_weight_prev,
                                double add_linear, double add_log, double inv_cum_weight) {
  const int lane = lane_id();
  bool ok = true;
  store = store && cur.store != 0;
  if (store && n > cur.room - cur.used && !cursor_take(a, cur, n)) {
    ok = false;
    store = false;
  }
  const int at = cur.used;
  for (int base = 0; base < n; base += WAVE) {
    int i = base + lane;
    if (i < n) {
      double li = f.Lin(i) * cum_weight_prev;
      double lo = f.Log(i) * cum_weight_prev;
      double co = f.Con(i) * cum_weight_prev;
      double mx = f.mx(i), prv = f.prv(i);
      int di = f.di(i);
      li = li + add_linear;
      lo = lo + add_log;
      co = co + 0.0;
      f.Lin(i) = li * inv_cum_weight;
      f.Log(i) = lo * inv_cum_weight;
      f.Con(i) = co * inv_cum_weight;
      if (store) {
        cursor_mx()[at + i] = mx;
        cursor_prv()[at + i] = prv;
        cursor_di()[at + i] = di;
      }
    }
  }
  if (store) {
    if (lane == 0)
      ((gull *)a.fn_ref)[fn_index] =
          ((cur.base + (unsigned long long)at) << FN_COUNT_BITS) | (unsigned long long)n;
    cur.used += n;
  }
  return ok;
}

/* Minimize (fpl:689-712): first strict minimum over pieces of the clamped optimum. */
template <class L>
PSD_D void minimize_wave(const L &f, int n, double *best_cost, double *best_log_mean,
                         int *data_i, double *prev_log_mean) {
  const int lane = lane_id();
  double bc = PSD_INF, blm = 0.0, bprv = 0.0;
  int bdi = 0;
  for (int base = 0; base < n; base += WAVE) {
    int i = base + lane;
    double cost = PSD_INF, lm = 0.0;
    if (i < n) {
      Coef c = load_coef(f, i);
      lm = argmin(c);
      if (lm < f.mn(i)) {
        lm = f.mn(i);
      } else if (f.mx(i) < lm) {
        lm = f.mx(i);
      }
      cost = get_cost(c, lm);
    }
    /* lowest lane among those holding the chunk minimum; NaN never wins a strict '<' */
    bool usable = i < n && cost < PSD_INF;
    double v = usable ? cost : PSD_INF;
    double mn = v;
    for (int sft = 1; sft < WAVE; sft <<= 1) {
      double o = shfl_d(mn, lane ^ sft);
      mn = o < mn ? o : mn;
    }
    unsigned long long m = ballot(usable && v == mn);
    if (m && mn < bc) {
      int src = ctz64(m);
      bc = mn;
      blm = rdlane_d(lm, src);
      int ii = base + src;
      bdi = f.di(ii);
      bprv = f.prv(ii);
    }
  }
  *best_cost = bc;
  *best_log_mean = blm;
  *data_i = bdi;
  *prev_log_mean = bprv;
}

}  // namespace PSD_VARIANT
}  // namespace psd
