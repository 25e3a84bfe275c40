/* fpop_sync.h -- where the waves of a workgroup meet.
 *
 * The workgroup barrier that a helper wave mirrors (block_sync), the barrier at the end of every
 * data point between the two chain waves (step_sync), and taking the problem's slot of the HBM
 * spill pool, which both chain waves do together.
 *
 * Reached only through fpop_kernels.h: no include guard, compiled once per build variant into
 * namespace psd::PSD_VARIANT. */
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace psd {
namespace PSD_VARIANT {

#ifdef PSD_HELPER_WAVES
constexpr bool USE_HELPER = true;
constexpr int FORWARD_THREADS = 256; /* waves 0,1: the two chains; waves 2,3: their helpers */
/* every workgroup barrier of a main wave is mirrored by its helper */
PSD_D void block_sync(int chain) {
  if (!mail_wait(chain)) {
    if (lane_id() == 0) g_sm.mail[chain].abort = 1;
  }
  mail_post(chain, HOP_BARRIER);
  __syncthreads();
}
#else
constexpr bool USE_HELPER = false;
constexpr int FORWARD_THREADS = 128;
PSD_D void block_sync(int) { __syncthreads(); }
#endif

/* the workgroup barrier as a call (cold paths inside the kernel's loop) */
PSD_COLD_DEV void block_sync_cold(int chain) { block_sync(uniform_i(chain)); }

/* The barrier at the end of every data point, between the two chain waves only.
 * PSD_FLAG_BARRIER (latency build): each wave publishes the barrier's number in LDS and polls
 * the other's -- no s_barrier, and the helper waves, which never touch the lists, stay out of
 * it (waking them through their mailbox for every data point cost more than the data point's
 * imbalance).  Returns false if the other wave never came (never expected: the caller
 * aborts the problem).  Otherwise the workgroup barrier. */
PSD_D bool step_sync(int chain, unsigned seq) {
#ifdef PSD_FLAG_BARRIER
  constexpr int SPIN_LIMIT = WAIT_SPIN_LIMIT; /* seconds */
  wave_sync();
  if (lane_id() == 0) flag_store((int *)&g_sm.arrived[chain], (int)seq);
  for (int spin = 0; spin < SPIN_LIMIT; spin++) {
    /* lane 0's reading decides for the wave */
    if (rdlane_i(flag_load((int *)&g_sm.arrived[1 - chain]), 0) - (int)seq >= 0) {
      PSD_SPIN_NOTE(spin);
      return true;
    }
    spin_pause();
  }
  return false;
#else
  (void)seq;
  block_sync(chain);
  return true;
#endif
}

/* Take a slot of the HBM spill pool for this workgroup's problem (cold: at most once per
 * problem).  Both chain waves call it; returns the slot, or -1 when the pool is exhausted. */
PSD_COLD_DEV int take_spill_slot(const DeviceArgs &a, int chain) {
  chain = uniform_i(chain);
  if (chain == 0 && lane_id() == 0) {
    int sl = atomicAdd(a.spill_next, 1);
    g_sm.spill_slot = sl < a.spill_slots ? sl : -1;
  }
  block_sync(chain);
  return uniform_i(g_sm.spill_slot);
}

}  // namespace PSD_VARIANT
}  // namespace psd
