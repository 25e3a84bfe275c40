/* fpop_wave.h -- wavefront-level operations on piecewise Poisson-loss functions.
 *
 * One gfx950 wavefront (64 lanes) owns one cost function.  A function is a list of pieces
 * in struct-of-arrays form in LDS (an HBM scratch accessor can be plugged into the same
 * templates); lane i works on piece / merged interval i (chunks of 64 for longer lists).
 *
 * These are re-designs, not translations, of the reference's sequential std::list walks
 * (/root/reference/src/funPieceListLog.cpp, "fpl"):
 *   min_less_wave  <- set_to_min_less_of   fpl:236-437
 *   min_more_wave  <- set_to_min_more_of   fpl:439-616
 *   min_env_wave   <- set_to_min_env_of + push_min_pieces + push_piece  fpl:832-860,870-1285
 * Each produces bit-identical lists to the sequential algorithm:
 *   - everything a walk computes about a piece that does not depend on the walk's state
 *     (end costs, argmin, the "search mode" decision) is evaluated by all lanes at once;
 *   - the walk's state machine (search for a minimum / follow a constant) then advances
 *     with ballots; while following a constant every remaining piece tests the crossing
 *     speculatively (root finding in parallel) and the lowest (highest) lane with an event
 *     wins, which is exactly the piece the sequential walk would have stopped at;
 *   - the min-envelope's merged intervals are independent given the two input lists, so
 *     each lane classifies one interval (up to two Newton solves) and emits 1-3 candidate
 *     pieces; candidates are compacted with a ballot/prefix scan.  push_piece's coalescing
 *     compares against the run head with a non-transitive tolerance, so the scan is only
 *     used when every "same function" decision is also a bitwise equality (then comparing
 *     with the predecessor is equivalent); otherwise lane 0 replays the interval list
 *     sequentially (rare; counted in the stats).
 *
 * The three operations return the piece count (>= 0) or -(WERR_* bits).  Each exists as an
 * inline body (*_impl) and an out-of-line wrapper (*_wave): inlining everything -- the LDS
 * and the HBM instantiations, twice -- made a ~200 KB kernel against a 64 KB I-cache, so only
 * the latency build inlines, and only the LDS instantiations (see the end of this file).
 *
 * This file is the umbrella: it checks the variant's macros, includes the parts in order and
 * ends with the out-of-line wrappers.
 *   fpop_lds.h       LDS layout, helper mailbox, profiling macros, list accessors
 *   fpop_walks.h     first pass, min_less_impl, min_more_impl
 *   fpop_envelope.h  interval table, chunk load, classification, compaction (env_compact) --
 *                    each once, for every envelope; min_env_impl and its sequential replay
 *   fpop_coop.h      the helper wave's loop; how two waves share the chunks of an envelope in HBM
 */
#include "fpop_types.h"

/* NO include guard: everything below, and each of the parts, is compiled once per build
 * variant, into namespace psd::PSD_VARIANT.  The includer defines
 *   PSD_VARIANT       namespace of this variant (lat, thr, pk)
 *   PSD_LDS_CAP       pieces per LDS-resident list
 *   PSD_HELPER_WAVES  defined: 4 waves per workgroup (two chains + their helper waves)
 *   PSD_MATH_VK       defined: exp/log with their constants in vector registers */
#if !defined(PSD_VARIANT) || !defined(PSD_LDS_CAP)
#error "define PSD_VARIANT and PSD_LDS_CAP before including fpop_wave.h / fpop_kernels.h"
#endif
#include "fpop_pieces.h"
#include "fpop_lds.h"
#include "fpop_walks.h"
#include "fpop_envelope.h"
#include "fpop_coop.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace psd {
namespace PSD_VARIANT {

/* The three operations, out of line (see the head of this file).  The kernel inlines the
 * LDS instantiations into its loop -- one copy each, ~40 KB of code, and no call overhead
 * (saving and restoring ~40 scalar and ~40 vector registers per call) -- and calls these
 * wrappers for the HBM spill path. */
template <class L, class S>
PSD_NOINLINE int min_less_wave(L in, int n, L out, int cap, S s, int data_i_out,
                               double add_const) {
  MathFull mth;
  return min_less_impl<false>(in, n, out, cap, s, data_i_out, add_const, mth);
}
template <class L, class S>
PSD_NOINLINE int min_more_wave(L in, int n, L out, int cap, S s, int data_i_out) {
  MathFull mth;
  return min_more_impl<false>(in, n, out, cap, s, data_i_out, mth);
}
template <bool HELP, class L, class S>
PSD_NOINLINE int min_env_wave(L f1, int n1, L f2, int n2, L out, int cap, S s, int chain) {
  MathFull mth;
  return min_env_impl<HELP, false>(f1, n1, f2, n2, out, cap, s, chain, mth);
}
/* the same, specialised for n <= 64 (min_env: n1, n2 <= 32): what the throughput build, whose
 * operations all stay out of line, calls for nearly every data point.  Their exp / log come
 * without the rare-argument branches (StepMath): -WERR_SERIAL when such an argument was met,
 * and the caller takes the general version above. */
template <class L, class S>
PSD_NOINLINE int min_less_small_wave(L in, int n, L out, int cap, S s, int data_i_out,
                                     double add_const) {
  MathFast mth;
  const int r = min_less_impl<true>(in, n, out, cap, s, data_i_out, add_const, mth);
  return ballot(mth.rare != 0) ? -WERR_SERIAL : r;
}
template <class L, class S>
PSD_NOINLINE int min_more_small_wave(L in, int n, L out, int cap, S s, int data_i_out) {
  MathFast mth;
  const int r = min_more_impl<true>(in, n, out, cap, s, data_i_out, mth);
  return ballot(mth.rare != 0) ? -WERR_SERIAL : r;
}
template <bool HELP, class L, class S>
PSD_NOINLINE int min_env_small_wave(L f1, int n1, L f2, int n2, L out, int cap, S s, int chain) {
  MathFast mth;
  const int r = min_env_impl<HELP, true>(f1, n1, f2, n2, out, cap, s, chain, mth);
  return ballot(mth.rare != 0) ? -WERR_SERIAL : r;
}

}  // namespace PSD_VARIANT
}  // namespace psd
