/* reads_pileup.h -- coverage from aligned reads on the device: every read (chromStart, chromEnd,
 * count) adds +count where it starts and -count where it ends to a zeroed int32 buffer with one
 * slot per base of its contig's extent [lo, hi), and an inclusive prefix sum turns the differences
 * into the coverage, in place.  dense_encode.h reads that buffer where it lies.
 *
 * Four launches per call, however many contigs it has, and no workgroup ever waits for another:
 *   scatter_kernel    a workgroup per slice of SLICE reads of one contig, a read per lane.  A read
 *                     with start >= end or a negative count is bad and adds nothing; a good one is
 *                     clipped to the extent: +count at max(start, lo) - lo, -count at end - lo when
 *                     end < hi (beyond hi there is no slot and none is needed); one that misses the
 *                     extent adds nothing.  With last_base_only the read stands for [end - 1, end).
 *                     Both adds are no-return 32-bit atomics.  The workgroup reduces the sum of its
 *                     good counts and the index of its first bad read and sends them to the
 *                     contig's 16-byte record by one 64-bit add and one 64-bit max
 *                     (key = ~index: the smaller index wins, 0 = none).
 *   tile_sum_kernel   a workgroup per tile of dense::TILE bases (the encoder's tiling: a tile never
 *                     crosses a contig): the sum of the tile's differences
 *   tile_scan_kernel  a workgroup per contig: exclusive scan of its tile sums, the coverage in front
 *                     of each tile
 *   apply_kernel      a workgroup per tile again: inclusive prefix sum of the tile in place, lane-
 *                     local over four elements, wave scan by shuffles, wave offsets through LDS, plus
 *                     the tile's carry
 * between the first and the second the host downloads the records and refuses a bad read or a
 * contig whose good counts sum to 2^31 or more.  Below that every prefix of a contig's differences
 * is a coverage value in [0, sum of counts]: int32 holds it, and the difference of two of them
 * (a tile's sum, which may be negative) as well.  Sums of several such differences are formed in
 * unsigned arithmetic, which wraps and ends at the right value.
 * Algorithmic traffic for n reads and B bases: 8 n bytes of reads (12 n with counts), 2 atomics
 * per read, 4 B zeroed, 4 B read by tile_sum_kernel, 4 B read and 4 B written by apply_kernel.
 *
 * Every contig's slots begin at a multiple of 16 bytes and are padded with zeros to a multiple of
 * four, so that every lane loads and stores 16 aligned bytes.  Integer adds commute: the result
 * does not depend on the schedule.  Written against psd_platform.h only: the SIMT emulator of
 * tests/emu runs this source. */
#ifndef PSD_READS_PILEUP_H
#define PSD_READS_PILEUP_H

#include "dense_encode.h"
#include "psd_platform.h"

namespace psd {
namespace reads {

constexpr int THREADS = psd::dense::THREADS;
constexpr int WAVES = THREADS / WAVE;
constexpr int SLICE = THREADS; /* reads of a slice: one per lane */
constexpr int TILE = psd::dense::TILE;
constexpr int ROUNDS = psd::dense::ROUNDS;
constexpr int ROUND_SPAN = psd::dense::ROUND_SPAN;
constexpr int WAVE_SPAN = psd::dense::WAVE_SPAN;

typedef unsigned long long u64;
typedef psd::dense::Quad Quad;

struct Contig {
  const int *start, *end, *count; /* the reads; count == nullptr: every read counts 1 */
  int *cov;                       /* the contig's slots: 16-byte aligned, `padded` of them */
  long long n_reads;
  long long slice_first; /* index of the contig's first slice in scatter_kernel's grid */
  long long tile_first;  /* index of its first tile */
  long long padded;      /* hi - lo rounded up to a multiple of four */
  int lo, hi;
};

struct Check { /* per contig, zeroed */
  long long sum; /* of the good reads' counts */
  u64 bad;       /* ~index of the first bad read; 0: none */
};

PSD_D u64 shfl_u64(u64 v, int src) {
  const unsigned lo = (unsigned)shfl_i((int)(unsigned)v, src);
  const unsigned hi = (unsigned)shfl_i((int)(unsigned)(v >> 32), src);
  return ((u64)hi << 32) | lo;
}

__global__ __launch_bounds__(THREADS) void scatter_kernel(const Contig *contigs,
                                                          const int *slice_contig,
                                                          int last_base_only, Check *checks) {
  const long long slice = (long long)blockIdx.x;
  const int ci = slice_contig[slice];
  const Contig c = contigs[ci];
  const int lane = lane_id(), wave = wave_id();
  const long long i = (slice - c.slice_first) * SLICE + (long long)threadIdx.x;
  u64 good = 0, bad = 0;
  if (i < c.n_reads) {
    int s = c.start[i];
    const int e = c.end[i];
    const int k = c.count ? c.count[i] : 1;
    if (s >= e || k < 0) {
      bad = ~(u64)i;
    } else {
      good = (u64)k;
      if (last_base_only) s = e - 1;
      if (e > c.lo && s < c.hi && k > 0) {
        atomic_add_i32(c.cov + ((s > c.lo ? s : c.lo) - c.lo), k);
        if (e < c.hi) atomic_add_i32(c.cov + (e - c.lo), -k);
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const u64 o_good = shfl_u64(good, lane ^ off), o_bad = shfl_u64(bad, lane ^ off);
    good += o_good;
    bad = o_bad > bad ? o_bad : bad;
  }
  PSD_LDS u64 w_good[WAVES], w_bad[WAVES];
  if (lane == 0) {
    w_good[wave] = good;
    w_bad[wave] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < WAVES; w++) {
      good += w_good[w];
      bad = w_bad[w] > bad ? w_bad[w] : bad;
    }
    if (good) atomic_add_i64(&checks[ci].sum, (long long)good);
    if (bad) atomic_max_u64(&checks[ci].bad, bad);
  }
}

/* the four slots at u .. u + 3 of the contig; beyond its padded end: zeros (nothing is loaded) */
PSD_D Quad load_quad(const Contig &c, long long u) {
  Quad v;
  v.x = v.y = v.z = v.w = 0;
  if (u < c.padded) v = *(const Quad *)(c.cov + u);
  return v;
}

PSD_D unsigned quad_sum(const Quad &v) {
  return (unsigned)v.x + (unsigned)v.y + (unsigned)v.z + (unsigned)v.w;
}

__global__ __launch_bounds__(THREADS) void tile_sum_kernel(const Contig *contigs,
                                                           const int *tile_contig, int *tile_sum) {
  const long long tile = (long long)blockIdx.x;
  const Contig c = contigs[tile_contig[tile]];
  const int lane = lane_id(), wave = wave_id();
  const long long u = (tile - c.tile_first) * TILE + wave * WAVE_SPAN + lane * 4;
  const Quad v0 = load_quad(c, u), v1 = load_quad(c, u + ROUND_SPAN),
             v2 = load_quad(c, u + 2 * ROUND_SPAN), v3 = load_quad(c, u + 3 * ROUND_SPAN);
  unsigned s = quad_sum(v0) + quad_sum(v1) + quad_sum(v2) + quad_sum(v3);
  for (int off = 32; off > 0; off >>= 1) s += (unsigned)shfl_i((int)s, lane ^ off);
  PSD_LDS unsigned w_sum[WAVES];
  if (lane == 0) w_sum[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < WAVES; w++) s += w_sum[w];
    tile_sum[tile] = (int)s;
  }
}

/* One workgroup per contig.  Thread k takes the k-th share of the contig's tiles, adds it up,
 * learns from LDS what the shares before it hold, and walks its share again to write the scan
 * (the shape of dense::scan_kernel). */
__global__ __launch_bounds__(THREADS) void tile_scan_kernel(const Contig *contigs,
                                                            const int *tile_sum, int *tile_carry) {
  const Contig c = contigs[blockIdx.x];
  const int tid = (int)threadIdx.x;
  const long long n_tiles = (c.padded + TILE - 1) / TILE;
  const long long share = (n_tiles + THREADS - 1) / THREADS;
  const long long a = tid * share < n_tiles ? tid * share : n_tiles;
  const long long b = a + share < n_tiles ? a + share : n_tiles;
  unsigned sum = 0;
  for (long long t = a; t < b; t++) sum += (unsigned)tile_sum[c.tile_first + t];
  PSD_LDS unsigned s_sum[THREADS];
  s_sum[tid] = sum;
  __syncthreads();
  unsigned before = 0;
  for (int k = 0; k < tid; k++) before += s_sum[k];
  for (long long t = a; t < b; t++) {
    tile_carry[c.tile_first + t] = (int)before;
    before += (unsigned)tile_sum[c.tile_first + t];
  }
}

/* One round of a wave: the inclusive prefix sums of its 256 slots, on top of `running` (what the
 * wave's earlier rounds hold), which it advances.  Reached by all lanes of the wave. */
PSD_D void scan_round(Quad &v, unsigned &running) {
  const int lane = lane_id();
  const unsigned x = (unsigned)v.x, y = x + (unsigned)v.y, z = y + (unsigned)v.z,
                 w = z + (unsigned)v.w;
  unsigned incl = w; /* of the lanes' totals */
  for (int off = 1; off < WAVE; off <<= 1) {
    const unsigned o = (unsigned)shfl_i((int)incl, lane >= off ? lane - off : lane);
    if (lane >= off) incl += o;
  }
  const unsigned base = running + incl - w;
  v.x = (int)(base + x);
  v.y = (int)(base + y);
  v.z = (int)(base + z);
  v.w = (int)(base + w);
  running += (unsigned)shfl_i((int)incl, WAVE - 1);
}

PSD_D void store_quad(const Contig &c, long long u, const Quad &v, unsigned add) {
  if (u >= c.padded) return;
  Quad r;
  r.x = (int)((unsigned)v.x + add);
  r.y = (int)((unsigned)v.y + add);
  r.z = (int)((unsigned)v.z + add);
  r.w = (int)((unsigned)v.w + add);
  *(Quad *)(c.cov + u) = r;
}

__global__ __launch_bounds__(THREADS) void apply_kernel(const Contig *contigs,
                                                        const int *tile_contig,
                                                        const int *tile_carry) {
  const long long tile = (long long)blockIdx.x;
  const Contig c = contigs[tile_contig[tile]];
  const int lane = lane_id(), wave = wave_id();
  const long long u = (tile - c.tile_first) * TILE + wave * WAVE_SPAN + lane * 4;
  Quad v0 = load_quad(c, u), v1 = load_quad(c, u + ROUND_SPAN),
       v2 = load_quad(c, u + 2 * ROUND_SPAN), v3 = load_quad(c, u + 3 * ROUND_SPAN);
  unsigned running = 0;
  scan_round(v0, running);
  scan_round(v1, running);
  scan_round(v2, running);
  scan_round(v3, running);
  PSD_LDS unsigned w_total[WAVES];
  if (lane == 0) w_total[wave] = running;
  __syncthreads();
  unsigned add = (unsigned)tile_carry[tile];
  for (int w = 0; w < WAVES; w++)
    if (w < wave) add += w_total[w];
  store_quad(c, u, v0, add);
  store_quad(c, u + ROUND_SPAN, v1, add);
  store_quad(c, u + 2 * ROUND_SPAN, v2, add);
  store_quad(c, u + 3 * ROUND_SPAN, v3, add);
}

}  // namespace reads
}  // namespace psd
#endif
