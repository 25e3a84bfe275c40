/* strand_xcorr.h -- the strand cross-correlation of single-end reads on the device, in exact
 * integers, and the extension of stranded reads to a fragment length (the contract is in
 * include/peaksegdisk_hip.h).
 *
 * A read's tag is its 5' base: chromStart of a plus read, chromEnd - 1 of a minus read.  p[i] and
 * m[i] are the counts of the plus and minus tags at base lo + i of the contig's extent [lo, hi),
 * B = hi - lo.  Row s = 0 .. S of a contig's table holds six int64:
 *   pairs = max(B - s, 0), sum and sum of squares of p over i < B - s, sum and sum of squares of m
 *   over i >= s, and cross = sum of p[i] m[i + s] over i < B - s.
 *
 * Three launches per call, however many contigs it has, and no workgroup waits for another:
 *   tags_kernel    the shape of reads::scatter_kernel: a workgroup per slice of SLICE reads of one
 *                  contig, a read per lane.  A read with start >= end, a negative count or a strand
 *                  that is neither +1 nor -1 is bad and adds nothing; a good one adds its count at
 *                  its tag to the contig's zeroed `plus` or `minus` buffer (one int32 per base, one
 *                  no-return atomic per read) when the tag lies in the extent.  The workgroup's sum
 *                  of good counts and its first bad read go to the contig's 16-byte record
 *                  (reads::Check): key = ~index with the reason in the low REASON_BITS bits, a
 *                  64-bit max.
 *   xcorr_kernel   a workgroup per tile of TILE bases of `plus` (the encoder's tiling: a tile never
 *                  crosses a contig).  Every thread loads 16 plus and 16 minus slots of the tile;
 *                  the sums of p, p^2, m, m^2 go to one of the contig's copies of its totals by one
 *                  64-bit add each.  A
 *                  tile without a plus tag ends there, before it stages anything.  Otherwise
 *                  minus[t0 .. t0 + TILE + SHIFTS) goes to LDS (zeros beyond the contig's end) and
 *                  the tile's nonzero plus slots go to a compacted list (position, value) in LDS,
 *                  whose capacity is TILE.  The loop over the list is wave-uniform: a lane holds
 *                  one entry of each block of 64 and the wave reads it lane by lane (v_readlane).
 *                  Thread t owns the shifts t, t + 256, t + 512, t + 768 in four 64-bit
 *                  accumulators; per entry it reads minus_lds[pos + s] -- consecutive addresses
 *                  across the lanes -- and does one 32 x 32 -> 64-bit multiply-add.  At the end it
 *                  adds its nonzero accumulators to the cross column of the contig's rows.
 *   edges_kernel   a workgroup per contig: thread t owns the shifts 4t .. 4t + 3.  The sums of p
 *                  and p^2 over the last s bases and of m and m^2 over the first s bases are an
 *                  exclusive scan over the 1024 shifts (lane-local over four, the threads' totals
 *                  through LDS); with the totals they give the five other columns.
 * The host reads the records after tags_kernel and launches nothing further on a refusal.  Below a
 * sum of 2^31 per contig every slot fits int32, every product is below 2^62 and so is every sum of
 * products (at most sum p x sum m).  Integer adds commute: the table does not depend on the
 * schedule.
 *
 *   extend_kernel  a workgroup per slice of SLICE reads, a read per lane: a plus read becomes
 *                  [start, start + d), a minus read [end - d, end), formed in 64 bits and clamped
 *                  into int32.  The first read with start >= end or a bad strand goes to the
 *                  contig's record as above.
 *
 * Algorithmic traffic for n reads, B bases and S shifts: 9 n bytes of reads (13 n with counts),
 * one atomic per read, 8 B zeroed, 8 B read by xcorr_kernel (plus 4 SHIFTS per tile that has a plus
 * tag), at most SHIFTS 64-bit atomics per such tile, 48 (S + 1) bytes of table per contig.
 * Written against psd_platform.h only: the SIMT emulator of tests/emu runs this source. */
#ifndef PSD_STRAND_XCORR_H
#define PSD_STRAND_XCORR_H

#include "psd_platform.h"
#include "reads_pileup.h"

namespace psd {
namespace xcorr {

constexpr int THREADS = psd::reads::THREADS;
constexpr int WAVES = THREADS / WAVE;
constexpr int SLICE = THREADS;
constexpr int TILE = psd::reads::TILE;
constexpr int ROUND_SPAN = psd::reads::ROUND_SPAN;
constexpr int WAVE_SPAN = psd::reads::WAVE_SPAN;
constexpr int PER_THREAD = 4;                   /* shifts a thread owns */
constexpr int SHIFTS = THREADS * PER_THREAD;    /* 1024 */
constexpr int MAX_SHIFT = SHIFTS - 1;
constexpr int COLS = 6;   /* pairs, sum_plus, sq_plus, sum_minus, sq_minus, cross */
constexpr int TOTALS = 4; /* sum p, sum p^2, sum m, sum m^2 of a contig */
/* A contig's totals exist TOTAL_COPIES times, each copy in a 128-byte line of its own, and a tile
 * adds to the copy of its index modulo that: one line for all tiles of a long contig makes their
 * atomics queue behind each other (measured: DESIGN.md section 19).  edges_kernel adds them up. */
constexpr int TOTAL_COPIES = 32, TOTAL_STRIDE = 16;
constexpr int REASON_BITS = 2;
constexpr int BAD_ORDER = 1, BAD_COUNT = 2, BAD_STRAND = 3;

static_assert(TILE % 4 == 0 && SHIFTS == THREADS * 4 && TILE < 65536, "staging of xcorr_kernel");
static_assert((TILE + SHIFTS) * 4 + TILE * 6 + 1024 <= 65536, "static LDS of xcorr_kernel");

/* the short loops over a thread's own words: the library is built with -fno-unroll-loops, and this
 * pragma unrolls them all the same, so that the words are registers */
#ifdef __clang__
#define PSD_XCORR_UNROLL _Pragma("unroll")
#else
#define PSD_XCORR_UNROLL _Pragma("GCC unroll 4")
#endif

typedef psd::reads::u64 u64;
typedef psd::reads::Quad Quad;
typedef psd::reads::Check Check;
using psd::reads::shfl_u64;

struct Contig {
  const int *start, *end, *count; /* the reads; count == nullptr: every read counts 1 */
  const signed char *strand;      /* +1 or -1 per read, at any byte */
  int *plus, *minus;              /* the tags: 16-byte aligned, `padded` slots each, zeroed */
  long long *table;               /* (max_shift + 1) rows of COLS; the cross column zeroed */
  long long *totals;              /* TOTAL_COPIES x TOTAL_STRIDE words, zeroed */
  long long n_reads;
  long long slice_first; /* index of the contig's first slice in tags_kernel's grid */
  long long tile_first;  /* index of its first tile */
  long long padded;      /* hi - lo rounded up to a multiple of four */
  int lo, hi;
};

struct ExtendContig {
  const int *start, *end;
  const signed char *strand;
  int *out_start, *out_end;
  long long n_reads, slice_first;
  int length, pad; /* the fragment length d >= 1 */
};

PSD_D u64 check_key(long long read, int reason) { return ((~(u64)read) << REASON_BITS) | (u64)reason; }

/* the workgroup's sum of `good` and largest `bad` to the contig's record; reached by all threads */
PSD_D void send_check(u64 good, u64 bad, u64 *w_good, u64 *w_bad, Check *check) {
  const int lane = lane_id(), wave = wave_id();
  for (int off = 32; off > 0; off >>= 1) {
    const u64 o_good = shfl_u64(good, lane ^ off), o_bad = shfl_u64(bad, lane ^ off);
    good += o_good;
    bad = o_bad > bad ? o_bad : bad;
  }
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
    if (good) atomic_add_i64(&check->sum, (long long)good);
    if (bad) atomic_max_u64(&check->bad, bad);
  }
}

__global__ __launch_bounds__(THREADS) void tags_kernel(const Contig *contigs, const int *slice_contig,
                                                       Check *checks) {
  const long long slice = (long long)blockIdx.x;
  const int ci = slice_contig[slice];
  const Contig c = contigs[ci];
  const long long i = (slice - c.slice_first) * SLICE + (long long)threadIdx.x;
  u64 good = 0, bad = 0;
  if (i < c.n_reads) {
    const int s = c.start[i], e = c.end[i];
    const int k = c.count ? c.count[i] : 1;
    const int d = (int)c.strand[i];
    const int why = s >= e ? BAD_ORDER : (k < 0 ? BAD_COUNT : (d != 1 && d != -1 ? BAD_STRAND : 0));
    if (why) {
      bad = check_key(i, why);
    } else {
      good = (u64)k;
      const int at = d > 0 ? s : e - 1;
      if (at >= c.lo && at < c.hi && k > 0) atomic_add_i32((d > 0 ? c.plus : c.minus) + (at - c.lo), k);
    }
  }
  PSD_LDS u64 w_good[WAVES], w_bad[WAVES];
  send_check(good, bad, w_good, w_bad, checks + ci);
}

/* the four slots at u .. u + 3 of a contig's buffer; beyond its padded end: zeros */
PSD_D Quad load_quad(const int *slots, long long padded, long long u) {
  Quad v;
  v.x = v.y = v.z = v.w = 0;
  if (u < padded) v = *(const Quad *)(slots + u);
  return v;
}

PSD_D void add_moments(const Quad &v, u64 &s1, u64 &s2) {
  const u64 x = (unsigned)v.x, y = (unsigned)v.y, z = (unsigned)v.z, w = (unsigned)v.w;
  s1 += x + y + z + w;
  s2 += x * x + y * y + z * z + w * w;
}

PSD_D int quad_tags(const Quad &v) { return (v.x != 0) + (v.y != 0) + (v.z != 0) + (v.w != 0); }

/* the nonzero slots of v, which begins at slot `pos` of the tile, to the list from `at` on */
PSD_D void list_slot(int v, int pos, unsigned short *l_pos, int *l_val, int &at) {
  if (v) {
    l_pos[at] = (unsigned short)pos;
    l_val[at] = v;
    at++;
  }
}
PSD_D void list_quad(const Quad &v, int pos, unsigned short *l_pos, int *l_val, int &at) {
  list_slot(v.x, pos, l_pos, l_val, at);
  list_slot(v.y, pos + 1, l_pos, l_val, at);
  list_slot(v.z, pos + 2, l_pos, l_val, at);
  list_slot(v.w, pos + 3, l_pos, l_val, at);
}

/* The loop of xcorr_kernel over the n entries of the list, for the first NQ of the thread's four
 * shifts (the shifts beyond max_shift are not computed).  Reached by all lanes. */
template <int NQ>
PSD_D void cross_loop(const int *minus_lds, const unsigned short *l_pos, const int *l_val, int n,
                      u64 (&acc)[PER_THREAD]) {
  const int lane = lane_id();
  u64 a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  for (int base = 0; base < n; base += WAVE) {
    const int j = base + lane;
    const int my_pos = j < n ? (int)l_pos[j] : 0, my_val = j < n ? l_val[j] : 0;
    const int here = n - base < WAVE ? n - base : WAVE;
    /* four entries per trip, so that their LDS reads are in flight together (a lane beyond the
     * list holds the value 0 at position 0, and q + 3 stays below 64) */
    for (int q = 0; q < here; q += 4) {
      PSD_XCORR_UNROLL
      for (int k = 0; k < 4; k++) {
        const int pos = rdlane_i(my_pos, q + k);
        const u64 val = (unsigned)rdlane_i(my_val, q + k);
        const int *row = minus_lds + pos + (int)threadIdx.x;
        a0 += val * (unsigned)row[0];
        if (NQ > 1) a1 += val * (unsigned)row[THREADS];
        if (NQ > 2) a2 += val * (unsigned)row[2 * THREADS];
        if (NQ > 3) a3 += val * (unsigned)row[3 * THREADS];
      }
    }
  }
  acc[0] = a0;
  acc[1] = a1;
  acc[2] = a2;
  acc[3] = a3;
}

__global__ __launch_bounds__(THREADS) void xcorr_kernel(const Contig *contigs, const int *tile_contig,
                                                        int max_shift) {
  PSD_LDS int minus_lds[TILE + SHIFTS] __attribute__((aligned(16)));
  PSD_LDS int l_val[TILE];
  PSD_LDS unsigned short l_pos[TILE];
  PSD_LDS u64 w_sum[WAVES][TOTALS];
  PSD_LDS int w_tags[WAVES];
  const long long tile = (long long)blockIdx.x;
  const Contig c = contigs[tile_contig[tile]];
  const int lane = lane_id(), wave = wave_id();
  const long long t0 = (tile - c.tile_first) * TILE;
  const int own = wave * WAVE_SPAN + lane * 4; /* of the thread's first quad in the tile */
  const Quad p0 = load_quad(c.plus, c.padded, t0 + own),
             p1 = load_quad(c.plus, c.padded, t0 + own + ROUND_SPAN),
             p2 = load_quad(c.plus, c.padded, t0 + own + 2 * ROUND_SPAN),
             p3 = load_quad(c.plus, c.padded, t0 + own + 3 * ROUND_SPAN);
  const Quad m0 = load_quad(c.minus, c.padded, t0 + own),
             m1 = load_quad(c.minus, c.padded, t0 + own + ROUND_SPAN),
             m2 = load_quad(c.minus, c.padded, t0 + own + 2 * ROUND_SPAN),
             m3 = load_quad(c.minus, c.padded, t0 + own + 3 * ROUND_SPAN);
  u64 sum[TOTALS] = {0, 0, 0, 0};
  add_moments(p0, sum[0], sum[1]);
  add_moments(p1, sum[0], sum[1]);
  add_moments(p2, sum[0], sum[1]);
  add_moments(p3, sum[0], sum[1]);
  add_moments(m0, sum[2], sum[3]);
  add_moments(m1, sum[2], sum[3]);
  add_moments(m2, sum[2], sum[3]);
  add_moments(m3, sum[2], sum[3]);
  const int mine = quad_tags(p0) + quad_tags(p1) + quad_tags(p2) + quad_tags(p3);
  int incl = mine; /* the wave's inclusive scan of the threads' plus tags */
  for (int off = 1; off < WAVE; off <<= 1) {
    const int o = shfl_i(incl, lane >= off ? lane - off : lane);
    if (lane >= off) incl += o;
  }
  const int wave_tags = shfl_i(incl, WAVE - 1);
  PSD_XCORR_UNROLL
  for (int k = 0; k < TOTALS; k++)
    for (int off = 32; off > 0; off >>= 1) sum[k] += shfl_u64(sum[k], lane ^ off);
  if (lane == 0) {
    w_tags[wave] = wave_tags;
  PSD_XCORR_UNROLL
    for (int k = 0; k < TOTALS; k++) w_sum[wave][k] = sum[k];
  }
  __syncthreads();
  int n = 0, at = incl - mine;
  for (int w = 0; w < WAVES; w++) {
    n += w_tags[w];
    if (w < wave) at += w_tags[w];
  }
  if (threadIdx.x == 0) {
    long long *copy = c.totals + ((tile - c.tile_first) % TOTAL_COPIES) * TOTAL_STRIDE;
  PSD_XCORR_UNROLL
    for (int k = 0; k < TOTALS; k++) {
      u64 all = sum[k];
      for (int w = 1; w < WAVES; w++) all += w_sum[w][k];
      if (all) atomic_add_i64(copy + k, (long long)all);
    }
  }
  if (n == 0) return; /* (the same in every thread) */

  *(Quad *)(minus_lds + own) = m0;
  *(Quad *)(minus_lds + own + ROUND_SPAN) = m1;
  *(Quad *)(minus_lds + own + 2 * ROUND_SPAN) = m2;
  *(Quad *)(minus_lds + own + 3 * ROUND_SPAN) = m3;
  *(Quad *)(minus_lds + TILE + (int)threadIdx.x * 4) =
      load_quad(c.minus, c.padded, t0 + TILE + (long long)threadIdx.x * 4);
  list_quad(p0, own, l_pos, l_val, at);
  list_quad(p1, own + ROUND_SPAN, l_pos, l_val, at);
  list_quad(p2, own + 2 * ROUND_SPAN, l_pos, l_val, at);
  list_quad(p3, own + 3 * ROUND_SPAN, l_pos, l_val, at);
  __syncthreads();

  u64 acc[PER_THREAD];
  const int nq = max_shift / THREADS + 1;
  if (nq == 1)
    cross_loop<1>(minus_lds, l_pos, l_val, n, acc);
  else if (nq == 2)
    cross_loop<2>(minus_lds, l_pos, l_val, n, acc);
  else if (nq == 3)
    cross_loop<3>(minus_lds, l_pos, l_val, n, acc);
  else
    cross_loop<4>(minus_lds, l_pos, l_val, n, acc);
  PSD_XCORR_UNROLL
  for (int k = 0; k < PER_THREAD; k++) {
    const int s = (int)threadIdx.x + k * THREADS;
    if (s <= max_shift && acc[k]) atomic_add_i64(c.table + (long long)s * COLS + (COLS - 1), (long long)acc[k]);
  }
}

__global__ __launch_bounds__(THREADS) void edges_kernel(const Contig *contigs, int max_shift) {
  PSD_LDS u64 s_tot[TOTALS][THREADS];
  const Contig c = contigs[blockIdx.x];
  const int tid = (int)threadIdx.x;
  const long long bases = (long long)c.hi - c.lo;
  /* element e of the tail is p[B - 1 - e], of the head m[e]; beyond the contig: zeros */
  u64 tail[PER_THREAD], head[PER_THREAD];
  u64 tot[TOTALS] = {0, 0, 0, 0};
  PSD_XCORR_UNROLL
  for (int k = 0; k < PER_THREAD; k++) {
    const long long e = (long long)tid * PER_THREAD + k;
    tail[k] = e < bases ? (u64)(unsigned)c.plus[bases - 1 - e] : 0;
    head[k] = e < bases ? (u64)(unsigned)c.minus[e] : 0;
    tot[0] += tail[k];
    tot[1] += tail[k] * tail[k];
    tot[2] += head[k];
    tot[3] += head[k] * head[k];
  }
  PSD_XCORR_UNROLL
  for (int k = 0; k < TOTALS; k++) s_tot[k][tid] = tot[k];
  __syncthreads();
  u64 before[TOTALS] = {0, 0, 0, 0}; /* over the shifts in front of the thread's */
  for (int t = 0; t < tid; t++) {
  PSD_XCORR_UNROLL
    for (int k = 0; k < TOTALS; k++) before[k] += s_tot[k][t];
  }
  u64 all[TOTALS] = {0, 0, 0, 0};
  for (int copy = 0; copy < TOTAL_COPIES; copy++) {
  PSD_XCORR_UNROLL
    for (int k = 0; k < TOTALS; k++) all[k] += (u64)c.totals[copy * TOTAL_STRIDE + k];
  }
  PSD_XCORR_UNROLL
  for (int k = 0; k < PER_THREAD; k++) {
    const int s = tid * PER_THREAD + k;
    if (s <= max_shift) {
      long long *row = c.table + (long long)s * COLS;
      row[0] = bases > s ? bases - s : 0;
      row[1] = (long long)(all[0] - before[0]);
      row[2] = (long long)(all[1] - before[1]);
      row[3] = (long long)(all[2] - before[2]);
      row[4] = (long long)(all[3] - before[3]);
    }
    before[0] += tail[k];
    before[1] += tail[k] * tail[k];
    before[2] += head[k];
    before[3] += head[k] * head[k];
  }
}

__global__ __launch_bounds__(THREADS) void extend_kernel(const ExtendContig *contigs,
                                                         const int *slice_contig, Check *checks) {
  const long long slice = (long long)blockIdx.x;
  const int ci = slice_contig[slice];
  const ExtendContig c = contigs[ci];
  const long long i = (slice - c.slice_first) * SLICE + (long long)threadIdx.x;
  u64 bad = 0;
  if (i < c.n_reads) {
    const int s = c.start[i], e = c.end[i];
    const int d = (int)c.strand[i];
    const int why = s >= e ? BAD_ORDER : (d != 1 && d != -1 ? BAD_STRAND : 0);
    if (why) {
      bad = check_key(i, why);
    } else {
      const long long to = (long long)s + c.length, from = (long long)e - c.length;
      c.out_start[i] = d > 0 ? s : (int)(from < psd::dense::I32_MIN ? psd::dense::I32_MIN : from);
      c.out_end[i] = d > 0 ? (int)(to > psd::dense::I32_MAX ? psd::dense::I32_MAX : to) : e;
    }
  }
  PSD_LDS u64 w_good[WAVES], w_bad[WAVES];
  send_check(0, bad, w_good, w_bad, checks + ci);
}

}  // namespace xcorr
}  // namespace psd
#endif
