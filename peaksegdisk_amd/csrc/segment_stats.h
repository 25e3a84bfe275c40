/* segment_stats.h -- what every row of the segments table holds, from the runs resident in HBM:
 * the reads under the segment (sum of count x weight), its largest count, and the coordinates of
 * the first run in genomic order that attains it (the summit).
 *
 * Row r of a problem's segment table covers the runs seg_start[r] + 1 ... seg_start[r - 1] of its
 * contig (row 0 runs to the contig's last run, seg_start < 0 starts at run 0): the rows are in
 * reverse genomic order and seg_start decreases with r.
 *
 * Two launches per call, however many problems the set has, and no workgroup waits for another:
 *   tile_kernel    a workgroup per tile of TILE runs of a (problem, contig) pair.  The row of the
 *                  tile's first run is found by a 64-way search of the segment table that every
 *                  wave makes for itself; the rows that begin inside the tile are read from the
 *                  table (coalesced) and leave a mark in LDS; each lane folds its four runs, a
 *                  segmented scan combines the lanes of a wave, and the two partial results of a
 *                  wave that other waves may share (its first and its last segment) meet in LDS.
 *                  What a workgroup knows of a row goes to HBM by two 64-bit integer atomics on
 *                  zeroed words: an add to sum[] and an unsigned max to key[], where
 *                  key = count << 32 | ~run index, so that the larger count wins and, among equal
 *                  counts, the EARLIER run.  Integer atomics commute: the results do not depend on
 *                  the schedule.
 *   finish_kernel  a thread per row: max = key >> 32, and the summit's coordinates from run_end[]
 *                  and weight[] of the run the key names (the only reads of run_end).
 * Algorithmic traffic per problem: 8 R bytes of count and weight for R runs, and per row 4 B of
 * seg_start, 16 B zeroed, 16 B of atomics, 8 B of key read back, 8 B of run_end / weight and 12 B
 * of max / summitStart / summitEnd.
 *
 * As in dense_encode.h a contig may begin at any run offset: its tiles are laid over the 16-byte
 * aligned range that holds it (`lead` = 0..3 entries in front of its first run) so that every lane
 * loads 16 aligned bytes of count[] and of weight[]; only a contig's first and last load may be
 * partial.  Written against psd_platform.h only: the SIMT emulator of tests/emu runs this source. */
#ifndef PSD_SEGMENT_STATS_H
#define PSD_SEGMENT_STATS_H

#include "dense_encode.h"
#include "psd_platform.h"

namespace psd {
namespace stats {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;
constexpr int TILE = THREADS * 4; /* runs of a tile: four per lane, a contiguous quarter per wave */
constexpr int DESC = 8;           /* long longs per problem in the descriptor array */

typedef unsigned long long u64;
typedef psd::dense::Quad Quad;

/* per problem, desc[DESC p + ...] */
enum {
  D_TO = 0,     /* first packed row */
  D_ROWS = 1,   /* rows of its segment table (0: not solved, nothing to do) */
  D_FROM = 2,   /* offset of the table in seg_start */
  D_RUN0 = 3,   /* first run of its contig in count / weight / run_end */
  D_RUNS = 4,   /* runs of the contig */
  D_FIRST = 5,  /* chromStart of the contig's first base */
  D_TILE0 = 6,  /* index of the problem's first tile in the grid */
};

/* what is known of a segment: (0, 0) is "nothing", and combining is commutative and associative */
struct Part {
  long long sum;
  u64 key;
};

PSD_D Part join(const Part &a, const Part &b) {
  Part r;
  r.sum = a.sum + b.sum;
  r.key = a.key > b.key ? a.key : b.key;
  return r;
}

PSD_D u64 shfl_u64(u64 v, int src) {
  const unsigned lo = (unsigned)shfl_i((int)(unsigned)v, src);
  const unsigned hi = (unsigned)shfl_i((int)(unsigned)(v >> 32), src);
  return ((u64)hi << 32) | lo;
}

PSD_D Part shfl_part(const Part &p, int src) {
  Part r;
  r.sum = (long long)shfl_u64((u64)p.sum, src);
  r.key = shfl_u64(p.key, src);
  return r;
}

PSD_D void post(long long *sum, u64 *key, long long row, const Part &p) {
  if (p.key == 0) return; /* no run */
  atomic_add_i64(sum + row, p.sum);
  atomic_max_u64(key + row, p.key);
}

/* the four entries at u .. u + 3 of the contig's aligned range [.. lo, hi ..): entries outside the
 * contig read as 0 */
PSD_D void load_quad(const int *base, long long u, long long lo, long long hi, Quad &v) {
  if (u >= lo && u + 4 <= hi) {
    v = *(const Quad *)(base + u);
    return;
  }
  v.x = v.y = v.z = v.w = 0;
  if (u >= lo && u < hi) v.x = base[u];
  if (u + 1 >= lo && u + 1 < hi) v.y = base[u + 1];
  if (u + 2 >= lo && u + 2 < hi) v.z = base[u + 2];
  if (u + 3 >= lo && u + 3 < hi) v.w = base[u + 3];
}

/* One run of a lane, in order.  `head`: a row begins with this run; what the lane had gathered
 * belongs to the row before it: the first such part is kept (it joins what earlier lanes hold),
 * the later ones are whole segments inside the lane and go out at once. */
struct LaneFold {
  Part pre, cur;
  bool seen;
  long long row; /* packed row of the run at hand */
};

PSD_D void fold_run(LaneFold &f, bool valid, bool head, int count, int weight, long long run,
                    long long *sum, u64 *key) {
  if (head) {
    if (!f.seen) {
      f.pre = f.cur;
      f.seen = true;
    } else {
      post(sum, key, f.row, f.cur);
    }
    f.cur.sum = 0;
    f.cur.key = 0;
    f.row -= 1;
  }
  if (valid) {
    const u64 k = ((u64)(unsigned)count << 32) | (u64)(0xffffffffu - (unsigned)run);
    f.cur.sum += (long long)count * (long long)weight;
    f.cur.key = k > f.cur.key ? k : f.cur.key;
  }
}

__global__ __launch_bounds__(THREADS) void tile_kernel(const long long *desc, const int *tile_problem,
                                                       const int *seg_start, const int *count,
                                                       const int *weight, long long *sum, u64 *key) {
  const long long *d = desc + (long long)DESC * tile_problem[blockIdx.x];
  const long long n_rows = d[D_ROWS];
  if (n_rows <= 0) return; /* (the whole workgroup) */
  const long long to = d[D_TO], run0 = d[D_RUN0], n_runs = d[D_RUNS];
  const int *table = seg_start + d[D_FROM];
  const int lane = lane_id(), wave = wave_id(), tid = (int)threadIdx.x;
  /* the contig in aligned coordinates: run i is entry u = i + lead of base[] */
  const long long lead = run0 & 3;
  const long long u_tile = ((long long)blockIdx.x - d[D_TILE0]) * TILE;
  const long long u_first = u_tile > lead ? u_tile : lead; /* the tile's first run */
  const long long u_end = u_tile + TILE;

  /* r_hi: the row of the tile's first run, the smallest r with seg_start[r] + 1 <= that run.
   * seg_start decreases with r, the last row starts at run 0: the probes of a round that fail are
   * its first ones.  Every wave searches for itself (the same addresses: no barrier). */
  long long lo = 0, hi = n_rows - 1;
  if (u_tile <= lead) lo = hi;
  while (lo < hi) {
    const long long step = (hi - lo + WAVE) / WAVE;
    const long long r = lo + lane * step;
    const bool below = r <= hi && (long long)table[r] + 1 + lead > u_first;
    const int n_below = popc64(ballot(below));
    if (n_below == 0) {
      hi = lo;
    } else {
      const long long first_at = lo + n_below * step; /* the first probe that holds, if in range */
      lo = lo + (n_below - 1) * step + 1;
      hi = first_at < hi ? first_at : hi;
    }
  }
  const long long r_hi = lo;

  /* the rows that begin inside the tile are r_hi - 1, r_hi - 2, ... while they start before its end */
  PSD_LDS Quad l_head4[TILE / 4]; /* 1: a row begins with the run at this place of the tile */
  int *l_head = (int *)l_head4;
  PSD_LDS int w_heads[WAVES];
  PSD_LDS long long w_row[2 * WAVES], w_sum[2 * WAVES];
  PSD_LDS u64 w_key[2 * WAVES];
  for (int j = tid; j < TILE; j += THREADS) l_head[j] = 0;
  __syncthreads();
  for (int k = 0; k < 4; k++) {
    const long long r = r_hi - 1 - (tid + k * THREADS);
    if (r < 0) break;
    const long long u = (long long)table[r] + 1 + lead;
    if (u >= u_end) break;
    if (u > u_first) l_head[u - u_tile] = 1;
  }
  __syncthreads();

  const long long u = u_tile + 4 * tid;
  Quad c, w;
  load_quad(count + run0 - lead, u, lead, lead + n_runs, c);
  load_quad(weight + run0 - lead, u, lead, lead + n_runs, w);
  const Quad h = l_head4[tid];
  const unsigned long long b0 = ballot(h.x != 0), b1 = ballot(h.y != 0), b2 = ballot(h.z != 0),
                           b3 = ballot(h.w != 0);
  if (lane == 0) w_heads[wave] = popc64(b0) + popc64(b1) + popc64(b2) + popc64(b3);
  __syncthreads();
  int heads_before = 0;
  for (int k = 0; k < WAVES; k++)
    if (k < wave) heads_before += w_heads[k];
  const unsigned long long below = lanes_below(lane);
  heads_before += popc64(b0 & below) + popc64(b1 & below) + popc64(b2 & below) + popc64(b3 & below);

  LaneFold f;
  f.pre.sum = f.cur.sum = 0;
  f.pre.key = f.cur.key = 0;
  f.seen = false;
  f.row = to + r_hi - heads_before;
  const long long row_in = f.row; /* the row the lane's first run continues, unless it is a head */
  const long long i = u - lead;
  const long long v_lo = lead, v_hi = lead + n_runs;
  fold_run(f, u >= v_lo && u < v_hi, h.x != 0, c.x, w.x, i, sum, key);
  fold_run(f, u + 1 >= v_lo && u + 1 < v_hi, h.y != 0, c.y, w.y, i + 1, sum, key);
  fold_run(f, u + 2 >= v_lo && u + 2 < v_hi, h.z != 0, c.z, w.z, i + 2, sum, key);
  fold_run(f, u + 3 >= v_lo && u + 3 < v_hi, h.w != 0, c.w, w.w, i + 3, sum, key);

  /* segmented inclusive scan of the lanes' last parts: after it `s` holds what the lanes from the
   * last one with a head (or lane 0) up to this one gathered for the row this lane ends in */
  Part s = f.cur;
  bool stop = f.seen;
  for (int off = 1; off < WAVE; off <<= 1) {
    const int src = lane >= off ? lane - off : lane;
    const Part o = shfl_part(s, src);
    const int o_stop = shfl_i(stop ? 1 : 0, src);
    if (lane >= off && !stop) {
      s = join(o, s);
      stop = o_stop != 0;
    }
  }
  /* a lane with a head closes the row it came in with: what the lanes before it hold, and its own
   * first part.  The first such lane of the wave may share that row with earlier waves. */
  Part before = shfl_part(s, lane > 0 ? lane - 1 : 0);
  if (lane == 0) before.sum = 0, before.key = 0;
  const unsigned long long seen_mask = ballot(f.seen);
  const int first_seen = seen_mask ? ctz64(seen_mask) : -1;
  if (f.seen) {
    const Part e = join(before, f.pre);
    if (lane == first_seen) {
      w_row[2 * wave] = row_in;
      w_sum[2 * wave] = e.sum;
      w_key[2 * wave] = e.key;
    } else {
      post(sum, key, row_in, e);
    }
  }
  if (lane == WAVE - 1) {
    if (first_seen < 0) { /* the wave lies in one row: one part */
      w_row[2 * wave] = f.row;
      w_sum[2 * wave] = 0;
      w_key[2 * wave] = 0;
    }
    w_row[2 * wave + 1] = f.row;
    w_sum[2 * wave + 1] = s.sum;
    w_key[2 * wave + 1] = s.key;
  }
  __syncthreads();
  if (tid == 0) { /* the waves' shared parts in genomic order: equal rows are one segment */
    long long row = w_row[0];
    Part p;
    p.sum = w_sum[0];
    p.key = w_key[0];
    for (int k = 1; k < 2 * WAVES; k++) {
      Part q;
      q.sum = w_sum[k];
      q.key = w_key[k];
      if (w_row[k] == row) {
        p = join(p, q);
      } else {
        post(sum, key, row, p);
        row = w_row[k];
        p = q;
      }
    }
    post(sum, key, row, p);
  }
}

/* A thread per packed row.  Its problem is the last one whose first packed row is not beyond it
 * (problems without rows share their successor's): a binary search of the descriptors, a few
 * cached lines that all threads read.  A key that names no run of the contig (a row no tile met:
 * there is none in a solved set) gives zeros, not a read beyond the arrays. */
__global__ __launch_bounds__(THREADS) void finish_kernel(const long long *desc, int n_problems,
                                                         long long total, const u64 *key,
                                                         const int *weight, const int *run_end,
                                                         int *mx, int *summit_start,
                                                         int *summit_end) {
  const long long row = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (row >= total) return;
  int lo = 0, hi = n_problems - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (desc[(long long)DESC * mid + D_TO] <= row)
      lo = mid;
    else
      hi = mid - 1;
  }
  const long long *d = desc + (long long)DESC * lo;
  const long long run0 = d[D_RUN0], n_runs = d[D_RUNS];
  const int first = (int)d[D_FIRST];
  const u64 k = key[row];
  const long long run = (long long)(0xffffffffu - (unsigned)k);
  if (k == 0 || run >= n_runs) {
    mx[row] = 0;
    summit_start[row] = first;
    summit_end[row] = first;
    return;
  }
  const int e = run_end[run0 + run];
  mx[row] = (int)(unsigned)(k >> 32);
  summit_start[row] = first + e - weight[run0 + run];
  summit_end[row] = first + e;
}

}  // namespace stats
}  // namespace psd
#endif
