/* dense_encode.h -- run-length encoding of dense coverage (one int32 count per base) on the
 * device, straight into the layout the forward kernels read (count[], weight[]) plus run_end[].
 *
 * Three launches per call, however many contigs it has, and no workgroup ever waits for another:
 *   count_kernel    a workgroup per tile of TILE bases: the run starts in the tile, the position of
 *                   the last of them, minimum, maximum and sum of the tile's counts
 *   scan_kernel     a workgroup per contig: exclusive scan of its tiles' run counts, the start of
 *                   the run that is open where each tile begins, the contig's statistics
 *   scatter_kernel  a workgroup per tile again (the input is read a second time): the tile's runs
 *                   go through LDS in order and leave in coalesced stores
 * between the second and the third the host downloads the per-contig statistics (24 bytes each),
 * refuses what it has to refuse and allocates the outputs at their exact sizes.
 * Algorithmic traffic: 8 B + 12 R bytes for B bases and R runs.
 *
 * A tile never crosses a contig.  A contig may begin at any 4-byte address: its tiles are laid
 * over the 16-byte aligned range that holds it (`lead` = 0..3 elements in front of its first
 * base), so that every lane loads 16 aligned bytes; only a contig's first and last load may be
 * partial and are made element by element.  Inside a tile each wave owns a contiguous quarter and
 * reads it in ROUNDS rounds of 64 lanes x 4 bases (1 KB per load instruction).
 *
 * Written against psd_platform.h only (ballot, popc64, lane shuffles, __syncthreads, LDS), so the
 * SIMT emulator of tests/emu runs the same source. */
#ifndef PSD_DENSE_ENCODE_H
#define PSD_DENSE_ENCODE_H

#include "psd_platform.h"

namespace psd {
namespace dense {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;
constexpr int ROUNDS = 4;
constexpr int ROUND_SPAN = WAVE * 4;             /* bases one wave loads at once */
constexpr int WAVE_SPAN = ROUND_SPAN * ROUNDS;   /* bases of a tile one wave owns */
constexpr int TILE = WAVE_SPAN * WAVES;          /* 4096 bases */
constexpr int I32_MAX = 2147483647;
constexpr int I32_MIN = -I32_MAX - 1;

struct alignas(16) Quad {
  int x, y, z, w;
};

struct Contig {
  const int *base;      /* the contig's first base minus `lead` elements: 16-byte aligned */
  long long n;          /* bases */
  long long tile_first; /* index of the contig's first tile */
  long long run_off;    /* index of its first run in the outputs (scatter_kernel only) */
  int lead;
  int pad;
};

struct TileInfo {
  long long sum;
  int runs;
  int last_start; /* offset from the contig's first base of the last run start in the tile; -1: none */
  int mn, mx;
};

struct TileScan {
  int runs_before; /* runs of the contig that start in earlier tiles */
  int open_start;  /* where the run that is open at the tile's first base started */
};

struct ContigStats {
  long long sum;
  long long runs;
  int mn, mx;
};

/* the four elements at u .. u+3 of the contig's aligned range; `in`: bit j = element j is a base
 * of the contig */
PSD_D void load_quad(const Contig &c, long long u, Quad &v, unsigned &in) {
  const long long lo = c.lead, hi = c.lead + c.n;
  if (u >= lo && u + 4 <= hi) {
    v = *(const Quad *)(c.base + u);
    in = 15u;
    return;
  }
  in = 0u;
  v.x = v.y = v.z = v.w = 0;
  if (u >= lo && u < hi) v.x = c.base[u], in |= 1u;
  if (u + 1 >= lo && u + 1 < hi) v.y = c.base[u + 1], in |= 2u;
  if (u + 2 >= lo && u + 2 < hi) v.z = c.base[u + 2], in |= 4u;
  if (u + 3 >= lo && u + 3 < hi) v.w = c.base[u + 3], in |= 8u;
}

/* bit j: a run starts at element j (the contig's first base, or a count that differs from the one
 * before it).  Reached by all lanes of the wave. */
PSD_D unsigned run_starts(const Contig &c, long long u, const Quad &v, unsigned in) {
  const int lane = lane_id();
  int before = shfl_i(v.w, (lane + 63) & 63);
  if (lane == 0 && (in & 1u) && u > c.lead) before = c.base[u - 1];
  const long long lo = c.lead;
  unsigned f = 0u;
  if ((in & 1u) && (u == lo || v.x != before)) f |= 1u;
  if ((in & 2u) && (u + 1 == lo || v.y != v.x)) f |= 2u;
  if ((in & 4u) && (u + 2 == lo || v.z != v.y)) f |= 4u;
  if ((in & 8u) && (u + 3 == lo || v.w != v.z)) f |= 8u;
  return f;
}

struct Tally {
  long long sum = 0;
  int runs = 0; /* of the wave */
  int last = -1;
  int mn = I32_MAX, mx = I32_MIN;
};

PSD_D void tally_round(const Contig &c, long long u, const Quad &v, unsigned in, Tally &t) {
  const unsigned f = run_starts(c, u, v, in);
  t.runs += popc64(ballot((f & 1u) != 0)) + popc64(ballot((f & 2u) != 0)) +
            popc64(ballot((f & 4u) != 0)) + popc64(ballot((f & 8u) != 0));
  if (f) t.last = (int)(u - c.lead) + (f & 8u ? 3 : f & 4u ? 2 : f & 2u ? 1 : 0);
  if (in & 1u) t.sum += v.x, t.mn = v.x < t.mn ? v.x : t.mn, t.mx = v.x > t.mx ? v.x : t.mx;
  if (in & 2u) t.sum += v.y, t.mn = v.y < t.mn ? v.y : t.mn, t.mx = v.y > t.mx ? v.y : t.mx;
  if (in & 4u) t.sum += v.z, t.mn = v.z < t.mn ? v.z : t.mn, t.mx = v.z > t.mx ? v.z : t.mx;
  if (in & 8u) t.sum += v.w, t.mn = v.w < t.mn ? v.w : t.mn, t.mx = v.w > t.mx ? v.w : t.mx;
}

__global__ __launch_bounds__(THREADS) void count_kernel(const Contig *contigs,
                                                        const int *tile_contig, TileInfo *tiles) {
  const long long tile = (long long)blockIdx.x;
  const Contig c = contigs[tile_contig[tile]];
  const int lane = lane_id(), wave = wave_id();
  const long long u = (tile - c.tile_first) * TILE + wave * WAVE_SPAN + lane * 4;
  Quad v0, v1, v2, v3;
  unsigned in0, in1, in2, in3;
  load_quad(c, u, v0, in0);
  load_quad(c, u + ROUND_SPAN, v1, in1);
  load_quad(c, u + 2 * ROUND_SPAN, v2, in2);
  load_quad(c, u + 3 * ROUND_SPAN, v3, in3);
  Tally t;
  tally_round(c, u, v0, in0, t);
  tally_round(c, u + ROUND_SPAN, v1, in1, t);
  tally_round(c, u + 2 * ROUND_SPAN, v2, in2, t);
  tally_round(c, u + 3 * ROUND_SPAN, v3, in3, t);
  int lo = (int)(unsigned)(unsigned long long)t.sum, hi = (int)(unsigned)((unsigned long long)t.sum >> 32);
  for (int off = 32; off > 0; off >>= 1) {
    /* (64-bit sum of two lanes from its halves: the low words are added as unsigned) */
    const int o_lo = shfl_i(lo, lane ^ off), o_hi = shfl_i(hi, lane ^ off);
    const int o_last = shfl_i(t.last, lane ^ off);
    const int o_mn = shfl_i(t.mn, lane ^ off), o_mx = shfl_i(t.mx, lane ^ off);
    const unsigned long long a = ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
    const unsigned long long b = ((unsigned long long)(unsigned)o_hi << 32) | (unsigned)o_lo;
    const unsigned long long s = a + b;
    lo = (int)(unsigned)s;
    hi = (int)(unsigned)(s >> 32);
    t.last = o_last > t.last ? o_last : t.last;
    t.mn = o_mn < t.mn ? o_mn : t.mn;
    t.mx = o_mx > t.mx ? o_mx : t.mx;
  }
  PSD_LDS long long w_sum[WAVES];
  PSD_LDS int w_runs[WAVES], w_last[WAVES], w_mn[WAVES], w_mx[WAVES];
  if (lane == 0) {
    w_sum[wave] = (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
    w_runs[wave] = t.runs;
    w_last[wave] = t.last;
    w_mn[wave] = t.mn;
    w_mx[wave] = t.mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    TileInfo ti;
    ti.sum = 0;
    ti.runs = 0;
    ti.last_start = -1;
    ti.mn = I32_MAX;
    ti.mx = I32_MIN;
    for (int w = 0; w < WAVES; w++) {
      ti.sum += w_sum[w];
      ti.runs += w_runs[w];
      ti.last_start = w_last[w] > ti.last_start ? w_last[w] : ti.last_start;
      ti.mn = w_mn[w] < ti.mn ? w_mn[w] : ti.mn;
      ti.mx = w_mx[w] > ti.mx ? w_mx[w] : ti.mx;
    }
    tiles[tile] = ti;
  }
}

/* One workgroup per contig.  Thread k takes the k-th share of the contig's tiles, adds it up,
 * learns from LDS what the shares before it hold, and walks its share again to write the scan. */
__global__ __launch_bounds__(THREADS) void scan_kernel(const Contig *contigs, const TileInfo *tiles,
                                                       TileScan *scan, ContigStats *stats) {
  const Contig c = contigs[blockIdx.x];
  const int tid = (int)threadIdx.x;
  const long long n_tiles = (c.lead + c.n + TILE - 1) / TILE;
  const long long share = (n_tiles + THREADS - 1) / THREADS;
  const long long a = tid * share < n_tiles ? tid * share : n_tiles;
  const long long b = a + share < n_tiles ? a + share : n_tiles;
  long long runs = 0, sum = 0;
  int last = -1, mn = I32_MAX, mx = I32_MIN;
  for (long long t = a; t < b; t++) {
    const TileInfo ti = tiles[c.tile_first + t];
    runs += ti.runs;
    sum += ti.sum;
    last = ti.last_start > last ? ti.last_start : last;
    mn = ti.mn < mn ? ti.mn : mn;
    mx = ti.mx > mx ? ti.mx : mx;
  }
  PSD_LDS long long s_runs[THREADS], s_sum[THREADS];
  PSD_LDS int s_last[THREADS], s_mn[THREADS], s_mx[THREADS];
  s_runs[tid] = runs;
  s_sum[tid] = sum;
  s_last[tid] = last;
  s_mn[tid] = mn;
  s_mx[tid] = mx;
  __syncthreads();
  long long before = 0;
  int open = -1;
  for (int k = 0; k < tid; k++) {
    before += s_runs[k];
    open = s_last[k] > open ? s_last[k] : open;
  }
  for (long long t = a; t < b; t++) {
    const TileInfo ti = tiles[c.tile_first + t];
    TileScan ts;
    ts.runs_before = (int)before; /* (a contig of 2^30 runs or more is refused before the scatter) */
    ts.open_start = open;
    scan[c.tile_first + t] = ts;
    before += ti.runs;
    open = ti.last_start > open ? ti.last_start : open;
  }
  if (tid == 0) {
    ContigStats cs;
    cs.sum = 0;
    cs.runs = 0;
    cs.mn = I32_MAX;
    cs.mx = I32_MIN;
    for (int k = 0; k < THREADS; k++) {
      cs.sum += s_sum[k];
      cs.runs += s_runs[k];
      cs.mn = s_mn[k] < cs.mn ? s_mn[k] : cs.mn;
      cs.mx = s_mx[k] > cs.mx ? s_mx[k] : cs.mx;
    }
    stats[blockIdx.x] = cs;
  }
}

/* the wave's run starts of one round, in order, into the wave's part of the tile's LDS lists */
PSD_D void place_round(const Contig &c, long long u, const Quad &v, unsigned in, int *l_start,
                       int *l_val, int &placed) {
  const unsigned f = run_starts(c, u, v, in);
  const unsigned long long b0 = ballot((f & 1u) != 0), b1 = ballot((f & 2u) != 0),
                           b2 = ballot((f & 4u) != 0), b3 = ballot((f & 8u) != 0);
  const unsigned long long below = lanes_below(lane_id());
  int r = placed + popc64(b0 & below) + popc64(b1 & below) + popc64(b2 & below) + popc64(b3 & below);
  const int pos = (int)(u - c.lead);
  if (f & 1u) l_start[r] = pos, l_val[r] = v.x, r++;
  if (f & 2u) l_start[r] = pos + 1, l_val[r] = v.y, r++;
  if (f & 4u) l_start[r] = pos + 2, l_val[r] = v.z, r++;
  if (f & 8u) l_start[r] = pos + 3, l_val[r] = v.w, r++;
  placed += popc64(b0) + popc64(b1) + popc64(b2) + popc64(b3);
}

__global__ __launch_bounds__(THREADS) void scatter_kernel(const Contig *contigs,
                                                          const int *tile_contig,
                                                          const TileScan *scan, int *count,
                                                          int *weight, int *run_end) {
  const long long tile = (long long)blockIdx.x;
  const Contig c = contigs[tile_contig[tile]];
  const int lane = lane_id(), wave = wave_id();
  const long long tile_in_contig = tile - c.tile_first;
  const long long u = tile_in_contig * TILE + wave * WAVE_SPAN + lane * 4;
  Quad v0, v1, v2, v3;
  unsigned in0, in1, in2, in3;
  load_quad(c, u, v0, in0);
  load_quad(c, u + ROUND_SPAN, v1, in1);
  load_quad(c, u + 2 * ROUND_SPAN, v2, in2);
  load_quad(c, u + 3 * ROUND_SPAN, v3, in3);
  PSD_LDS int l_start[TILE], l_val[TILE], w_placed[WAVES];
  int placed = 0;
  int *ws = l_start + wave * WAVE_SPAN, *wv = l_val + wave * WAVE_SPAN;
  place_round(c, u, v0, in0, ws, wv, placed);
  place_round(c, u + ROUND_SPAN, v1, in1, ws, wv, placed);
  place_round(c, u + 2 * ROUND_SPAN, v2, in2, ws, wv, placed);
  place_round(c, u + 3 * ROUND_SPAN, v3, in3, ws, wv, placed);
  if (lane == 0) w_placed[wave] = placed;
  __syncthreads();
  const int p1 = w_placed[0], p2 = p1 + w_placed[1], p3 = p2 + w_placed[2];
  const int total = p3 + w_placed[3];
  /* run j of the tile lies in the part of the wave that placed it */
  auto slot = [&](int j) -> int {
    return j >= p3 ? 3 * WAVE_SPAN + j - p3
                   : j >= p2 ? 2 * WAVE_SPAN + j - p2 : j >= p1 ? WAVE_SPAN + j - p1 : j;
  };
  const TileScan ts = scan[tile];
  const long long out = c.run_off + ts.runs_before;
  /* a run's start writes its count and closes the run before it */
  for (int j = (int)threadIdx.x; j < total; j += THREADS) {
    const int sj = slot(j);
    const int start = l_start[sj];
    count[out + j] = l_val[sj];
    if (ts.runs_before + j > 0) {
      const int prev = j > 0 ? l_start[slot(j - 1)] : ts.open_start;
      run_end[out + j - 1] = start;
      weight[out + j - 1] = start - prev;
    }
  }
  const long long n_tiles = (c.lead + c.n + TILE - 1) / TILE;
  if (threadIdx.x == 0 && tile_in_contig == n_tiles - 1) { /* the contig's last run ends with it */
    const int last = total > 0 ? l_start[slot(total - 1)] : ts.open_start;
    run_end[out + total - 1] = (int)c.n;
    weight[out + total - 1] = (int)c.n - last;
  }
}

/* A workgroup per problem: the reference's segments table (chromStart, chromEnd, mean; the status
 * is the row's parity) from the problem's segment table and its contig's run_end[].
 * rows[3 p] = first packed row, rows[3 p + 1] = row count, rows[3 p + 2] = offset of the table in
 * seg_start / seg_mean; lay[3 p] = first run of the contig in run_end, lay[3 p + 1] = chromStart of
 * its first base, lay[3 p + 2] = its bases. */
__global__ void pack_segments_kernel(const int *seg_start, const double *seg_mean,
                                     const long long *rows, const long long *lay,
                                     const int *run_end, int *out_start, int *out_end,
                                     double *out_mean) {
  const long long to = rows[3 * blockIdx.x], n = rows[3 * blockIdx.x + 1],
                  from = rows[3 * blockIdx.x + 2];
  const long long run0 = lay[3 * blockIdx.x];
  const int first = (int)lay[3 * blockIdx.x + 1], bases = (int)lay[3 * blockIdx.x + 2];
  for (long long i = threadIdx.x; i < n; i += blockDim.x) {
    const int s = seg_start[from + i];
    out_start[to + i] = s < 0 ? first : first + run_end[run0 + s];
    if (i == 0) {
      out_end[to + i] = first + bases;
    } else {
      const int sp = seg_start[from + i - 1];
      out_end[to + i] = sp < 0 ? first : first + run_end[run0 + sp];
    }
    out_mean[to + i] = seg_mean[from + i];
  }
}

}  // namespace dense
}  // namespace psd
#endif
