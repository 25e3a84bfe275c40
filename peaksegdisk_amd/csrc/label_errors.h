/* label_errors.h -- the label errors of every model of a solved set, counted on the device from
 * the segment tables and the runs resident in HBM (the PeakError convention).
 *
 * A label is [ls, le) with an annotation; a peak is an odd row [ps, pe) of the segments table.
 *   noPeaks    count = peaks with ps < le && ls < pe   false positive: count >= 1
 *   peaks      count = the same                        false negative: count == 0
 *   peakStart  count = peaks with ls <= ps < le        fp: count >= 2, fn: count == 0
 *   peakEnd    count = peaks with ls < pe <= le        fp: count >= 2, fn: count == 0
 * With the boundaries b_1 < ... < b_{S-1} of a model of S segments (odd k: a peak's start, even k:
 * a peak's end), L(x) = #{k : b_k < x} and E(x) = #{k : b_k <= x}:
 *   starts in the label = (L(le) + 1) / 2 - (L(ls) + 1) / 2
 *   ends in the label   = E(le) / 2 - E(ls) / 2
 *   overlapping         = (L(le) + 1) / 2 - E(ls) / 2
 *
 * The boundaries are run indices: b_k = first + run_end[run0 + j_k] with j_k = seg_start[S - 1 - k]
 * (segment_stats.h has the row-to-runs relation), so seg_start[0 .. S - 2] holds them in decreasing
 * order.  run_end increases strictly: with A(x) = the runs of the contig that end before x,
 * b_k < x iff j_k < A(x), and b_k <= x iff j_k < A(x) + 1 where a run ends exactly at x.
 *
 * Two launches per call, however many problems and labels there are; no workgroup waits for another:
 *   translate_kernel  a thread per (contig, label): A(ls) and A(le) by binary search of the contig's
 *                     run_end[], each with the bit "a run ends exactly here", kept with the
 *                     annotation in 16 bytes per label.  Once per contig: the problems of a contig
 *                     (the penalties of a grid) share it.  A coordinate outside the contig needs no
 *                     special case: no run ends before its first base, all end before what lies
 *                     beyond its last.  A label with ls >= le or an annotation outside 0..3 is bad:
 *                     the contig's check word keeps the first one (key = ~index, a 64-bit max on a
 *                     zeroed word, as reads_pileup.h's scatter kernel keeps its first bad read).
 *   count_kernel      a thread per (problem, label): two binary searches of the problem's
 *                     seg_start[] give L at both ends, the entry next to where each search ends
 *                     gives E; count, fp and fn go to the packed columns.  The totals of a problem
 *                     (errors, fp, fn, possible fp, possible fn) are formed by a segmented scan over
 *                     the lanes of a wave (a wave's rows belong to consecutive problems) and one
 *                     32-bit add per total for every (wave, problem) pair, on zeroed words.
 * Integer adds commute: the results do not depend on the schedule.
 * Algorithmic traffic: per (contig, label) 12 B of label, 2 ceil(log2(R + 1)) probes of run_end for
 * R runs and 16 B written; per (problem, label) those 16 B, 2 ceil(log2 S) + 2 probes of seg_start
 * for S segments and 12 B written; per (wave, problem) at most five 4-byte atomics.
 * Written against psd_platform.h only: the SIMT emulator of tests/emu runs this source. */
#ifndef PSD_LABEL_ERRORS_H
#define PSD_LABEL_ERRORS_H

#include "dense_encode.h"
#include "psd_platform.h"

namespace psd {
namespace labels {

constexpr int THREADS = 256;
constexpr int DESC = 4;   /* long longs per problem in the descriptor array */
constexpr int TOTALS = 5; /* ints per problem: errors, fp, fn, possible fp, possible fn */

typedef unsigned long long u64;
typedef psd::dense::Quad Quad;

enum { NO_PEAKS = 0, PEAK_START = 1, PEAK_END = 2, PEAKS = 3 };

/* per problem, desc[DESC p + ...] */
enum {
  D_TO = 0,   /* first packed row */
  D_ROWS = 1, /* rows of its segment table (0: not solved, its labels get zeros) */
  D_FROM = 2, /* offset of the table in seg_start */
  D_LAB0 = 3, /* index of its contig's first label among all labels of the call */
};

struct Contig {
  const gint *start, *end, *annotation; /* the contig's labels */
  long long lab0;                       /* index of its first label among all labels */
  long long run0, n_runs;               /* its runs in run_end[] */
  long long first;                      /* chromStart of its first base */
};

/* the runs of the contig that end before x (a coordinate relative to the contig's first base),
 * doubled, plus one when a run ends exactly at x */
PSD_D int runs_before(const int *run_end, long long n_runs, long long x) {
  long long lo = 0, hi = n_runs; /* the first run whose end is not before x */
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if ((long long)run_end[mid] < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int exact = lo < n_runs && (long long)run_end[lo] == x ? 1 : 0;
  return (int)(2 * lo) + exact;
}

/* lab_off[c .. c + 1]: the labels of contig c among all labels (n_contigs + 1 entries) */
__global__ __launch_bounds__(THREADS) void translate_kernel(const Contig *contigs,
                                                            const long long *lab_off, int n_contigs,
                                                            const int *run_end, Quad *where,
                                                            u64 *check) {
  const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (g >= lab_off[n_contigs]) return;
  int lo = 0, hi = n_contigs - 1; /* the last contig whose first label is not beyond g */
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (lab_off[mid] <= g)
      lo = mid;
    else
      hi = mid - 1;
  }
  const Contig *c = contigs + lo;
  const long long i = g - c->lab0;
  const int ls = c->start[i], le = c->end[i], a = c->annotation[i];
  if (ls >= le || a < 0 || a > 3) atomic_max_u64(check + lo, ~(u64)i);
  const int *ends = run_end + c->run0;
  Quad q;
  q.x = runs_before(ends, c->n_runs, (long long)ls - c->first);
  q.y = runs_before(ends, c->n_runs, (long long)le - c->first);
  q.z = a;
  q.w = 0;
  where[g] = q;
}

/* L and E of a coordinate in a model: table[0 .. nb) holds the boundaries' runs in decreasing
 * order, t is what runs_before() gave for the coordinate */
PSD_D void boundaries_before(const int *table, long long nb, int t, int &L, int &E) {
  const int before = t >> 1;
  long long lo = 0, hi = nb; /* the first entry that is < before */
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (table[mid] < before)
      hi = mid;
    else
      lo = mid + 1;
  }
  L = (int)(nb - lo);
  E = L + ((t & 1) && lo > 0 && table[lo - 1] == before ? 1 : 0);
}

/* A thread per packed row; its problem is the last one whose first packed row is not beyond it
 * (segment_stats.h's finish_kernel).  No lane leaves before the scan. */
__global__ __launch_bounds__(THREADS) void count_kernel(const long long *desc, int n_problems,
                                                        long long total, const int *seg_start,
                                                        const Quad *where, int *count, int *fp,
                                                        int *fn, int *totals) {
  const long long row = (long long)blockIdx.x * THREADS + threadIdx.x;
  const int lane = lane_id();
  int problem = -1, packed = 0;
  if (row < total) {
    int lo = 0, hi = n_problems - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) / 2;
      if (desc[(long long)DESC * mid + D_TO] <= row)
        lo = mid;
      else
        hi = mid - 1;
    }
    problem = lo;
    const long long *d = desc + (long long)DESC * lo;
    const long long nb = d[D_ROWS] - 1;
    const Quad q = where[d[D_LAB0] + (row - d[D_TO])];
    int n = 0;
    if (nb > 0) {
      const int *table = seg_start + d[D_FROM];
      int Ls, Es, Le, Ee;
      boundaries_before(table, nb, q.x, Ls, Es);
      boundaries_before(table, nb, q.y, Le, Ee);
      if (q.z == PEAK_START)
        n = (Le + 1) / 2 - (Ls + 1) / 2;
      else if (q.z == PEAK_END)
        n = Ee / 2 - Es / 2;
      else
        n = (Le + 1) / 2 - Es / 2;
    }
    const bool solved = nb >= 0;
    const int many = q.z == NO_PEAKS ? 1 : 2;
    const int is_fp = solved && q.z != PEAKS && n >= many ? 1 : 0;
    const int is_fn = solved && q.z != NO_PEAKS && n == 0 ? 1 : 0;
    count[row] = n;
    fp[row] = is_fp;
    fn[row] = is_fn;
    /* four sums of at most 64 ones each, a byte apiece */
    packed = is_fp | (is_fn << 8) | ((q.z != PEAKS ? 1 : 0) << 16) | ((q.z != NO_PEAKS ? 1 : 0) << 24);
  }
  /* inclusive scan over the lanes of the same problem (problems do not decrease with the lane) */
  for (int off = 1; off < WAVE; off <<= 1) {
    const int src = lane >= off ? lane - off : lane;
    const int o = shfl_i(packed, src), o_problem = shfl_i(problem, src);
    if (lane >= off && o_problem == problem) packed += o;
  }
  const int next = shfl_i(problem, lane < WAVE - 1 ? lane + 1 : lane);
  if (problem >= 0 && (lane == WAVE - 1 || next != problem)) { /* a problem's last lane in the wave */
    int *t = totals + (long long)TOTALS * problem;
    const int s_fp = packed & 255, s_fn = (packed >> 8) & 255, s_pfp = (packed >> 16) & 255,
              s_pfn = (packed >> 24) & 255;
    if (s_fp + s_fn) atomic_add_i32(t, s_fp + s_fn);
    if (s_fp) atomic_add_i32(t + 1, s_fp);
    if (s_fn) atomic_add_i32(t + 2, s_fn);
    if (s_pfp) atomic_add_i32(t + 3, s_pfp);
    if (s_pfn) atomic_add_i32(t + 4, s_pfn);
  }
}

}  // namespace labels
}  // namespace psd
#endif
