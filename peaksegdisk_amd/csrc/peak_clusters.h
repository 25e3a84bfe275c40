/* peak_clusters.h -- which peaks of several models are the same peak: the clusters of overlapping
 * peaks over the members of a group, and what every member has under every cluster (DESIGN.md
 * section 15; PeakSegPipeline calls the first step clusterPeaks).
 *
 * A group has members (problems of a solved set, in increasing problem index); a member's peaks
 * [ps, pe) are the odd rows of its segments table in genomic coordinates.  Two peaks overlap when
 * ps_a < pe_b && ps_b < pe_a (abutting peaks do not); the clusters of a group are the connected
 * components of that relation over all peaks of all its members.  NOTE the order: the segments
 * tables hold their rows in DECREASING coordinates; here the peaks of a member are laid out in
 * INCREASING ps, and the clusters of a group are packed in INCREASING clusterStart.
 *
 * The peaks of all members lie in two flat arrays, group after group, member after member.  Every
 * member's peaks are sorted and disjoint, so no sort is needed, only ranks from binary searches:
 *   a peak LEADS a cluster  iff no peak q of another member has ps_q < ps < pe_q (only the last q
 *                           that starts before ps can), and no member before its own has a peak
 *                           with the same ps (of equal starts the first member leads);
 *   the cluster of a peak   is, among its group's clusters in increasing start, the number of
 *                           leaders with a start <= ps, less one: per member an upper bound of ps
 *                           and the prefix sum of the leader flags there.
 * Launches, whatever the numbers of problems, groups, members and peaks:
 *   gather_kernel  a thread per peak: ps and pe from the member's seg_start[] and its contig's
 *                  run_end[] (sets only: the probe is handed the arrays)
 *   mark_kernel    a thread per peak: the leader flag, and the workgroup's scan of the flags
 *                  (region_stats.h's block_scan; its scan_top_kernel completes the prefix sums)
 *   assign_kernel  a thread per peak: its cluster c; a 32-bit max to clusterEnd[c], a 32-bit add to
 *                  peaks[c], and the leader writes clusterStart[c]; a thread per group: its clusters
 *   -- the host reads the groups' cluster counts: the one download, 8 bytes per group --
 *   matrix_kernel  a thread per (cluster, member) entry: the member's peaks with ps < clusterEnd &&
 *                  clusterStart < pe by two binary searches, a 32-bit add to samples[c] where there
 *                  are any, and the cluster as a region of the member's contig, which
 *                  region_stats.h's three launches then fold into bases, sum and max.
 * Cost: mark and assign make one binary search per (peak, member of its group) pair, so
 * members x peaks x log2(peaks per member) probes per group, and 12 B read, 12 B written and two
 * atomics per peak; the matrix two searches and 16 B written per entry.  Integer atomics commute:
 * the results do not depend on the schedule.
 * Written against psd_platform.h only: the SIMT emulator of tests/emu runs this source. */
#ifndef PSD_PEAK_CLUSTERS_H
#define PSD_PEAK_CLUSTERS_H

#include "psd_platform.h"
#include "region_stats.h"

namespace psd {
namespace clusters {

constexpr int THREADS = psd::regions::THREADS;
constexpr int WAVES = THREADS / WAVE;

/* a member as gather_kernel reads it */
struct Member {
  long long seg_from; /* offset of its table in seg_start */
  long long run0;     /* first run of its contig in run_end */
  int n_segments;     /* rows of its table: 2 peaks + 1 */
  int first;          /* chromStart of its contig's first base */
};

/* the entries of v[0 .. n) below x (or, with `or_equal`, at most x); v increases */
PSD_D long long below(const int *v, long long n, int x, bool or_equal) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    const int e = v[mid];
    if (e < x || (or_equal && e == x))
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

/* the member of flat peak i: the last one whose first peak is not beyond i */
PSD_D int member_of(const long long *member_off, int n_members, long long i) {
  return (int)psd::regions::last_at_most(member_off, (long long)n_members, i);
}

/* peak j of a member in genomic order is row n_segments - 2 - 2 j of its table */
__global__ __launch_bounds__(THREADS) void gather_kernel(const Member *members,
                                                         const long long *member_off, int n_members,
                                                         long long n, const int *seg_start,
                                                         const int *run_end, int *peak_start,
                                                         int *peak_end) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= n) return;
  const int m = member_of(member_off, n_members, i);
  const Member *k = members + m;
  const long long row = k->n_segments - 2 - 2 * (i - member_off[m]);
  const int *table = seg_start + k->seg_from;
  peak_start[i] = k->first + run_end[k->run0 + table[row]];
  peak_end[i] = k->first + run_end[k->run0 + table[row - 1]];
}

/* A thread per entry of the flags' prefix sum: the n peaks and one entry more, which stands for
 * "all of them".  member_group[m]: the group of member m; group_member0[g .. g + 1]: its members.
 * No thread leaves before the scan. */
__global__ __launch_bounds__(THREADS) void mark_kernel(const long long *member_off, int n_members,
                                                       const int *member_group,
                                                       const int *group_member0, long long n,
                                                       const int *peak_start, const int *peak_end,
                                                       int *lead, int *off, long long *block_sum) {
  PSD_LDS int w_tot[WAVES];
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  int flag = 0;
  if (i < n) {
    const int m = member_of(member_off, n_members, i);
    const int g = member_group[m];
    const int x = peak_start[i];
    flag = 1;
    for (int o = group_member0[g]; o < group_member0[g + 1] && flag; o++) {
      if (o == m) continue;
      const long long lo = member_off[o], cnt = member_off[o + 1] - lo;
      const long long pos = below(peak_start + lo, cnt, x, false);
      if (pos > 0 && peak_end[lo + pos - 1] > x) flag = 0;              /* inside a peak */
      if (o < m && pos < cnt && peak_start[lo + pos] == x) flag = 0;    /* an earlier member leads */
    }
    lead[i] = flag;
  }
  int total;
  const int before = psd::regions::block_scan(flag, w_tot, total);
  if (i <= n) off[i] = before;
  if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

/* A thread per peak, and (the first n_groups threads) per group.  clusterEnd[] holds the smallest
 * int, peaks[] zeros. */
__global__ __launch_bounds__(THREADS) void assign_kernel(
    const long long *member_off, int n_members, const int *member_group, const int *group_member0,
    int n_groups, long long n, const int *peak_start, const int *peak_end, const int *lead,
    const int *off, const long long *block_sum, int *cluster_start, int *cluster_end,
    int *cluster_peaks, long long *group_clusters) {
  using psd::regions::scan_at;
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i < n_groups)
    group_clusters[i] = scan_at(off, block_sum, member_off[group_member0[i + 1]]) -
                        scan_at(off, block_sum, member_off[group_member0[i]]);
  if (i >= n) return;
  const int m = member_of(member_off, n_members, i);
  const int g = member_group[m];
  const int x = peak_start[i];
  long long c = scan_at(off, block_sum, member_off[group_member0[g]]) - 1;
  for (int o = group_member0[g]; o < group_member0[g + 1]; o++) {
    const long long lo = member_off[o], cnt = member_off[o + 1] - lo;
    const long long pos = below(peak_start + lo, cnt, x, true);
    c += scan_at(off, block_sum, lo + pos) - scan_at(off, block_sum, lo);
  }
  atomic_max_i32(cluster_end + c, peak_end[i]);
  atomic_add_i32(cluster_peaks + c, 1);
  if (lead[i]) cluster_start[c] = x;
}

/* A thread per entry e < n_entries.  entry_off[g], cluster_off[g]: the first entry and the first
 * cluster of group g (n_groups + 1 entries each); member_contig[m]: the contig of member m.
 * samples[] holds zeros.  region_start / region_end / region_contig may be NULL (the probe). */
__global__ __launch_bounds__(THREADS) void matrix_kernel(
    const long long *entry_off, const long long *cluster_off, int n_groups, long long n_entries,
    const long long *member_off, const int *group_member0, const int *member_contig,
    const int *peak_start, const int *peak_end, const int *cluster_start, const int *cluster_end,
    int *samples, int *m_peaks, int *region_start, int *region_end, int *region_contig) {
  const long long e = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (e >= n_entries) return;
  const int g = (int)psd::regions::last_at_most(entry_off, (long long)n_groups, e);
  const int members = group_member0[g + 1] - group_member0[g];
  const long long r = e - entry_off[g];
  const long long c = cluster_off[g] + r / members;
  const int m = group_member0[g] + (int)(r % members);
  const int cs = cluster_start[c], ce = cluster_end[c];
  const long long lo = member_off[m], cnt = member_off[m + 1] - lo;
  const long long k = below(peak_start + lo, cnt, ce, false) - below(peak_end + lo, cnt, cs, true);
  m_peaks[e] = (int)k;
  if (k > 0) atomic_add_i32(samples + c, 1);
  if (region_contig) {
    region_start[e] = cs;
    region_end[e] = ce;
    region_contig[e] = member_contig[m];
  }
}

}  // namespace clusters
}  // namespace psd
#endif
