/* joint_labels.h -- the label errors of every model of a packed joint path (joint_path.h), counted
 * on the device from its columns (the PeakError convention of label_errors.h).
 *
 * A label [ls, le) with an annotation belongs to a problem and is in genomic coordinates, as the
 * joint peaks are.  The peaks of problem q in model p: the joint peaks [ps, pe) of the windows w of
 * q's group with ps >= 0 and m_up[p, w, member of q] == 1 -- every window's, also where two
 * windows' peaks overlap or coincide.  A problem in no group has none.
 *   noPeaks    count = peaks with ps < le && ls < pe   false positive: count >= 1
 *   peaks      count = the same                        false negative: count == 0
 *   peakStart  count = peaks with ls <= ps < le        fp: count >= 2, fn: count == 0
 *   peakEnd    count = peaks with ls < pe <= le        fp: count >= 2, fn: count == 0
 *
 * Two launches per call, however many penalties, problems, labels and windows there are:
 *   count_kernel  a thread per (penalty, label), penalty-major: a loop over the windows of the
 *                 problem's group (they come in any order and may overlap: no search applies),
 *                 count, fp and fn to the packed columns; the totals of (penalty, problem) by
 *                 label_errors.h's segmented scan over the lanes of a wave and one 32-bit add per
 *                 total for every (wave, penalty, problem), on zeroed words.  A label with
 *                 ls >= le or an annotation outside 0..3 is bad: its problem's check word keeps
 *                 the first one (key = ~index, a 64-bit max on a zeroed word).
 *   sum_kernel    a workgroup per penalty: its five totals over the problems, as 64-bit integers.
 * Integer adds commute: the results do not depend on the schedule.
 * Both kernels are templates (`template <int = 0>`) for their place in the code object: joint_path.h
 * says why.
 * Written against psd_platform.h only: the SIMT emulator of tests/emu runs this source. */
#ifndef PSD_JOINT_LABELS_H
#define PSD_JOINT_LABELS_H

#include "joint_peaks.h"
#include "label_errors.h"

namespace psd {
namespace joint_labels {

using psd::labels::NO_PEAKS;
using psd::labels::PEAKS;
using psd::labels::PEAK_END;
using psd::labels::PEAK_START;
using psd::labels::THREADS;
using psd::labels::TOTALS;
typedef unsigned long long u64;

struct Problem {
  const gint *start, *end, *annotation; /* its labels */
  int group;                            /* -1: in no group */
  int member;                           /* its index among the group's members */
};

/* n_labels: labels of all problems, lab_off[q .. q + 1] those of problem q; the path's columns:
 * peak_start, peak_end at p * n_windows + w, m_up at p * n_entries + entry. */
template <int = 0>
__global__ __launch_bounds__(THREADS) void count_kernel(
    const Problem *problems, const long long *lab_off, int n_problems, int n_pen,
    psd::joint::Groups g, long long n_windows, long long n_entries, const int *peak_start,
    const int *peak_end, const int *m_up, int *count, int *fp, int *fn, int *totals, u64 *check) {
  const long long n_labels = lab_off[n_problems];
  const long long x = (long long)blockIdx.x * THREADS + threadIdx.x;
  const int lane = lane_id();
  int key = -1, packed = 0;
  if (x < n_labels * n_pen) {
    const long long p = x / n_labels, row = x % n_labels;
    const int q = (int)psd::regions::last_at_most(lab_off, (long long)n_problems, row);
    const Problem *pr = problems + q;
    const long long i = row - lab_off[q];
    const int ls = pr->start[i], le = pr->end[i], a = pr->annotation[i];
    if (ls >= le || a < 0 || a > 3) atomic_max_u64(check + q, ~(u64)i);
    int n = 0;
    if (pr->group >= 0) {
      const int k = pr->group;
      const long long members = g.member0[k + 1] - g.member0[k];
      const long long w0 = g.win_off[k], w1 = g.win_off[k + 1];
      const int *ps = peak_start + p * n_windows, *pe = peak_end + p * n_windows;
      const int *up = m_up + p * n_entries + g.entry_off[k] + pr->member;
      for (long long w = w0; w < w1; w++) {
        const int s = ps[w], e = pe[w];
        if (s < 0 || up[(w - w0) * members] != 1) continue;
        if (a == PEAK_START)
          n += ls <= s && s < le;
        else if (a == PEAK_END)
          n += ls < e && e <= le;
        else
          n += s < le && ls < e;
      }
    }
    const int many = a == NO_PEAKS ? 1 : 2;
    const int is_fp = a != PEAKS && n >= many ? 1 : 0;
    const int is_fn = a != NO_PEAKS && n == 0 ? 1 : 0;
    count[x] = n;
    fp[x] = is_fp;
    fn[x] = is_fn;
    key = (int)p * n_problems + q;
    /* four sums of at most 64 ones each, a byte apiece */
    packed = is_fp | (is_fn << 8) | ((a != PEAKS ? 1 : 0) << 16) | ((a != NO_PEAKS ? 1 : 0) << 24);
  }
  /* inclusive scan over the lanes of the same (penalty, problem): keys do not decrease with the lane */
  for (int off = 1; off < WAVE; off <<= 1) {
    const int src = lane >= off ? lane - off : lane;
    const int o = shfl_i(packed, src), o_key = shfl_i(key, src);
    if (lane >= off && o_key == key) packed += o;
  }
  const int next = shfl_i(key, lane < WAVE - 1 ? lane + 1 : lane);
  if (key >= 0 && (lane == WAVE - 1 || next != key)) { /* a key's last lane in the wave */
    int *t = totals + (long long)TOTALS * key;
    const int s_fp = packed & 255, s_fn = (packed >> 8) & 255, s_pfp = (packed >> 16) & 255,
              s_pfn = (packed >> 24) & 255;
    if (s_fp + s_fn) atomic_add_i32(t, s_fp + s_fn);
    if (s_fp) atomic_add_i32(t + 1, s_fp);
    if (s_fn) atomic_add_i32(t + 2, s_fn);
    if (s_pfp) atomic_add_i32(t + 3, s_pfp);
    if (s_pfn) atomic_add_i32(t + 4, s_pfn);
  }
}

/* A workgroup per penalty p: model[5 p + j] = the sum over the problems of totals[5 (p n + q) + j];
 * model holds zeros. */
template <int = 0>
__global__ __launch_bounds__(THREADS) void sum_kernel(const int *totals, int n_problems,
                                                      long long *model) {
  const int p = (int)blockIdx.x;
  const int *from = totals + (long long)TOTALS * p * n_problems;
  for (int j = 0; j < TOTALS; j++) {
    long long part = 0;
    for (int q = (int)threadIdx.x; q < n_problems; q += THREADS) part += from[(long long)TOTALS * q + j];
    if (part) atomic_add_i64(model + (long long)TOTALS * p + j, part);
  }
}

}  // namespace joint_labels
}  // namespace psd
#endif
