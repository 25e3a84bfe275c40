/* peakseg_joint_path.h -- the host side of the joint peaks at many penalties (kernels:
 * joint_path.h): the check of the penalties, the launches level by level after joint_run()'s setup
 * (peakseg_joint.h does the checks of the groups and windows, the layout, the room and the head),
 * and the download of the columns.  The call keeps its own table, s->joint_path. */

namespace {

/* the search kernels are compiled for 1, 2, 4, 8 and 16 penalties' accumulators */
template <int PT>
int joint_path_search0(psd_problem_set *s, JointTable &t, const psd::joint::Groups &groups,
                       const psd::joint::Windows &win, long long windows, int n_pen,
                       const psd::joint_path::Penalties &pen) {
  namespace jn = psd::joint;
  hipLaunchKernelGGL(psd::joint_path::search0_kernel<PT>, dim3((unsigned)windows), dim3(jn::THREADS), 0,
                     s->stream, groups, windows, n_pen, pen, win, (const long long *)t.fold.sum, t.total,
                     t.carry);
  HIP_TRY(hipGetLastError());
  return 0;
}

template <int PT>
int joint_path_refine(psd_problem_set *s, JointTable &t, const psd::joint::Groups &groups,
                      const psd::joint::Windows &win, long long windows, long long entries, int n_pen,
                      const psd::joint_path::Penalties &pen) {
  namespace jn = psd::joint;
  hipLaunchKernelGGL(psd::joint_path::refine_kernel<PT>, dim3((unsigned)windows), dim3(jn::THREADS), 0,
                     s->stream, groups, windows, entries, n_pen, pen, win,
                     (const long long *)t.fold.sum, (const long long *)t.total);
  HIP_TRY(hipGetLastError());
  return 0;
}

int joint_path_launches(psd_problem_set *s, JointTable &t, const psd::joint::Groups &groups,
                        const psd::joint::Windows &win, int n_groups, long long windows,
                        long long entries, int n_pen, const double *penalties, int max_levels,
                        long long most_items, long long most_items_path) {
  namespace jn = psd::joint;
  namespace jp = psd::joint_path;
  RegionTable &ft = t.fold;
  int st = 0;
  jp::Penalties pen;
  for (int p = 0; p < jp::MAX_PENALTIES; p++) pen.v[p] = p < n_pen ? penalties[p] : HUGE_VAL;
  const int width = n_pen <= 1 ? 1 : n_pen <= 2 ? 2 : n_pen <= 4 ? 4 : n_pen <= 8 ? 8 : 16;
  auto fold = [&](long long n, long long items) -> int {
    return regions_fold(s, ft, n, (const int *)t.region_start, (const int *)t.region_end,
                        (const int *)t.region_contig, items, false, []() { return 0; });
  };
  auto pass = [&](int slots) -> int { /* a later level or the last pass: a piece per penalty */
    const long long n = entries * slots * n_pen;
    if (n == 0) return 0;
    hipLaunchKernelGGL(jp::bins_kernel<>, dim3((unsigned)((n + jn::THREADS - 1) / jn::THREADS)),
                       dim3(jn::THREADS), 0, s->stream, groups, n_groups, windows, entries, n_pen, slots,
                       win, (const int *)t.member_contig, t.region_start, t.region_end,
                       t.region_contig);
    HIP_TRY(hipGetLastError());
    return fold(n, most_items_path);
  };
  for (int level = 0; level < max_levels; level++) {
    if (level == 0) {
      /* the bins of level 0 are every penalty's: the rows of penalty 0 stand for all */
      const long long n = entries * jn::BINS;
      if (n > 0) {
        hipLaunchKernelGGL(jn::bins_kernel, dim3((unsigned)((n + jn::THREADS - 1) / jn::THREADS)),
                           dim3(jn::THREADS), 0, s->stream, groups, n_groups, entries, jn::BINS, win,
                           (const int *)t.member_contig, t.region_start, t.region_end,
                           t.region_contig);
        HIP_TRY(hipGetLastError());
        if ((st = fold(n, most_items))) return st;
      }
      st = width == 1   ? joint_path_search0<1>(s, t, groups, win, windows, n_pen, pen)
           : width == 2 ? joint_path_search0<2>(s, t, groups, win, windows, n_pen, pen)
           : width == 4 ? joint_path_search0<4>(s, t, groups, win, windows, n_pen, pen)
           : width == 8 ? joint_path_search0<8>(s, t, groups, win, windows, n_pen, pen)
                        : joint_path_search0<16>(s, t, groups, win, windows, n_pen, pen);
    } else {
      if ((st = pass(jn::REFINE))) return st;
      st = width == 1   ? joint_path_refine<1>(s, t, groups, win, windows, entries, n_pen, pen)
           : width == 2 ? joint_path_refine<2>(s, t, groups, win, windows, entries, n_pen, pen)
           : width == 4 ? joint_path_refine<4>(s, t, groups, win, windows, entries, n_pen, pen)
           : width == 8 ? joint_path_refine<8>(s, t, groups, win, windows, entries, n_pen, pen)
                        : joint_path_refine<16>(s, t, groups, win, windows, entries, n_pen, pen);
    }
    if (st) return st;
  }
  if ((st = pass(jn::FINAL))) return st;
  const long long cells = entries * n_pen;
  if (cells > 0) {
    hipLaunchKernelGGL(jp::report_kernel<>, dim3((unsigned)((cells + jn::THREADS - 1) / jn::THREADS)),
                       dim3(jn::THREADS), 0, s->stream, groups, n_groups, windows, entries, n_pen, pen,
                       win, (const long long *)ft.sum, t.m_gain, t.m_up, t.m_sum, t.m_bases);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

}  // namespace

extern "C" int peakseg_hip_joint_path_max_penalties(void) { return psd::joint_path::MAX_PENALTIES; }

extern "C" long long peakseg_hip_problem_set_pack_joint_path(
    psd_problem_set *s, const int *first_chromStart, int n_groups, const int *group, int n_penalties,
    const double *penalties, const long long *n_windows, const int *const *window_start,
    const int *const *window_end, int windows_on_device, long long *windows_out,
    long long *members_out, const int **windowStart_dev, const int **windowEnd_dev,
    const int **peakStart_dev, const int **peakEnd_dev, const double **objective_dev,
    const int **samples_up_dev, const int **levels_dev, const double **m_gain_dev,
    const int **m_up_dev, const long long **m_sum_dev, const int **m_bases_dev) {
  const char *who = "pack_joint_path";
  if (!s || (!n_windows && !s->solved)) return -1;
  if (!s->dense) {
    set_error("%s: the set was not made from dense counts or reads and has no run_end[]", who);
    return -1;
  }
  if (hipSetDevice(s->device) != hipSuccess) return -1;
  JointTable &t = s->joint_path;
  t.windows = t.entries = -1;
  s->joint_labels.labels = -1;
  if (first_chromStart_check(s, first_chromStart, who)) return -1;
  if (n_penalties < 1 || n_penalties > psd::joint_path::MAX_PENALTIES || !penalties) {
    set_error("%s: %d penalties%s, outside 1 .. %d", who, n_penalties,
              penalties ? "" : " and no array of them", psd::joint_path::MAX_PENALTIES);
    return -ERROR_REGION_ARGUMENTS;
  }
  for (int p = 0; p < n_penalties; p++)
    if (!(penalties[p] >= 0.0)) {
      set_error("%s: penalty %d, %g, is negative or not a number", who, p, penalties[p]);
      return -ERROR_REGION_ARGUMENTS;
    }
  if (const long long bad = joint_check_groups(s, who, n_groups, group, n_windows, window_start,
                                               window_end, windows_on_device))
    return bad;
  long long total = 0;
  const int st = joint_run(s, t, who, first_chromStart, n_groups, group, 0.0, n_penalties, penalties,
                           n_windows, window_start, window_end, n_windows ? windows_on_device : 0,
                           windows_out, members_out, &total);
  if (st) return st == ERROR_REGION_ARGUMENTS || st == ERROR_DEVICE_MEMORY ? -st : -1;
  t.windows = total;
  t.penalties = n_penalties;
  t.groups = n_groups;
  t.problem_group.assign(group, group + s->n_problems);
  if (windowStart_dev) *windowStart_dev = t.ws;
  if (windowEnd_dev) *windowEnd_dev = t.we;
  if (peakStart_dev) *peakStart_dev = t.s;
  if (peakEnd_dev) *peakEnd_dev = t.e;
  if (objective_dev) *objective_dev = t.objective;
  if (samples_up_dev) *samples_up_dev = t.samples_up;
  if (levels_dev) *levels_dev = t.levels;
  if (m_gain_dev) *m_gain_dev = t.m_gain;
  if (m_up_dev) *m_up_dev = t.m_up;
  if (m_sum_dev) *m_sum_dev = t.m_sum;
  if (m_bases_dev) *m_bases_dev = t.m_bases;
  return total;
}

extern "C" int peakseg_hip_problem_set_packed_joint_path_download(
    psd_problem_set *s, int *windowStart_out, int *windowEnd_out, int *peakStart_out,
    int *peakEnd_out, double *objective_out, int *samples_up_out, int *levels_out, double *m_gain_out,
    int *m_up_out, long long *m_sum_out, int *m_bases_out) {
  if (!s || s->joint_path.windows < 0) return -1;
  const JointTable &t = s->joint_path;
  const size_t k = (size_t)(t.windows * t.penalties), e = (size_t)(t.entries * t.penalties);
  const void *from[11] = {t.ws, t.we, t.s, t.e, t.objective, t.samples_up, t.levels,
                          t.m_gain, t.m_up, t.m_sum, t.m_bases};
  void *to[11] = {windowStart_out, windowEnd_out, peakStart_out, peakEnd_out, objective_out,
                  samples_up_out, levels_out, m_gain_out, m_up_out, m_sum_out, m_bases_out};
  const size_t bytes[11] = {k * 4, k * 4, k * 4, k * 4, k * 8, k * 4, k * 4, e * 8, e * 4, e * 8, e * 4};
  for (int j = 0; j < 11; j++)
    if (to[j] && bytes[j] > 0 && hipMemcpy(to[j], from[j], bytes[j], hipMemcpyDeviceToHost) != hipSuccess) {
      set_error("download of the packed joint path failed");
      return -1;
    }
  return 0;
}

extern "C" int peakseg_hip_joint_path_last_ms(float *ms) {
  if (ms) *ms = g_joint_path_ms;
  return 0;
}
