/* peakseg_joint_labels.h -- the host side of the label errors of a packed joint path (kernels:
 * joint_labels.h): the checks of the labels, the problems' descriptors, the two launches between
 * two events, and the download. */

namespace {

thread_local float g_joint_labels_ms = 0.f;

void joint_label_error_text(int problem, long long index, long long ls, long long le, long long a,
                            bool known) {
  const char *who = "pack_joint_label_errors";
  if (!known)
    set_error("%s: problem %d: label %lld has chromStart >= chromEnd or an annotation code outside "
              "0..3", who, problem, index);
  else if (ls >= le)
    set_error("%s: problem %d: label %lld has chromStart %lld >= chromEnd %lld", who, problem, index,
              ls, le);
  else
    set_error("%s: problem %d: label %lld has annotation code %lld, outside 0..3", who, problem, index,
              a);
}

/* 0 or a status; the device is set and the arguments' shape has been checked */
int joint_labels_run(psd_problem_set *s, const long long *n_labels, const int *const *label_start,
                     const int *const *label_end, const int *const *label_annotation, int on_device,
                     long long *total_out) {
  namespace jl = psd::joint_labels;
  namespace jn = psd::joint;
  JointLabelTable &t = s->joint_labels;
  const JointTable &path = s->joint_path;
  const size_t np = (size_t)s->n_problems;
  const long long n_pen = path.penalties;
  int st = 0;
  std::vector<long long> lab_off(np + 1, 0);
  for (size_t q = 0; q < np; q++) lab_off[q + 1] = lab_off[q] + n_labels[q];
  const long long n_all = lab_off[np], rows = n_all * n_pen, cells = (long long)np * n_pen;
  /* (a grid dimension times the workgroup size stays below 2^32; the totals' keys are ints) */
  if ((rows + jl::THREADS - 1) / jl::THREADS >= (1ll << 24) || cells * jl::TOTALS >= (1ll << 31)) {
    set_error("pack_joint_label_errors: %lld rows and %lld totals in one call", rows, cells);
    return ERROR_LABEL_ARGUMENTS;
  }
  /* host arrays are checked here, before anything is allocated (count_kernel checks what the host
   * cannot see) */
  for (size_t q = 0; q < np && !on_device; q++)
    for (long long i = 0; i < n_labels[q]; i++) {
      const int ls = label_start[q][i], le = label_end[q][i], a = label_annotation[q][i];
      if (ls >= le || a < 0 || a > 3) {
        joint_label_error_text((int)q, i, ls, le, a, true);
        return ERROR_LABEL_ARGUMENTS;
      }
    }
  for (auto &e : t.ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  /* (the set's geometry: their sizes never change) */
  if ((!t.d_problems && (st = dev_alloc(s, &t.d_problems, np))) ||
      (!t.d_lab_off && (st = dev_alloc(s, &t.d_lab_off, np + 1))) ||
      (!t.d_check && (st = dev_alloc(s, &t.d_check, np))) ||
      (!t.model && (st = dev_alloc(s, &t.model, (size_t)(psd::joint_path::MAX_PENALTIES * jl::TOTALS)))))
    return st;
  if (n_all > t.label_capacity || !t.d_labels) {
    const long long need = n_all > 0 ? n_all : 1, have = t.label_capacity;
    t.label_capacity = 0;
    if ((st = label_room(s, t.d_labels, 3 * have, 3 * need))) return st;
    t.label_capacity = need;
  }
  if (rows > t.row_capacity || !t.count) {
    const long long need = rows > 0 ? rows : 1, have = t.row_capacity;
    t.row_capacity = 0;
    if ((st = label_room(s, t.count, have, need)) || (st = label_room(s, t.fp, have, need)) ||
        (st = label_room(s, t.fn, have, need)))
      return st;
    t.row_capacity = need;
  }
  if (cells > t.total_capacity || !t.totals) {
    const long long need = cells > 0 ? cells : 1, have = t.total_capacity;
    t.total_capacity = 0;
    if ((st = label_room(s, t.totals, jl::TOTALS * have, jl::TOTALS * need))) return st;
    t.total_capacity = need;
  }
  /* the problems' labels: where the caller has them, or the library's copy of host arrays */
  std::vector<jl::Problem> problems(np);
  std::vector<int> host_copy;
  if (!on_device) host_copy.resize((size_t)(3 * n_all));
  for (size_t q = 0; q < np; q++) {
    jl::Problem &k = problems[q];
    const long long n = n_labels[q], off = lab_off[q];
    const int *from[3] = {n ? label_start[q] : nullptr, n ? label_end[q] : nullptr,
                          n ? label_annotation[q] : nullptr};
    if (!on_device) {
      for (int j = 0; j < 3; j++) {
        if (n) memcpy(host_copy.data() + j * n_all + off, from[j], sizeof(int) * (size_t)n);
        from[j] = t.d_labels + j * n_all + off;
      }
    }
    k.start = (const gint *)from[0];
    k.end = (const gint *)from[1];
    k.annotation = (const gint *)from[2];
    k.group = path.problem_group[q];
    k.member = path.problem_member[q];
  }
  if (!on_device && n_all > 0)
    HIP_TRY(hipMemcpy(t.d_labels, host_copy.data(), sizeof(int) * host_copy.size(), hipMemcpyHostToDevice));
  if (np > 0)
    HIP_TRY(hipMemcpy(t.d_problems, problems.data(), sizeof(jl::Problem) * np, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t.d_lab_off, lab_off.data(), sizeof(long long) * (np + 1), hipMemcpyHostToDevice));
  jn::Groups groups;
  groups.member0 = path.member0;
  groups.win_off = path.win_off;
  groups.entry_off = path.entry_off;
  groups.lo = path.lo;
  groups.hi = path.hi;
  groups.start = (const gint *const *)(const void *)path.g_start;
  groups.end = (const gint *const *)(const void *)path.g_end;
  /* (device arrays: what the caller queued on the null stream -- torch's default -- has run) */
  if (on_device) HIP_TRY(hipStreamSynchronize((hipStream_t) nullptr));
  HIP_TRY(hipEventRecord(t.ev[0], s->stream));
  HIP_TRY(hipMemsetAsync(t.totals, 0, sizeof(int) * (size_t)(cells > 0 ? cells : 1) * jl::TOTALS, s->stream));
  HIP_TRY(hipMemsetAsync(t.model, 0, sizeof(long long) * psd::joint_path::MAX_PENALTIES * jl::TOTALS,
                         s->stream));
  HIP_TRY(hipMemsetAsync(t.d_check, 0, sizeof(unsigned long long) * (np ? np : 1), s->stream));
  g_joint_labels_ms = 0.f;
  if (rows > 0) {
    hipLaunchKernelGGL(jl::count_kernel<>, dim3((unsigned)((rows + jl::THREADS - 1) / jl::THREADS)),
                       dim3(jl::THREADS), 0, s->stream, (const jl::Problem *)t.d_problems,
                       (const long long *)t.d_lab_off, s->n_problems, (int)n_pen, groups, path.windows,
                       path.entries, (const int *)path.s, (const int *)path.e, (const int *)path.m_up,
                       t.count, t.fp, t.fn, t.totals, t.d_check);
    HIP_TRY(hipGetLastError());
    if (on_device) { /* nothing further is launched after a bad label */
      std::vector<unsigned long long> check(np);
      HIP_TRY(hipMemcpyAsync(check.data(), t.d_check, sizeof(unsigned long long) * np,
                             hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
      for (size_t q = 0; q < np; q++)
        if (check[q]) {
          joint_label_error_text((int)q, (long long)~check[q], 0, 0, 0, false);
          return ERROR_LABEL_ARGUMENTS;
        }
    }
    if (np > 0) {
      hipLaunchKernelGGL(jl::sum_kernel<>, dim3((unsigned)n_pen), dim3(jl::THREADS), 0, s->stream,
                         (const int *)t.totals, s->n_problems, t.model);
      HIP_TRY(hipGetLastError());
    }
  }
  HIP_TRY(hipEventRecord(t.ev[1], s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipEventElapsedTime(&g_joint_labels_ms, t.ev[0], t.ev[1]));
  *total_out = n_all;
  return 0;
}

}  // namespace

extern "C" long long peakseg_hip_problem_set_pack_joint_label_errors(
    psd_problem_set *s, const long long *n_labels, const int *const *label_start,
    const int *const *label_end, const int *const *label_annotation, int labels_on_device,
    const int **count_dev, const int **fp_dev, const int **fn_dev, const int **problem_totals_dev,
    const long long **model_totals_dev) {
  if (!s || s->joint_path.windows < 0) return -1;
  if (hipSetDevice(s->device) != hipSuccess) return -1;
  s->joint_labels.labels = -1;
  if (!n_labels && s->n_problems > 0) {
    set_error("pack_joint_label_errors: no label counts");
    return -ERROR_LABEL_ARGUMENTS;
  }
  for (int q = 0; q < s->n_problems; q++) {
    if (n_labels[q] < 0) {
      set_error("pack_joint_label_errors: problem %d has %lld labels", q, n_labels[q]);
      return -ERROR_LABEL_ARGUMENTS;
    }
    if (n_labels[q] == 0) continue;
    const int *const *arrays[3] = {label_start, label_end, label_annotation};
    for (int j = 0; j < 3; j++) {
      const int *a = arrays[j] ? arrays[j][q] : nullptr;
      if (!a || (labels_on_device && ((unsigned long long)a & 3ull))) {
        set_error("pack_joint_label_errors: problem %d: the %s array is %s", q, LABEL_WHAT[j],
                  a ? "at a device address that is no multiple of 4" : "NULL");
        return -ERROR_LABEL_ARGUMENTS;
      }
    }
  }
  long long total = 0;
  const int st = joint_labels_run(s, n_labels, label_start, label_end, label_annotation,
                                  labels_on_device, &total);
  if (st) return st == ERROR_LABEL_ARGUMENTS ? -ERROR_LABEL_ARGUMENTS : -1;
  JointLabelTable &t = s->joint_labels;
  t.labels = total;
  t.penalties = s->joint_path.penalties;
  if (count_dev) *count_dev = t.count;
  if (fp_dev) *fp_dev = t.fp;
  if (fn_dev) *fn_dev = t.fn;
  if (problem_totals_dev) *problem_totals_dev = t.totals;
  if (model_totals_dev) *model_totals_dev = t.model;
  return total;
}

extern "C" int peakseg_hip_problem_set_packed_joint_label_errors_download(
    psd_problem_set *s, int *count_out, int *fp_out, int *fn_out, int *problem_totals_out,
    long long *model_totals_out) {
  if (!s || s->joint_labels.labels < 0) return -1;
  const JointLabelTable &t = s->joint_labels;
  const size_t n = (size_t)(t.labels * t.penalties);
  const void *from[5] = {t.count, t.fp, t.fn, t.totals, t.model};
  void *to[5] = {count_out, fp_out, fn_out, problem_totals_out, model_totals_out};
  const size_t bytes[5] = {n * 4, n * 4, n * 4,
                           (size_t)s->n_problems * (size_t)t.penalties * psd::joint_labels::TOTALS * 4,
                           (size_t)t.penalties * psd::joint_labels::TOTALS * 8};
  for (int k = 0; k < 5; k++)
    if (to[k] && bytes[k] > 0 && hipMemcpy(to[k], from[k], bytes[k], hipMemcpyDeviceToHost) != hipSuccess) {
      set_error("download of the packed joint label errors failed");
      return -1;
    }
  return 0;
}

extern "C" int peakseg_hip_joint_label_errors_last_ms(float *ms) {
  if (ms) *ms = g_joint_labels_ms;
  return 0;
}
