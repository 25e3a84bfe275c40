/* peakseg_labels.h -- the host side of the label errors (kernels: label_errors.h): the checks of
 * the labels, the descriptors, the two launches between two events, and the download. */

namespace {

thread_local float g_labels_ms = 0.f;

const char *const LABEL_WHAT[3] = {"chromStart", "chromEnd", "annotation"};

/* room for `need` entries of T behind p, which holds `have` of them (nothing is kept) */
template <class T>
int label_room(psd_problem_set *s, T *&p, long long have, long long need) {
  if (p && need <= have) return 0;
  dev_free(s, p, (unsigned long long)have * sizeof(T));
  return dev_alloc(s, &p, (size_t)need);
}

void label_error_text(int contig, long long index, long long ls, long long le, long long a, bool known) {
  if (!known)
    set_error("pack_label_errors: contig %d: label %lld has chromStart >= chromEnd or an annotation "
              "code outside 0..3", contig, index);
  else if (ls >= le)
    set_error("pack_label_errors: contig %d: label %lld has chromStart %lld >= chromEnd %lld", contig,
              index, ls, le);
  else
    set_error("pack_label_errors: contig %d: label %lld has annotation code %lld, outside 0..3", contig,
              index, a);
}

/* 0 or a status; the device is set and the arguments' shape has been checked.  *total_out: rows */
int labels_run(psd_problem_set *s, const int *first_chromStart, const long long *n_labels,
               const int *const *label_start, const int *const *label_end,
               const int *const *label_annotation, int on_device, long long *rows_out,
               long long *total_out) {
  namespace lb = psd::labels;
  LabelTable &t = s->labels;
  const size_t nc = (size_t)s->n_contigs, np = (size_t)s->n_problems;
  int st = 0;
  std::vector<long long> lab_off(nc + 1, 0);
  for (size_t c = 0; c < nc; c++) lab_off[c + 1] = lab_off[c] + n_labels[c];
  const long long n_all = lab_off[nc];
  std::vector<long long> desc(np * lb::DESC, 0);
  long long total = 0;
  for (size_t p = 0; p < np; p++) {
    const psd::ProbResult &r = s->results[p];
    const size_t c = (size_t)s->prob_contig[p];
    long long *d = desc.data() + p * lb::DESC;
    d[lb::D_TO] = total;
    d[lb::D_ROWS] = r.status == 0 ? r.n_segments : 0;
    d[lb::D_FROM] = s->prob_seg_off[p];
    d[lb::D_LAB0] = lab_off[c];
    if (rows_out) rows_out[p] = n_labels[c];
    total += n_labels[c];
  }
  /* (a grid dimension times the workgroup size stays below 2^32) */
  if ((total + lb::THREADS - 1) / lb::THREADS >= (1ll << 24)) {
    set_error("pack_label_errors: %lld rows in one call", total);
    return ERROR_LABEL_ARGUMENTS;
  }
  /* host arrays are checked here, before anything is allocated (translate_kernel checks what the
   * host cannot see) */
  for (size_t c = 0; c < nc && !on_device; c++)
    for (long long i = 0; i < n_labels[c]; i++) {
      const int ls = label_start[c][i], le = label_end[c][i], a = label_annotation[c][i];
      if (ls >= le || a < 0 || a > 3) {
        label_error_text((int)c, i, ls, le, a, true);
        return ERROR_LABEL_ARGUMENTS;
      }
    }
  for (auto &e : t.ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  /* (the set's geometry: their sizes never change) */
  if ((!t.d_contigs && (st = dev_alloc(s, &t.d_contigs, nc))) ||
      (!t.d_lab_off && (st = dev_alloc(s, &t.d_lab_off, nc + 1))) ||
      (!t.d_check && (st = dev_alloc(s, &t.d_check, nc))) ||
      (!t.d_desc && (st = dev_alloc(s, &t.d_desc, np * lb::DESC))) ||
      (!t.totals && (st = dev_alloc(s, &t.totals, np * lb::TOTALS))))
    return st;
  if (n_all > t.label_capacity || !t.where) {
    const long long need = n_all > 0 ? n_all : 1;
    const long long have = t.label_capacity;
    t.label_capacity = 0;
    if ((st = label_room(s, t.where, have, need)) ||
        (st = label_room(s, t.d_labels, 3 * have, 3 * need)))
      return st;
    t.label_capacity = need;
  }
  if (total > t.row_capacity || !t.count) {
    const long long need = total > 0 ? total : 1;
    const long long have = t.row_capacity;
    t.row_capacity = 0;
    if ((st = label_room(s, t.count, have, need)) || (st = label_room(s, t.fp, have, need)) ||
        (st = label_room(s, t.fn, have, need)))
      return st;
    t.row_capacity = need;
  }
  /* the contigs' labels: where the caller has them, or the library's copy of host arrays */
  std::vector<lb::Contig> contigs(nc);
  std::vector<int> host_copy;
  if (!on_device) host_copy.resize((size_t)(3 * n_all));
  for (size_t c = 0; c < nc; c++) {
    lb::Contig &k = contigs[c];
    const long long n = n_labels[c], off = lab_off[c];
    const int *from[3] = {n ? label_start[c] : nullptr, n ? label_end[c] : nullptr,
                          n ? label_annotation[c] : nullptr};
    if (!on_device) {
      for (int j = 0; j < 3; j++) {
        if (n) memcpy(host_copy.data() + j * n_all + off, from[j], sizeof(int) * (size_t)n);
        from[j] = t.d_labels + j * n_all + off;
      }
    }
    k.start = (const gint *)from[0];
    k.end = (const gint *)from[1];
    k.annotation = (const gint *)from[2];
    k.lab0 = off;
    k.run0 = s->contig_off[c];
    k.n_runs = s->contig_n[c];
    k.first = first_chromStart ? first_chromStart[c] : 0;
  }
  if (!on_device && n_all > 0)
    HIP_TRY(hipMemcpy(t.d_labels, host_copy.data(), sizeof(int) * host_copy.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t.d_contigs, contigs.data(), sizeof(lb::Contig) * nc, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t.d_lab_off, lab_off.data(), sizeof(long long) * (nc + 1), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t.d_desc, desc.data(), sizeof(long long) * desc.size(), hipMemcpyHostToDevice));
  /* (device arrays: what the caller queued on the null stream -- torch's default -- has run) */
  if (on_device) HIP_TRY(hipStreamSynchronize((hipStream_t) nullptr));
  HIP_TRY(hipEventRecord(t.ev[0], s->stream));
  HIP_TRY(hipMemsetAsync(t.totals, 0, sizeof(int) * np * lb::TOTALS, s->stream));
  HIP_TRY(hipMemsetAsync(t.d_check, 0, sizeof(unsigned long long) * nc, s->stream));
  if (n_all > 0) {
    hipLaunchKernelGGL(lb::translate_kernel, dim3((unsigned)((n_all + lb::THREADS - 1) / lb::THREADS)),
                       dim3(lb::THREADS), 0, s->stream, (const lb::Contig *)t.d_contigs,
                       (const long long *)t.d_lab_off, s->n_contigs, (const int *)s->d_run_end,
                       t.where, t.d_check);
    HIP_TRY(hipGetLastError());
    if (on_device) { /* nothing further is launched after a bad label */
      std::vector<unsigned long long> check(nc);
      HIP_TRY(hipMemcpyAsync(check.data(), t.d_check, sizeof(unsigned long long) * nc,
                             hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
      for (size_t c = 0; c < nc; c++)
        if (check[c]) {
          label_error_text((int)c, (long long)~check[c], 0, 0, 0, false);
          return ERROR_LABEL_ARGUMENTS;
        }
    }
  }
  if (total > 0) {
    hipLaunchKernelGGL(lb::count_kernel, dim3((unsigned)((total + lb::THREADS - 1) / lb::THREADS)),
                       dim3(lb::THREADS), 0, s->stream, (const long long *)t.d_desc, s->n_problems,
                       total, (const int *)s->d.seg_start, (const lb::Quad *)t.where, t.count, t.fp,
                       t.fn, t.totals);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(t.ev[1], s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipEventElapsedTime(&g_labels_ms, t.ev[0], t.ev[1]));
  *total_out = total;
  return 0;
}

}  // namespace

extern "C" long long peakseg_hip_problem_set_pack_label_errors(
    psd_problem_set *s, const int *first_chromStart, const long long *n_labels,
    const int *const *label_start, const int *const *label_end, const int *const *label_annotation,
    int labels_on_device, long long *rows_out, const int **count_dev, const int **fp_dev,
    const int **fn_dev, const int **totals_dev) {
  if (!s || !s->solved) return -1;
  if (!s->dense) {
    set_error("pack_label_errors: the set was not made from dense counts and has no run_end[]");
    return -1;
  }
  if (hipSetDevice(s->device) != hipSuccess) return -1;
  s->run.labels_total = -1;
  for (int c = 0; c < s->n_contigs; c++) {
    const long long first = first_chromStart ? first_chromStart[c] : 0;
    if (first < 0 || first + s->contig_bases[(size_t)c] > 2147483647ll) {
      set_error("pack_label_errors: contig %d: chromStart %lld + %lld bases is no 32-bit coordinate", c,
                first, s->contig_bases[(size_t)c]);
      return -1;
    }
  }
  if (!n_labels) {
    set_error("pack_label_errors: no label counts");
    return -ERROR_LABEL_ARGUMENTS;
  }
  for (int c = 0; c < s->n_contigs; c++) {
    if (n_labels[c] < 0) {
      set_error("pack_label_errors: contig %d has %lld labels", c, n_labels[c]);
      return -ERROR_LABEL_ARGUMENTS;
    }
    if (n_labels[c] == 0) continue;
    const int *const *arrays[3] = {label_start, label_end, label_annotation};
    for (int j = 0; j < 3; j++) {
      const int *a = arrays[j] ? arrays[j][c] : nullptr;
      if (!a || (labels_on_device && ((unsigned long long)a & 3ull))) {
        set_error("pack_label_errors: contig %d: the %s array is %s", c, LABEL_WHAT[j],
                  a ? "at a device address that is no multiple of 4" : "NULL");
        return -ERROR_LABEL_ARGUMENTS;
      }
    }
  }
  long long total = 0;
  const int st = labels_run(s, first_chromStart, n_labels, label_start, label_end, label_annotation,
                            labels_on_device, rows_out, &total);
  if (st) return st == ERROR_LABEL_ARGUMENTS ? -ERROR_LABEL_ARGUMENTS : -1;
  s->run.labels_total = total;
  if (count_dev) *count_dev = s->labels.count;
  if (fp_dev) *fp_dev = s->labels.fp;
  if (fn_dev) *fn_dev = s->labels.fn;
  if (totals_dev) *totals_dev = s->labels.totals;
  return total;
}

extern "C" int peakseg_hip_problem_set_packed_label_errors_download(psd_problem_set *s, int *count_out,
                                                                    int *fp_out, int *fn_out,
                                                                    int *totals_out) {
  if (!s || !s->solved || s->run.labels_total < 0) return -1;
  const size_t n = (size_t)s->run.labels_total;
  const LabelTable &t = s->labels;
  const void *from[4] = {t.count, t.fp, t.fn, t.totals};
  void *to[4] = {count_out, fp_out, fn_out, totals_out};
  const size_t entries[4] = {n, n, n, (size_t)s->n_problems * psd::labels::TOTALS};
  for (int k = 0; k < 4; k++)
    if (to[k] && entries[k] > 0 &&
        hipMemcpy(to[k], from[k], entries[k] * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) {
      set_error("download of the packed label errors failed");
      return -1;
    }
  return 0;
}

extern "C" int peakseg_hip_label_errors_last_ms(float *ms) {
  if (ms) *ms = g_labels_ms;
  return 0;
}
