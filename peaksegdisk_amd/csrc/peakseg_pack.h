/* peakseg_pack.h -- segment tables packed in HBM at their exact sizes (the multi-GPU gather's
 * payload) and their downloads: (start, mean) of any set, and the reference's segments table of
 * a set made from dense counts (its kernel is in dense_encode.h). */

/* one workgroup per problem: rows[3 p] = first packed row, rows[3 p + 1] = row count,
 * rows[3 p + 2] = the table's offset in seg_start / seg_mean */
__global__ void pack_tables_kernel(const int *seg_start, const double *seg_mean,
                                   const long long *rows, int *out_start, double *out_mean) {
  const long long to = rows[3 * blockIdx.x], n = rows[3 * blockIdx.x + 1],
                  from = rows[3 * blockIdx.x + 2];
  for (long long i = threadIdx.x; i < n; i += blockDim.x) {
    out_start[to + i] = seg_start[from + i];
    out_mean[to + i] = seg_mean[from + i];
  }
}

namespace {

/* What both packers do but for their kernel: rows[3 p ..] of every problem as the kernels read
 * them, room for the packed rows in columns of col_bytes[] bytes per entry (0: no such column;
 * columns that are too small are replaced), the rows array on the device, launch(), and the wait
 * for it on the set's stream.  Returns the packed rows in all, or -1. */
template <class Launch>
long long pack(psd_problem_set *s, PackedTable &t, const size_t (&col_bytes)[3],
               std::vector<long long> &rows, long long *rows_out, const char *what, Launch launch) {
  long long total = 0;
  for (int p = 0; p < s->n_problems; p++) {
    const psd::ProbResult &r = s->results[(size_t)p];
    const long long n = r.status == 0 ? r.n_segments : 0;
    rows[(size_t)3 * p] = total;
    rows[(size_t)3 * p + 1] = n;
    rows[(size_t)3 * p + 2] = s->prob_seg_off[(size_t)p];
    if (rows_out) rows_out[p] = n;
    total += n;
  }
  if (total > t.capacity || !t.d_rows) {
    for (int k = 0; k < 3; k++) dev_free(s, t.col[k], (unsigned long long)t.capacity * col_bytes[k]);
    t.capacity = 0;
    const size_t entries = total > 0 ? (size_t)total : 1;
    for (int k = 0; k < 3; k++)
      if (col_bytes[k] && dev_alloc(s, (char **)&t.col[k], entries * col_bytes[k])) return -1;
    t.capacity = (long long)entries;
    if (!t.d_rows && dev_alloc(s, &t.d_rows, rows.size())) return -1;
  }
  if (hipMemcpy(t.d_rows, rows.data(), rows.size() * sizeof(long long), hipMemcpyHostToDevice) !=
      hipSuccess)
    return -1;
  launch();
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess) {
    set_error("packing the %s failed", what);
    return -1;
  }
  return total;
}

int pack_download(const PackedTable &t, const size_t (&col_bytes)[3], long long total,
                  void *const (&out)[3], const char *what) {
  if (total < 0) return -1;
  for (int k = 0; k < 3 && total > 0; k++)
    if (col_bytes[k] && hipMemcpy(out[k], t.col[k], (size_t)total * col_bytes[k],
                                  hipMemcpyDeviceToHost) != hipSuccess) {
      set_error("download of the packed %s failed", what);
      return -1;
    }
  return 0;
}

constexpr size_t PACK_COLS[3] = {sizeof(int), sizeof(double), 0};           /* start, mean */
constexpr size_t SEGS_COLS[3] = {sizeof(int), sizeof(int), sizeof(double)}; /* start, end, mean */

}  // namespace

extern "C" long long peakseg_hip_problem_set_pack_tables(psd_problem_set *s, long long *rows_out,
                                                         const int **start_dev,
                                                         const double **mean_dev) {
  if (!s || !s->solved) return -1;
  if (hipSetDevice(s->device) != hipSuccess) return -1;
  std::vector<long long> rows((size_t)3 * (size_t)s->n_problems);
  PackedTable &t = s->pack;
  const long long total = pack(s, t, PACK_COLS, rows, rows_out, "segment tables", [&]() {
    hipLaunchKernelGGL(pack_tables_kernel, dim3((unsigned)s->n_problems), dim3(256), 0, s->stream,
                       (const int *)s->d.seg_start, (const double *)s->d.seg_mean,
                       (const long long *)t.d_rows, (int *)t.col[0], (double *)t.col[1]);
  });
  if (total < 0) return -1;
  s->run.pack_total = total;
  if (start_dev) *start_dev = (const int *)t.col[0];
  if (mean_dev) *mean_dev = (const double *)t.col[1];
  return total;
}

extern "C" int peakseg_hip_problem_set_packed_download(psd_problem_set *s, int *start_out,
                                                       double *mean_out) {
  if (!s) return -1;
  return pack_download(s->pack, PACK_COLS, s->run.pack_total, {start_out, mean_out, nullptr},
                       "segment tables");
}

extern "C" long long peakseg_hip_problem_set_pack_segments(psd_problem_set *s,
                                                           const int *first_chromStart,
                                                           long long *rows_out,
                                                           const int **chromStart_dev,
                                                           const int **chromEnd_dev,
                                                           const double **mean_dev) {
  if (!s || !s->solved) return -1;
  if (!s->dense) {
    set_error("pack_segments: the set was not made from dense counts and has no run_end[]");
    return -1;
  }
  if (hipSetDevice(s->device) != hipSuccess) return -1;
  std::vector<long long> rows((size_t)6 * (size_t)s->n_problems);
  long long *lay = rows.data() + (size_t)3 * (size_t)s->n_problems;
  for (int p = 0; p < s->n_problems; p++) {
    const int c = s->prob_contig[(size_t)p];
    const long long first = first_chromStart ? first_chromStart[c] : 0;
    if (first < 0 || first + s->contig_bases[(size_t)c] > 2147483647ll) {
      set_error("pack_segments: contig %d: chromStart %lld + %lld bases is no 32-bit coordinate", c,
                first, s->contig_bases[(size_t)c]);
      return -1;
    }
    lay[(size_t)3 * p] = s->contig_off[(size_t)c];
    lay[(size_t)3 * p + 1] = first;
    lay[(size_t)3 * p + 2] = s->contig_bases[(size_t)c];
  }
  PackedTable &t = s->segs;
  const long long total = pack(s, t, SEGS_COLS, rows, rows_out, "segments", [&]() {
    hipLaunchKernelGGL(psd::dense::pack_segments_kernel, dim3((unsigned)s->n_problems), dim3(256), 0,
                       s->stream, (const int *)s->d.seg_start, (const double *)s->d.seg_mean,
                       (const long long *)t.d_rows,
                       (const long long *)(t.d_rows + (size_t)3 * (size_t)s->n_problems),
                       (const int *)s->d_run_end, (int *)t.col[0], (int *)t.col[1], (double *)t.col[2]);
  });
  if (total < 0) return -1;
  s->run.segs_total = total;
  if (chromStart_dev) *chromStart_dev = (const int *)t.col[0];
  if (chromEnd_dev) *chromEnd_dev = (const int *)t.col[1];
  if (mean_dev) *mean_dev = (const double *)t.col[2];
  return total;
}

extern "C" int peakseg_hip_problem_set_packed_segments_download(psd_problem_set *s,
                                                                int *chromStart_out,
                                                                int *chromEnd_out,
                                                                double *mean_out) {
  if (!s) return -1;
  return pack_download(s->segs, SEGS_COLS, s->run.segs_total, {chromStart_out, chromEnd_out, mean_out},
                       "segments");
}
