/* peakseg_pack.h -- segment tables packed in HBM at their exact sizes (the multi-GPU gather's
 * payload) and their downloads: (start, mean) of any set, and the reference's segments table of
 * a set made from dense counts (its kernel is in dense_encode.h), and the reads, maximum and
 * summit of every row of that table (kernels: segment_stats.h). */

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
  s->run.pack_total = -1; /* (nothing is packed after a call that fails) */
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
  s->run.segs_total = -1; /* (nothing is packed after a call that fails) */
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

/* ---- reads, maximum and summit of every row (kernels: segment_stats.h) ---------------------- */

namespace {

thread_local float g_stats_ms = 0.f;

/* the columns at `total` rows at least, the grid's geometry (first call), the descriptors, the two
 * launches between two events.  0 or a status; the device is set. */
int stats_run(psd_problem_set *s, const int *first_chromStart, long long *rows_out, long long *total_out) {
  namespace sg = psd::stats;
  StatsTable &t = s->stats;
  const size_t np = (size_t)s->n_problems;
  if (t.tile0.empty()) { /* tiles over each problem's contig, laid over its 16-byte aligned range */
    std::vector<long long> tile0(np + 1, 0);
    for (size_t p = 0; p < np; p++) {
      const int c = s->prob_contig[p];
      const long long lead = s->contig_off[(size_t)c] & 3;
      tile0[p + 1] = tile0[p] + (lead + s->contig_n[(size_t)c] + sg::TILE - 1) / sg::TILE;
    }
    /* (a grid dimension times the workgroup size stays below 2^32) */
    if (tile0[np] >= (1ll << 24)) {
      set_error("pack_segment_stats: %lld tiles of %d runs in one call, 2^24 or more", tile0[np], sg::TILE);
      return ERROR_DENSE_ARGUMENTS;
    }
    std::vector<int> tile_problem((size_t)tile0[np]);
    for (size_t p = 0; p < np; p++)
      std::fill(tile_problem.begin() + tile0[p], tile_problem.begin() + tile0[p + 1], (int)p);
    int st = 0;
    if ((st = dev_alloc(s, &t.d_tile_problem, tile_problem.size())) ||
        (st = dev_alloc(s, &t.d_desc, np * sg::DESC)))
      return st;
    HIP_TRY(hipMemcpy(t.d_tile_problem, tile_problem.data(), tile_problem.size() * sizeof(int),
                      hipMemcpyHostToDevice));
    for (auto &e : t.ev) HIP_TRY(hipEventCreate(&e));
    t.n_tiles = tile0[np];
    t.tile0.swap(tile0);
  }
  std::vector<long long> desc(np * sg::DESC, 0);
  long long total = 0;
  for (size_t p = 0; p < np; p++) {
    const psd::ProbResult &r = s->results[p];
    const int c = s->prob_contig[p];
    const long long n = r.status == 0 ? r.n_segments : 0;
    long long *d = desc.data() + p * sg::DESC;
    d[sg::D_TO] = total;
    d[sg::D_ROWS] = n;
    d[sg::D_FROM] = s->prob_seg_off[p];
    d[sg::D_RUN0] = s->contig_off[(size_t)c];
    d[sg::D_RUNS] = s->contig_n[(size_t)c];
    d[sg::D_FIRST] = first_chromStart ? first_chromStart[c] : 0;
    d[sg::D_TILE0] = t.tile0[p];
    if (rows_out) rows_out[p] = n;
    total += n;
  }
  if (total > t.capacity || !t.sum) {
    const unsigned long long cap = (unsigned long long)t.capacity;
    dev_free(s, t.sum, cap * 8);
    dev_free(s, t.key, cap * 8);
    dev_free(s, t.mx, cap * 4);
    dev_free(s, t.summit_start, cap * 4);
    dev_free(s, t.summit_end, cap * 4);
    t.capacity = 0;
    const size_t entries = total > 0 ? (size_t)total : 1;
    int st = 0;
    if ((st = dev_alloc(s, &t.sum, entries)) || (st = dev_alloc(s, &t.key, entries)) ||
        (st = dev_alloc(s, &t.mx, entries)) || (st = dev_alloc(s, &t.summit_start, entries)) ||
        (st = dev_alloc(s, &t.summit_end, entries)))
      return st;
    t.capacity = (long long)entries;
  }
  HIP_TRY(hipMemcpy(t.d_desc, desc.data(), desc.size() * sizeof(long long), hipMemcpyHostToDevice));
  HIP_TRY(hipEventRecord(t.ev[0], s->stream));
  if (total > 0) {
    HIP_TRY(hipMemsetAsync(t.sum, 0, (size_t)total * 8, s->stream));
    HIP_TRY(hipMemsetAsync(t.key, 0, (size_t)total * 8, s->stream));
    hipLaunchKernelGGL(sg::tile_kernel, dim3((unsigned)t.n_tiles), dim3(sg::THREADS), 0, s->stream,
                       (const long long *)t.d_desc, (const int *)t.d_tile_problem,
                       (const int *)s->d.seg_start, (const int *)s->d.count, (const int *)s->d.weight,
                       t.sum, t.key);
    HIP_TRY(hipGetLastError());
    if ((total + sg::THREADS - 1) / sg::THREADS >= (1ll << 24)) {
      set_error("pack_segment_stats: %lld rows in one call", total);
      return ERROR_DENSE_ARGUMENTS;
    }
    hipLaunchKernelGGL(sg::finish_kernel, dim3((unsigned)((total + sg::THREADS - 1) / sg::THREADS)),
                       dim3(sg::THREADS), 0, s->stream, (const long long *)t.d_desc, s->n_problems,
                       total, (const unsigned long long *)t.key, (const int *)s->d.weight,
                       (const int *)s->d_run_end, t.mx, t.summit_start, t.summit_end);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(t.ev[1], s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipEventElapsedTime(&g_stats_ms, t.ev[0], t.ev[1]));
  *total_out = total;
  return 0;
}

}  // namespace

extern "C" long long peakseg_hip_problem_set_pack_segment_stats(
    psd_problem_set *s, const int *first_chromStart, long long *rows_out, const long long **sum_dev,
    const int **max_dev, const int **summitStart_dev, const int **summitEnd_dev) {
  if (!s || !s->solved) return -1;
  if (!s->dense) {
    set_error("pack_segment_stats: the set was not made from dense counts and has no run_end[]");
    return -1;
  }
  if (hipSetDevice(s->device) != hipSuccess) return -1;
  s->run.stats_total = -1; /* (nothing is packed after a call that fails) */
  for (int c = 0; c < s->n_contigs; c++) {
    const long long first = first_chromStart ? first_chromStart[c] : 0;
    if (first < 0 || first + s->contig_bases[(size_t)c] > 2147483647ll) {
      set_error("pack_segment_stats: contig %d: chromStart %lld + %lld bases is no 32-bit coordinate",
                c, first, s->contig_bases[(size_t)c]);
      return -1;
    }
  }
  long long total = 0;
  if (stats_run(s, first_chromStart, rows_out, &total)) return -1;
  s->run.stats_total = total;
  if (sum_dev) *sum_dev = s->stats.sum;
  if (max_dev) *max_dev = s->stats.mx;
  if (summitStart_dev) *summitStart_dev = s->stats.summit_start;
  if (summitEnd_dev) *summitEnd_dev = s->stats.summit_end;
  return total;
}

extern "C" int peakseg_hip_problem_set_packed_segment_stats_download(psd_problem_set *s,
                                                                     long long *sum_out, int *max_out,
                                                                     int *summitStart_out,
                                                                     int *summitEnd_out) {
  if (!s || !s->solved || s->run.stats_total < 0) return -1;
  const size_t n = (size_t)s->run.stats_total;
  const StatsTable &t = s->stats;
  const void *from[4] = {t.sum, t.mx, t.summit_start, t.summit_end};
  void *to[4] = {sum_out, max_out, summitStart_out, summitEnd_out};
  const size_t width[4] = {8, 4, 4, 4};
  for (int k = 0; k < 4 && n > 0; k++)
    if (to[k] && hipMemcpy(to[k], from[k], n * width[k], hipMemcpyDeviceToHost) != hipSuccess) {
      set_error("download of the packed segment statistics failed");
      return -1;
    }
  return 0;
}

extern "C" int peakseg_hip_segment_stats_tile_runs(void) { return psd::stats::TILE; }

extern "C" int peakseg_hip_segment_stats_last_ms(float *ms) {
  if (ms) *ms = g_stats_ms;
  return 0;
}
