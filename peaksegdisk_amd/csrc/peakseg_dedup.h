/* peakseg_dedup.h -- the host side of duplicate removal (kernels: reads_dedup.h): the marking of
 * every read with the units of it that survive, and the stable compaction of reads by such a mark.
 * Neither call is tied to a problem set; everything a call allocates on the device is freed before
 * it returns.  Device and input handling are those of the pile-up (peakseg_reads.h). */

namespace {

thread_local float g_dedup_ms[3] = {0.f, 0.f, 0.f};
thread_local int g_dedup_passes = 0;

struct DedupSpan {
  unsigned long long lo, hi;
  int out;
};

/* does an output overlap an input?  (a sweep over the spans in the order of their first bytes) */
bool dedup_overlap(std::vector<DedupSpan> &spans) {
  std::sort(spans.begin(), spans.end(),
            [](const DedupSpan &a, const DedupSpan &b) { return a.lo < b.lo; });
  unsigned long long in_hi = 0, out_hi = 0;
  for (const DedupSpan &s : spans) {
    if (s.lo < (s.out ? in_hi : out_hi)) return true;
    unsigned long long &hi = s.out ? out_hi : in_hi;
    hi = std::max(hi, s.hi);
  }
  return false;
}

void dedup_span(std::vector<DedupSpan> &spans, const void *p, long long n, size_t item, int out) {
  if (p && n > 0)
    spans.push_back({(unsigned long long)p, (unsigned long long)p + (unsigned long long)n * item, out});
}

/* what the host can see of the reads of a call: `ints` are the int32 arrays of a contig (the first
 * `required` of them must be there), in the pile-up's words and statuses */
int dedup_check_arrays(int c, long long n, const int *const *ints, int n_ints, int required,
                       int on_device) {
  for (int j = 0; j < n_ints; j++) {
    if (j < required && !ints[j]) {
      set_error("reads: contig %d: an array of its %lld reads is NULL", c, n);
      return ERROR_READS_ARGUMENTS;
    }
    if (on_device && ((unsigned long long)ints[j] & 3ull)) {
      set_error("reads: contig %d: a device address is not a multiple of 4", c);
      return ERROR_READS_ARGUMENTS;
    }
  }
  return 0;
}

int dedup_check_counts(int n_contigs, const long long *n_reads, long long *total) {
  if (n_contigs <= 0) {
    set_error("reads: no contig");
    return ERROR_NO_DATA;
  }
  if (!n_reads) {
    set_error("reads: the read counts are NULL");
    return ERROR_READS_ARGUMENTS;
  }
  *total = 0;
  for (int c = 0; c < n_contigs; c++) {
    if (n_reads[c] < 0) {
      set_error("reads: contig %d has %lld reads", c, n_reads[c]);
      return ERROR_READS_ARGUMENTS;
    }
    *total += n_reads[c];
    if (*total >= (1ll << 31)) {
      set_error("dedup: the call has 2^31 or more rows up to contig %d (row numbers are 32 bits)", c);
      return ERROR_DEDUP_ARGUMENTS;
    }
  }
  return 0;
}

/* a contig's host array on the device, in `room` from `off` on; nullptr stays nullptr */
template <class T>
int dedup_upload(const T **array, long long n, T *room, long long &off) {
  if (!*array || n == 0) {
    *array = nullptr;
    return 0;
  }
  HIP_TRY(hipMemcpy(room + off, *array, sizeof(T) * (size_t)n, hipMemcpyHostToDevice));
  *array = room + off;
  off += n;
  return 0;
}

}  // namespace

extern "C" int peakseg_hip_dedup_block_rows(void) { return psd::dedup::BLOCK_ROWS; }
extern "C" int peakseg_hip_dedup_scan_span(void) { return psd::dedup::SCAN_SPAN; }

extern "C" int peakseg_hip_reads_last_dedup_ms(float *keys_ms, float *sort_ms, float *runs_ms) {
  if (keys_ms) *keys_ms = g_dedup_ms[0];
  if (sort_ms) *sort_ms = g_dedup_ms[1];
  if (runs_ms) *runs_ms = g_dedup_ms[2];
  return 0;
}

extern "C" int peakseg_hip_reads_last_dedup_passes(void) { return g_dedup_passes; }

extern "C" int peakseg_hip_reads_dedup(int device, int n_contigs, const long long *n_reads,
                                       const int *const *read_start, const int *const *read_end,
                                       const int *const *read_count,
                                       const signed char *const *read_strand, int reads_on_device,
                                       int by, int keep, int *const *out_count,
                                       long long *summary_out) {
  namespace dd = psd::dedup;
  long long N = 0;
  int st = dedup_check_counts(n_contigs, n_reads, &N);
  if (st) return st;
  const int nc = n_contigs;
  if (by != dd::BY_FRAGMENT && by != dd::BY_FIVE_PRIME) {
    set_error("dedup: by is %d, neither %d (fragment) nor %d (five_prime)", by, dd::BY_FRAGMENT,
              dd::BY_FIVE_PRIME);
    return ERROR_DEDUP_ARGUMENTS;
  }
  if (keep < 1) {
    set_error("dedup: keep is %d, below 1", keep);
    return ERROR_DEDUP_ARGUMENTS;
  }
  if (by == dd::BY_FIVE_PRIME && !read_strand) {
    set_error("dedup: by five_prime needs the strands, which are NULL");
    return ERROR_DEDUP_ARGUMENTS;
  }
  if (!summary_out) {
    set_error("reads: the summary is NULL");
    return ERROR_READS_ARGUMENTS;
  }
  std::vector<DedupSpan> spans;
  for (int c = 0; c < nc; c++) {
    const long long n = n_reads[c];
    if (n == 0) continue;
    const int *ints[4] = {read_start ? read_start[c] : nullptr, read_end ? read_end[c] : nullptr,
                          out_count ? out_count[c] : nullptr, read_count ? read_count[c] : nullptr};
    if ((st = dedup_check_arrays(c, n, ints, 4, 3, reads_on_device))) return st;
    if (read_strand && !read_strand[c]) {
      set_error("strand: contig %d: the strand array is NULL", c);
      return ERROR_STRAND_ARGUMENTS;
    }
    dedup_span(spans, ints[0], n, 4, 0);
    dedup_span(spans, ints[1], n, 4, 0);
    dedup_span(spans, ints[3], n, 4, 0);
    dedup_span(spans, read_strand ? read_strand[c] : nullptr, n, 1, 0);
    dedup_span(spans, ints[2], n, 4, 1);
  }
  if (dedup_overlap(spans)) {
    set_error("dedup: an out_count array overlaps an input array");
    return ERROR_DEDUP_ARGUMENTS;
  }
  if ((st = strand_device(device))) return st;
  g_dedup_ms[0] = g_dedup_ms[1] = g_dedup_ms[2] = 0.f;
  g_dedup_passes = 0;
  if (N == 0) {
    std::fill(summary_out, summary_out + (size_t)nc * dd::SUMMARY, 0ll);
    return 0;
  }
  std::vector<dd::Contig> contigs((size_t)nc);
  long long n_slices = 0, row = 0, in_ints = 0, in_bytes = 0;
  int first_contig = -1;
  for (int c = 0; c < nc; c++) {
    dd::Contig &k = contigs[(size_t)c];
    k.n_reads = n_reads[c];
    k.slice_first = n_slices;
    k.row_first = row;
    n_slices += (k.n_reads + dd::SLICE - 1) / dd::SLICE;
    row += k.n_reads;
    if (k.n_reads && first_contig < 0) first_contig = c;
    in_ints += k.n_reads * (read_count && read_count[c] ? 3 : 2);
    in_bytes += read_strand ? k.n_reads : 0;
  }
  const long long n_blocks = (N + dd::BLOCK_ROWS - 1) / dd::BLOCK_ROWS;
  const long long n_runs = (N + dd::RUN_ROWS - 1) / dd::RUN_ROWS;
  const unsigned long long U = (unsigned long long)N;
  /* the largest the call can need: every key word moves */
  if ((st = strand_fits("reads_dedup",
                        4ull * U * (2ull * (dd::KEY_WORDS + 1) + 1ull) +
                            4ull * dd::DIGITS * (unsigned long long)(n_blocks + dd::MAX_PASSES) +
                            12ull * (unsigned long long)n_runs +
                            (reads_on_device ? 0ull : 4ull * (unsigned long long)in_ints +
                                                          (unsigned long long)in_bytes + 4ull * U) +
                            (unsigned long long)nc * (sizeof(dd::Contig) + sizeof(dd::Check) +
                                                      8ull * dd::SUMMARY_STRIDE * dd::SUMMARY_COPIES) +
                            4ull * (unsigned long long)n_slices + 256ull)))
    return st;
  /* few contigs: their summaries in many copies; many contigs spread the adds by themselves */
  const int copies = nc >= dd::SUMMARY_COPIES ? 1 : dd::SUMMARY_COPIES;
  const size_t summary_words = (size_t)copies * (size_t)nc * dd::SUMMARY_STRIDE;
  DenseScratch scratch;
  unsigned *d_a = nullptr, *d_b = nullptr, *d_table = nullptr, *d_trail = nullptr, *d_carry = nullptr;
  int *d_cnt = nullptr, *d_totals = nullptr, *d_head = nullptr, *d_in = nullptr, *d_out = nullptr,
      *d_slice_contig = nullptr;
  signed char *d_strand = nullptr;
  long long *d_summary = nullptr;
  dd::Contig *d_contigs = nullptr;
  /* the records and, in a 128-byte line of its own behind them (the looks at the mask would queue
   * behind the adds to a record in its line), the four words of the mask: one read-back */
  const size_t check_records = (size_t)nc + 16;
  dd::Check *d_checks = nullptr;
  if ((st = scratch.get(&d_a, (size_t)((dd::KEY_WORDS + 1) * N))) || (st = scratch.get(&d_cnt, (size_t)N)) ||
      (st = scratch.get(&d_totals, (size_t)(dd::MAX_PASSES * dd::DIGITS))) ||
      (st = scratch.get(&d_trail, (size_t)n_runs)) || (st = scratch.get(&d_head, (size_t)n_runs)) ||
      (st = scratch.get(&d_carry, (size_t)n_runs)) ||
      (!reads_on_device && ((st = scratch.get(&d_in, (size_t)in_ints)) ||
                            (st = scratch.get(&d_strand, (size_t)in_bytes)) ||
                            (st = scratch.get(&d_out, (size_t)N)))) ||
      (st = scratch.get(&d_summary, summary_words)) ||
      (st = scratch.get(&d_contigs, (size_t)nc)) || (st = scratch.get(&d_checks, check_records)) ||
      (st = scratch.get(&d_slice_contig, (size_t)n_slices)))
    return st;
  unsigned *d_mask = (unsigned *)(d_checks + nc + 8);
  long long int_off = 0, byte_off = 0;
  for (int c = 0; c < nc; c++) {
    dd::Contig &k = contigs[(size_t)c];
    k.start = k.n_reads ? read_start[c] : nullptr;
    k.end = k.n_reads ? read_end[c] : nullptr;
    k.count = k.n_reads && read_count ? read_count[c] : nullptr;
    k.strand = k.n_reads && read_strand ? read_strand[c] : nullptr;
    k.out = k.n_reads ? out_count[c] : nullptr;
    if (reads_on_device) continue;
    if ((st = dedup_upload(&k.start, k.n_reads, d_in, int_off)) ||
        (st = dedup_upload(&k.end, k.n_reads, d_in, int_off)) ||
        (st = dedup_upload(&k.count, k.n_reads, d_in, int_off)) ||
        (st = dedup_upload(&k.strand, k.n_reads, d_strand, byte_off)))
      return st;
    k.out = d_out + k.row_first;
  }
  std::vector<int> slice_contig((size_t)n_slices);
  for (int c = 0; c < nc; c++)
    std::fill(slice_contig.begin() + contigs[(size_t)c].slice_first,
              slice_contig.begin() + (c + 1 == nc ? n_slices : contigs[(size_t)c + 1].slice_first), c);
  HIP_TRY(hipMemcpy(d_contigs, contigs.data(), sizeof(dd::Contig) * (size_t)nc, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_slice_contig, slice_contig.data(), sizeof(int) * (size_t)n_slices,
                    hipMemcpyHostToDevice));
  for (int k = 0; k < 4; k++) HIP_TRY(hipEventCreate(&scratch.ev[k]));
  hipStream_t stream = (hipStream_t) nullptr;
  dd::Rows side[2];
  for (int w = 0; w < dd::KEY_WORDS; w++) side[0].key[w] = d_a + (long long)w * N;
  side[0].row = d_a + (long long)dd::KEY_WORDS * N;
  HIP_TRY(hipEventRecord(scratch.ev[0], stream));
  HIP_TRY(hipMemsetAsync(d_checks, 0, sizeof(dd::Check) * check_records, stream));
  HIP_TRY(hipMemsetAsync(d_totals, 0, sizeof(int) * (size_t)(dd::MAX_PASSES * dd::DIGITS), stream));
  HIP_TRY(hipMemsetAsync(d_summary, 0, sizeof(long long) * summary_words, stream));
  hipLaunchKernelGGL(dd::keys_kernel, dim3((unsigned)n_slices), dim3(dd::THREADS), 0, stream,
                     (const dd::Contig *)d_contigs, (const int *)d_slice_contig, by, first_contig, side[0],
                     d_cnt, d_checks, d_mask);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(scratch.ev[1], stream));
  std::vector<dd::Check> checks(check_records);
  HIP_TRY(hipMemcpy(checks.data(), d_checks, sizeof(dd::Check) * check_records, hipMemcpyDeviceToHost));
  for (int c = 0; c < nc; c++)
    if (checks[(size_t)c].bad)
      return strand_refuse(c, checks[(size_t)c].bad, reads_on_device, read_start[c], read_end[c],
                           read_count ? read_count[c] : nullptr, read_strand ? read_strand[c] : nullptr);
  for (int c = 0; c < nc; c++)
    if (checks[(size_t)c].sum >= (1ll << 31)) {
      set_error("reads: contig %d: the reads' counts sum to %lld, 2^31 or more", c, checks[(size_t)c].sum);
      return ERROR_READS_ARGUMENTS;
    }
  unsigned mask[dd::KEY_WORDS];
  memcpy(mask, &checks[(size_t)nc + 8], sizeof mask);
  int move = 0, n_moving = 0, passes = 0;
  for (int w = 0; w < dd::KEY_WORDS; w++)
    if (mask[w]) {
      move |= 1 << w;
      n_moving++;
      for (int b = 0; b < 4; b++) passes += ((mask[w] >> (8 * b)) & 0xffu) != 0u;
    }
  g_dedup_passes = passes;
  int at = 0; /* the side that holds the moving words and the row numbers */
  if (passes) {
    if ((st = scratch.get(&d_b, (size_t)((n_moving + 1) * N))) ||
        (st = scratch.get(&d_table, (size_t)(dd::DIGITS * n_blocks))))
      return st;
    /* the words that never differ stay where keys_kernel wrote them, for both sides */
    long long slot = 0;
    for (int w = 0; w < dd::KEY_WORDS; w++)
      side[1].key[w] = (move >> w) & 1 ? d_b + (slot++) * N : side[0].key[w];
    side[1].row = d_b + slot * N;
    int pass = 0;
    for (int digit = 0; digit < dd::MAX_PASSES; digit++) {
      const int w = digit / 4, shift = 8 * (digit % 4);
      if (((mask[w] >> shift) & 0xffu) == 0u) continue;
      const dd::Rows src = side[at], dst = side[1 - at];
      int *totals = d_totals + pass * dd::DIGITS;
      hipLaunchKernelGGL(dd::hist_kernel, dim3((unsigned)n_blocks), dim3(dd::THREADS), 0, stream,
                         (const unsigned *)src.key[w], shift, N, (int)n_blocks, d_table, totals);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(dd::scan_kernel, dim3(dd::DIGITS / dd::WAVES), dim3(dd::THREADS), 0, stream, d_table,
                         (const int *)totals, (int)n_blocks);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(dd::scatter_kernel, dim3((unsigned)n_blocks), dim3(dd::THREADS), 0, stream, src,
                         dst, move, (const unsigned *)src.key[w], shift, N, (int)n_blocks,
                         (const unsigned *)d_table);
      HIP_TRY(hipGetLastError());
      at = 1 - at;
      pass++;
    }
  }
  HIP_TRY(hipEventRecord(scratch.ev[2], stream));
  const dd::Rows sorted = side[at];
  hipLaunchKernelGGL(dd::runs_kernel, dim3((unsigned)n_runs), dim3(dd::THREADS), 0, stream, sorted,
                     (const int *)d_cnt, N, d_trail, d_head);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(dd::carry_kernel, dim3(1), dim3(dd::THREADS), 0, stream, (const unsigned *)d_trail,
                     (const int *)d_head, n_runs, d_carry);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(dd::apply_kernel, dim3((unsigned)n_runs), dim3(dd::THREADS), 0, stream, sorted,
                     (const int *)d_cnt, N, (const unsigned *)d_carry, (const dd::Contig *)d_contigs, keep,
                     d_summary, copies, nc);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(scratch.ev[3], stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (int k = 0; k < 3; k++)
    HIP_TRY(hipEventElapsedTime(&g_dedup_ms[k], scratch.ev[k], scratch.ev[k + 1]));
  std::vector<long long> copied(summary_words), summary((size_t)nc * dd::SUMMARY, 0ll);
  HIP_TRY(hipMemcpy(copied.data(), d_summary, sizeof(long long) * summary_words, hipMemcpyDeviceToHost));
  for (size_t k = 0; k < (size_t)copies * (size_t)nc; k++)
    for (int j = 1; j < dd::SUMMARY; j++)
      summary[(k % (size_t)nc) * dd::SUMMARY + j] += copied[k * dd::SUMMARY_STRIDE + j];
  if (!reads_on_device)
    for (int c = 0; c < nc; c++)
      if (n_reads[c])
        HIP_TRY(hipMemcpy(out_count[c], contigs[(size_t)c].out, sizeof(int) * (size_t)n_reads[c],
                          hipMemcpyDeviceToHost));
  for (int c = 0; c < nc; c++) summary[(size_t)c * dd::SUMMARY] = checks[(size_t)c].sum;
  std::copy(summary.begin(), summary.end(), summary_out);
  return 0;
}

extern "C" int peakseg_hip_reads_compact(int device, int n_contigs, const long long *n_reads,
                                         const int *const *read_start, const int *const *read_end,
                                         const signed char *const *read_strand, int reads_on_device,
                                         const int *const *keep_count, int *const *out_start,
                                         int *const *out_end, int *const *out_count,
                                         signed char *const *out_strand, long long *rows_out) {
  namespace dd = psd::dedup;
  long long N = 0;
  int st = dedup_check_counts(n_contigs, n_reads, &N);
  if (st) return st;
  const int nc = n_contigs;
  if (!rows_out) {
    set_error("reads: the rows written are NULL");
    return ERROR_READS_ARGUMENTS;
  }
  std::vector<DedupSpan> spans;
  for (int c = 0; c < nc; c++) {
    const long long n = n_reads[c];
    if (n == 0) continue;
    const int *ints[6] = {read_start ? read_start[c] : nullptr, read_end ? read_end[c] : nullptr,
                          keep_count ? keep_count[c] : nullptr, out_start ? out_start[c] : nullptr,
                          out_end ? out_end[c] : nullptr, out_count ? out_count[c] : nullptr};
    if ((st = dedup_check_arrays(c, n, ints, 6, 6, reads_on_device))) return st;
    if (read_strand && (!read_strand[c] || !out_strand || !out_strand[c])) {
      set_error("strand: contig %d: a strand array is NULL", c);
      return ERROR_STRAND_ARGUMENTS;
    }
    for (int j = 0; j < 6; j++) dedup_span(spans, ints[j], n, 4, j >= 3);
    if (read_strand) {
      dedup_span(spans, read_strand[c], n, 1, 0);
      dedup_span(spans, out_strand[c], n, 1, 1);
    }
  }
  if (dedup_overlap(spans)) {
    set_error("dedup: an output array overlaps an input array");
    return ERROR_DEDUP_ARGUMENTS;
  }
  if ((st = strand_device(device))) return st;
  if (N == 0) {
    std::fill(rows_out, rows_out + nc, 0ll);
    return 0;
  }
  std::vector<dd::CompactContig> contigs((size_t)nc);
  long long n_slices = 0;
  for (int c = 0; c < nc; c++) {
    dd::CompactContig &k = contigs[(size_t)c];
    k.n_reads = n_reads[c];
    k.slice_first = n_slices;
    n_slices += (k.n_reads + dd::SLICE - 1) / dd::SLICE;
  }
  const unsigned long long U = (unsigned long long)N;
  if ((st = strand_fits("reads_compact",
                        (reads_on_device ? 0ull : (read_strand ? 26ull : 24ull) * U) +
                            (unsigned long long)nc * (sizeof(dd::CompactContig) + 8ull) +
                            12ull * (unsigned long long)n_slices)))
    return st;
  DenseScratch scratch;
  int *d_in = nullptr, *d_out = nullptr, *d_slice_contig = nullptr;
  signed char *d_strand = nullptr, *d_out_strand = nullptr;
  unsigned *d_total = nullptr, *d_carry = nullptr;
  long long *d_rows = nullptr;
  dd::CompactContig *d_contigs = nullptr;
  if ((!reads_on_device &&
       ((st = scratch.get(&d_in, (size_t)(3 * N))) || (st = scratch.get(&d_out, (size_t)(3 * N))) ||
        (read_strand && ((st = scratch.get(&d_strand, (size_t)N)) ||
                         (st = scratch.get(&d_out_strand, (size_t)N)))))) ||
      (st = scratch.get(&d_total, (size_t)n_slices)) || (st = scratch.get(&d_carry, (size_t)n_slices)) ||
      (st = scratch.get(&d_rows, (size_t)nc)) || (st = scratch.get(&d_contigs, (size_t)nc)) ||
      (st = scratch.get(&d_slice_contig, (size_t)n_slices)))
    return st;
  long long int_off = 0, byte_off = 0, out_off = 0, out_byte = 0;
  for (int c = 0; c < nc; c++) {
    dd::CompactContig &k = contigs[(size_t)c];
    const bool any = k.n_reads > 0;
    k.start = any ? read_start[c] : nullptr;
    k.end = any ? read_end[c] : nullptr;
    k.keep = any ? keep_count[c] : nullptr;
    k.strand = any && read_strand ? read_strand[c] : nullptr;
    k.out_start = any ? out_start[c] : nullptr;
    k.out_end = any ? out_end[c] : nullptr;
    k.out_count = any ? out_count[c] : nullptr;
    k.out_strand = any && read_strand ? out_strand[c] : nullptr;
    if (reads_on_device || !any) continue;
    if ((st = dedup_upload(&k.start, k.n_reads, d_in, int_off)) ||
        (st = dedup_upload(&k.end, k.n_reads, d_in, int_off)) ||
        (st = dedup_upload(&k.keep, k.n_reads, d_in, int_off)) ||
        (st = dedup_upload(&k.strand, k.n_reads, d_strand, byte_off)))
      return st;
    k.out_start = d_out + out_off;
    k.out_end = d_out + out_off + k.n_reads;
    k.out_count = d_out + out_off + 2 * k.n_reads;
    out_off += 3 * k.n_reads;
    if (read_strand) {
      k.out_strand = d_out_strand + out_byte;
      out_byte += k.n_reads;
    }
  }
  std::vector<int> slice_contig((size_t)n_slices);
  for (int c = 0; c < nc; c++)
    std::fill(slice_contig.begin() + contigs[(size_t)c].slice_first,
              slice_contig.begin() + (c + 1 == nc ? n_slices : contigs[(size_t)c + 1].slice_first), c);
  HIP_TRY(hipMemcpy(d_contigs, contigs.data(), sizeof(dd::CompactContig) * (size_t)nc, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_slice_contig, slice_contig.data(), sizeof(int) * (size_t)n_slices,
                    hipMemcpyHostToDevice));
  hipStream_t stream = (hipStream_t) nullptr;
  (void)stream;
  hipLaunchKernelGGL(dd::flag_kernel, dim3((unsigned)n_slices), dim3(dd::THREADS), 0, stream,
                     (const dd::CompactContig *)d_contigs, (const int *)d_slice_contig, d_total);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(dd::slice_scan_kernel, dim3((unsigned)nc), dim3(dd::THREADS), 0, stream,
                     (const dd::CompactContig *)d_contigs, (const unsigned *)d_total, d_carry, d_rows);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(dd::compact_kernel, dim3((unsigned)n_slices), dim3(dd::THREADS), 0, stream,
                     (const dd::CompactContig *)d_contigs, (const int *)d_slice_contig,
                     (const unsigned *)d_carry);
  HIP_TRY(hipGetLastError());
  std::vector<long long> rows((size_t)nc);
  HIP_TRY(hipMemcpy(rows.data(), d_rows, sizeof(long long) * (size_t)nc, hipMemcpyDeviceToHost));
  if (!reads_on_device)
    for (int c = 0; c < nc; c++) {
      const dd::CompactContig &k = contigs[(size_t)c];
      const size_t n = (size_t)rows[(size_t)c];
      if (n == 0) continue;
      HIP_TRY(hipMemcpy(out_start[c], k.out_start, sizeof(int) * n, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(out_end[c], k.out_end, sizeof(int) * n, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(out_count[c], k.out_count, sizeof(int) * n, hipMemcpyDeviceToHost));
      if (read_strand) HIP_TRY(hipMemcpy(out_strand[c], k.out_strand, n, hipMemcpyDeviceToHost));
    }
  std::copy(rows.begin(), rows.end(), rows_out);
  return 0;
}
