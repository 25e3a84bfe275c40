/* peakseg_strand.h -- the host side of stranded reads (kernels: strand_xcorr.h): the strand
 * cross-correlation table of every contig and the extension of reads to a fragment length.  Neither
 * call is tied to a problem set; everything a call allocates on the device is freed before it
 * returns.  Device and input handling are those of the pile-up (peakseg_reads.h). */

namespace {

thread_local float g_xcorr_ms[2] = {0.f, 0.f};

/* what the host can see of the reads of a stranded call, in the pile-up's words and statuses; a
 * strand array may begin at any byte */
int strand_check_reads(int n_contigs, const long long *n_reads, const int *const *start,
                       const int *const *end, const int *const *count, const signed char *const *strand,
                       const int *const *out_start, const int *const *out_end, int on_device) {
  if (n_contigs <= 0) {
    set_error("reads: no contig");
    return ERROR_NO_DATA;
  }
  if (!n_reads) {
    set_error("reads: the read counts are NULL");
    return ERROR_READS_ARGUMENTS;
  }
  for (int c = 0; c < n_contigs; c++) {
    if (n_reads[c] < 0) {
      set_error("reads: contig %d has %lld reads", c, n_reads[c]);
      return ERROR_READS_ARGUMENTS;
    }
    if (n_reads[c] == 0) continue;
    const int *arrays[5] = {start ? start[c] : nullptr, end ? end[c] : nullptr,
                            count ? count[c] : nullptr, out_start ? out_start[c] : nullptr,
                            out_end ? out_end[c] : nullptr};
    if (!arrays[0] || !arrays[1]) {
      set_error("reads: contig %d: chromStart or chromEnd is NULL", c);
      return ERROR_READS_ARGUMENTS;
    }
    if (on_device)
      for (const int *a : arrays)
        if ((unsigned long long)a & 3ull) {
          set_error("reads: contig %d: a device address is not a multiple of 4", c);
          return ERROR_READS_ARGUMENTS;
        }
    if (!strand || !strand[c]) {
      set_error("strand: contig %d: the strand array is NULL", c);
      return ERROR_STRAND_ARGUMENTS;
    }
  }
  return 0;
}

/* ERROR_DEVICE_MEMORY with its text when `bytes` do not fit, else 0: asked before anything is
 * allocated */
int strand_fits(const char *who, unsigned long long bytes) {
  size_t free_b = 0, total_b = 0;
  const bool known = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
  const unsigned long long cap = env_bytes("PEAKSEG_HIP_MAX_BYTES");
  if ((cap && bytes > cap) || (known && bytes > (unsigned long long)free_b)) {
    set_error("%s: the call needs %llu bytes on the device, which do not fit (free HBM / "
              "PEAKSEG_HIP_MAX_BYTES)", who, bytes);
    return ERROR_DEVICE_MEMORY;
  }
  return 0;
}

/* the status and the text of a contig's first bad read; host arrays give the values */
int strand_refuse(int c, unsigned long long key, int on_device, const int *start, const int *end,
                  const int *count, const signed char *strand) {
  namespace xc = psd::xcorr;
  const int why = (int)(key & ((1ull << xc::REASON_BITS) - 1ull));
  const long long i = (long long)((~(key >> xc::REASON_BITS)) & ((1ull << (64 - xc::REASON_BITS)) - 1ull));
  if (why == xc::BAD_STRAND) {
    if (on_device)
      set_error("strand: contig %d: read %lld has a strand that is neither +1 nor -1", c, i);
    else
      set_error("strand: contig %d: read %lld has the strand %d, neither +1 nor -1", c, i, (int)strand[i]);
    return ERROR_STRAND_ARGUMENTS;
  }
  if (on_device)
    set_error("reads: contig %d: read %lld has chromStart >= chromEnd or a negative count", c, i);
  else if (why == xc::BAD_ORDER)
    set_error("reads: contig %d: read %lld has chromStart %d >= chromEnd %d", c, i, start[i], end[i]);
  else
    set_error("reads: contig %d: read %lld has the negative count %d", c, i, count[i]);
  return ERROR_READS_ARGUMENTS;
}

/* The library's own copy of a contig's host arrays (the int32 ones into `ints`, the strands into
 * `bytes`), or the caller's device arrays as they are.  `arrays` and `strand` are replaced. */
int strand_upload(long long n, int on_device, const int **arrays, int n_arrays, const signed char **strand,
                  int *ints, long long &int_off, signed char *bytes, long long &byte_off) {
  if (n == 0) {
    for (int j = 0; j < n_arrays; j++) arrays[j] = nullptr;
    *strand = nullptr;
    return 0;
  }
  if (on_device) return 0;
  for (int j = 0; j < n_arrays; j++) {
    if (!arrays[j]) continue;
    HIP_TRY(hipMemcpy(ints + int_off, arrays[j], sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    arrays[j] = ints + int_off;
    int_off += n;
  }
  HIP_TRY(hipMemcpy(bytes + byte_off, *strand, (size_t)n, hipMemcpyHostToDevice));
  *strand = bytes + byte_off;
  byte_off += n;
  return 0;
}

int strand_device(int device) {
  if (peakseg_hip_device_count() <= device || device < 0) {
    set_error("no HIP device %d visible (this library has no CPU fallback)", device);
    return ERROR_NO_HIP_DEVICE;
  }
  HIP_TRY(hipSetDevice(device));
  return 0;
}

}  // namespace

extern "C" int peakseg_hip_xcorr_max_shift(void) { return psd::xcorr::MAX_SHIFT; }

extern "C" int peakseg_hip_reads_last_xcorr_ms(float *tags_ms, float *xcorr_ms) {
  if (tags_ms) *tags_ms = g_xcorr_ms[0];
  if (xcorr_ms) *xcorr_ms = g_xcorr_ms[1];
  return 0;
}

extern "C" int peakseg_hip_reads_strand_xcorr(int device, int n_contigs, const long long *n_reads,
                                              const int *const *read_start, const int *const *read_end,
                                              const int *const *read_count,
                                              const signed char *const *read_strand, int reads_on_device,
                                              const int *extent_start, const int *extent_end,
                                              int max_shift, long long *table_out) {
  namespace xc = psd::xcorr;
  int st = strand_check_reads(n_contigs, n_reads, read_start, read_end, read_count, read_strand, nullptr,
                              nullptr, reads_on_device);
  if (st) return st;
  if (max_shift < 0 || max_shift > xc::MAX_SHIFT) {
    set_error("strand: max_shift is %d, outside 0 .. %d", max_shift, xc::MAX_SHIFT);
    return ERROR_STRAND_ARGUMENTS;
  }
  if (!extent_start || !extent_end || !table_out) {
    set_error("reads: the extents or the table are NULL");
    return ERROR_READS_ARGUMENTS;
  }
  const int nc = n_contigs;
  const long long row_words = (long long)(max_shift + 1) * xc::COLS;
  std::vector<xc::Contig> contigs((size_t)nc);
  long long n_slices = 0, n_tiles = 0, slots = 0, read_ints = 0, read_bytes = 0;
  for (int c = 0; c < nc; c++) {
    const long long lo = extent_start[c], hi = extent_end[c];
    if (hi <= lo) {
      set_error("strand: contig %d: the extent [%lld, %lld) is empty", c, lo, hi);
      return ERROR_STRAND_ARGUMENTS;
    }
    if (lo < 0) {
      set_error("reads: contig %d: the extent starts at %lld, below 0", c, lo);
      return ERROR_READS_ARGUMENTS;
    }
    xc::Contig &k = contigs[(size_t)c];
    k.lo = extent_start[c];
    k.hi = extent_end[c];
    k.n_reads = n_reads[c];
    k.padded = (hi - lo + 3) & ~3ll;
    k.slice_first = n_slices;
    k.tile_first = n_tiles;
    n_slices += (k.n_reads + xc::SLICE - 1) / xc::SLICE;
    n_tiles += (k.padded + xc::TILE - 1) / xc::TILE;
    slots += k.padded;
    read_ints += k.n_reads * (read_count && read_count[c] ? 3 : 2);
    read_bytes += k.n_reads;
  }
  /* (a grid dimension times the workgroup size stays below 2^32) */
  if (n_slices >= (1ll << 24) || n_tiles >= (1ll << 24)) {
    set_error("reads: %lld slices of %d reads and %lld tiles of %d bases in one call, 2^24 or more",
              n_slices, xc::SLICE, n_tiles, xc::TILE);
    return ERROR_READS_ARGUMENTS;
  }
  if ((st = strand_device(device))) return st;
  const long long total_words = xc::TOTAL_COPIES * xc::TOTAL_STRIDE;
  const long long table_words = (long long)nc * (row_words + total_words);
  if ((st = strand_fits("strand_xcorr",
                        8ull * (unsigned long long)slots + 8ull * (unsigned long long)table_words +
                            (reads_on_device ? 0ull : 4ull * (unsigned long long)read_ints + (unsigned long long)read_bytes) +
                            (unsigned long long)nc * (sizeof(xc::Contig) + sizeof(xc::Check)) +
                            4ull * (unsigned long long)(n_slices + n_tiles))))
    return st;
  DenseScratch scratch;
  int *d_tags = nullptr, *d_reads = nullptr, *d_slice_contig = nullptr, *d_tile_contig = nullptr;
  signed char *d_strand = nullptr;
  long long *d_table = nullptr;
  xc::Contig *d_contigs = nullptr;
  xc::Check *d_checks = nullptr;
  if ((st = scratch.get(&d_tags, (size_t)(2 * slots))) || (st = scratch.get(&d_table, (size_t)table_words)) ||
      (!reads_on_device && ((st = scratch.get(&d_reads, (size_t)read_ints)) ||
                            (st = scratch.get(&d_strand, (size_t)read_bytes)))) ||
      (st = scratch.get(&d_contigs, (size_t)nc)) || (st = scratch.get(&d_checks, (size_t)nc)) ||
      (st = scratch.get(&d_slice_contig, (size_t)n_slices)) ||
      (st = scratch.get(&d_tile_contig, (size_t)n_tiles)))
    return st;
  long long tag_off = 0, int_off = 0, byte_off = 0;
  for (int c = 0; c < nc; c++) {
    xc::Contig &k = contigs[(size_t)c];
    k.plus = d_tags + tag_off;
    k.minus = d_tags + slots + tag_off;
    tag_off += k.padded;
    k.table = d_table + (long long)c * row_words;
    k.totals = d_table + (long long)nc * row_words + (long long)c * total_words;
    const int *arrays[3] = {read_start ? read_start[c] : nullptr, read_end ? read_end[c] : nullptr,
                            read_count ? read_count[c] : nullptr};
    const signed char *strand = read_strand ? read_strand[c] : nullptr;
    if ((st = strand_upload(k.n_reads, reads_on_device, arrays, 3, &strand, d_reads, int_off, d_strand, byte_off)))
      return st;
    k.start = arrays[0];
    k.end = arrays[1];
    k.count = arrays[2];
    k.strand = strand;
  }
  std::vector<int> slice_contig((size_t)n_slices), tile_contig((size_t)n_tiles);
  for (int c = 0; c < nc; c++) {
    const bool last = c + 1 == nc;
    std::fill(slice_contig.begin() + contigs[(size_t)c].slice_first,
              slice_contig.begin() + (last ? n_slices : contigs[(size_t)c + 1].slice_first), c);
    std::fill(tile_contig.begin() + contigs[(size_t)c].tile_first,
              tile_contig.begin() + (last ? n_tiles : contigs[(size_t)c + 1].tile_first), c);
  }
  HIP_TRY(hipMemcpy(d_contigs, contigs.data(), sizeof(xc::Contig) * (size_t)nc, hipMemcpyHostToDevice));
  if (n_slices)
    HIP_TRY(hipMemcpy(d_slice_contig, slice_contig.data(), sizeof(int) * (size_t)n_slices, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_tile_contig, tile_contig.data(), sizeof(int) * (size_t)n_tiles, hipMemcpyHostToDevice));
  for (int k = 0; k < 3; k++) HIP_TRY(hipEventCreate(&scratch.ev[k]));
  hipStream_t stream = (hipStream_t) nullptr;
  g_xcorr_ms[0] = g_xcorr_ms[1] = 0.f;
  HIP_TRY(hipEventRecord(scratch.ev[0], stream));
  HIP_TRY(hipMemsetAsync(d_tags, 0, sizeof(int) * (size_t)(2 * slots), stream));
  HIP_TRY(hipMemsetAsync(d_table, 0, sizeof(long long) * (size_t)table_words, stream));
  HIP_TRY(hipMemsetAsync(d_checks, 0, sizeof(xc::Check) * (size_t)nc, stream));
  if (n_slices) {
    hipLaunchKernelGGL(xc::tags_kernel, dim3((unsigned)n_slices), dim3(xc::THREADS), 0, stream,
                       (const xc::Contig *)d_contigs, (const int *)d_slice_contig, d_checks);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(scratch.ev[1], stream));
  std::vector<xc::Check> checks((size_t)nc);
  HIP_TRY(hipMemcpy(checks.data(), d_checks, sizeof(xc::Check) * (size_t)nc, hipMemcpyDeviceToHost));
  for (int c = 0; c < nc; c++)
    if (checks[(size_t)c].bad)
      return strand_refuse(c, checks[(size_t)c].bad, reads_on_device, read_start[c], read_end[c],
                           read_count ? read_count[c] : nullptr, read_strand[c]);
  for (int c = 0; c < nc; c++)
    if (checks[(size_t)c].sum >= (1ll << 31)) {
      set_error("reads: contig %d: the reads' counts sum to %lld, 2^31 or more", c, checks[(size_t)c].sum);
      return ERROR_READS_ARGUMENTS;
    }
  hipLaunchKernelGGL(xc::xcorr_kernel, dim3((unsigned)n_tiles), dim3(xc::THREADS), 0, stream,
                     (const xc::Contig *)d_contigs, (const int *)d_tile_contig, max_shift);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(xc::edges_kernel, dim3((unsigned)nc), dim3(xc::THREADS), 0, stream,
                     (const xc::Contig *)d_contigs, max_shift);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(scratch.ev[2], stream));
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipEventElapsedTime(&g_xcorr_ms[0], scratch.ev[0], scratch.ev[1]));
  HIP_TRY(hipEventElapsedTime(&g_xcorr_ms[1], scratch.ev[1], scratch.ev[2]));
  HIP_TRY(hipMemcpy(table_out, d_table, sizeof(long long) * (size_t)((long long)nc * row_words),
                    hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int peakseg_hip_reads_extend(int device, int n_contigs, const long long *n_reads,
                                        const int *const *read_start, const int *const *read_end,
                                        const signed char *const *read_strand, int reads_on_device,
                                        const int *fragment_length, int *const *out_start,
                                        int *const *out_end) {
  namespace xc = psd::xcorr;
  int st = strand_check_reads(n_contigs, n_reads, read_start, read_end, nullptr, read_strand,
                              (const int *const *)out_start, (const int *const *)out_end, reads_on_device);
  if (st) return st;
  const int nc = n_contigs;
  if (!fragment_length) {
    set_error("strand: the fragment lengths are NULL");
    return ERROR_STRAND_ARGUMENTS;
  }
  std::vector<xc::ExtendContig> contigs((size_t)nc);
  long long n_slices = 0, n_all = 0;
  for (int c = 0; c < nc; c++) {
    if (fragment_length[c] < 1) {
      set_error("strand: contig %d: fragment_length is %d, below 1", c, fragment_length[c]);
      return ERROR_STRAND_ARGUMENTS;
    }
    if (n_reads[c] > 0 && (!out_start || !out_end || !out_start[c] || !out_end[c])) {
      set_error("reads: contig %d: an output array is NULL", c);
      return ERROR_READS_ARGUMENTS;
    }
    xc::ExtendContig &k = contigs[(size_t)c];
    k.n_reads = n_reads[c];
    k.slice_first = n_slices;
    k.length = fragment_length[c];
    k.pad = 0;
    n_slices += (k.n_reads + xc::SLICE - 1) / xc::SLICE;
    n_all += k.n_reads;
  }
  if (n_slices >= (1ll << 24)) {
    set_error("reads: %lld slices of %d reads in one call, 2^24 or more", n_slices, xc::SLICE);
    return ERROR_READS_ARGUMENTS;
  }
  if ((st = strand_device(device))) return st;
  if ((st = strand_fits("reads_extend",
                        (reads_on_device ? 0ull : 17ull * (unsigned long long)n_all) +
                            (unsigned long long)nc * (sizeof(xc::ExtendContig) + sizeof(xc::Check)) +
                            4ull * (unsigned long long)n_slices)))
    return st;
  DenseScratch scratch;
  int *d_reads = nullptr, *d_out = nullptr, *d_slice_contig = nullptr;
  signed char *d_strand = nullptr;
  xc::ExtendContig *d_contigs = nullptr;
  xc::Check *d_checks = nullptr;
  if ((!reads_on_device && ((st = scratch.get(&d_reads, (size_t)(2 * n_all))) ||
                            (st = scratch.get(&d_out, (size_t)(2 * n_all))) ||
                            (st = scratch.get(&d_strand, (size_t)n_all)))) ||
      (st = scratch.get(&d_contigs, (size_t)nc)) || (st = scratch.get(&d_checks, (size_t)nc)) ||
      (st = scratch.get(&d_slice_contig, (size_t)n_slices)))
    return st;
  long long int_off = 0, byte_off = 0, out_off = 0;
  for (int c = 0; c < nc; c++) {
    xc::ExtendContig &k = contigs[(size_t)c];
    const int *arrays[2] = {read_start ? read_start[c] : nullptr, read_end ? read_end[c] : nullptr};
    const signed char *strand = read_strand ? read_strand[c] : nullptr;
    if ((st = strand_upload(k.n_reads, reads_on_device, arrays, 2, &strand, d_reads, int_off, d_strand, byte_off)))
      return st;
    k.start = arrays[0];
    k.end = arrays[1];
    k.strand = strand;
    k.out_start = k.n_reads == 0 ? nullptr : (reads_on_device ? out_start[c] : d_out + out_off);
    k.out_end = k.n_reads == 0 ? nullptr : (reads_on_device ? out_end[c] : d_out + out_off + k.n_reads);
    out_off += 2 * k.n_reads;
  }
  std::vector<int> slice_contig((size_t)n_slices);
  for (int c = 0; c < nc; c++)
    std::fill(slice_contig.begin() + contigs[(size_t)c].slice_first,
              slice_contig.begin() + (c + 1 == nc ? n_slices : contigs[(size_t)c + 1].slice_first), c);
  HIP_TRY(hipMemcpy(d_contigs, contigs.data(), sizeof(xc::ExtendContig) * (size_t)nc, hipMemcpyHostToDevice));
  if (n_slices)
    HIP_TRY(hipMemcpy(d_slice_contig, slice_contig.data(), sizeof(int) * (size_t)n_slices, hipMemcpyHostToDevice));
  hipStream_t stream = (hipStream_t) nullptr;
  HIP_TRY(hipMemsetAsync(d_checks, 0, sizeof(xc::Check) * (size_t)nc, stream));
  if (n_slices) {
    hipLaunchKernelGGL(xc::extend_kernel, dim3((unsigned)n_slices), dim3(xc::THREADS), 0, stream,
                       (const xc::ExtendContig *)d_contigs, (const int *)d_slice_contig, d_checks);
    HIP_TRY(hipGetLastError());
  }
  std::vector<xc::Check> checks((size_t)nc);
  HIP_TRY(hipMemcpy(checks.data(), d_checks, sizeof(xc::Check) * (size_t)nc, hipMemcpyDeviceToHost));
  for (int c = 0; c < nc; c++)
    if (checks[(size_t)c].bad)
      return strand_refuse(c, checks[(size_t)c].bad, reads_on_device, read_start[c], read_end[c], nullptr,
                           read_strand[c]);
  if (!reads_on_device)
    for (int c = 0; c < nc; c++) {
      const xc::ExtendContig &k = contigs[(size_t)c];
      if (k.n_reads == 0) continue;
      HIP_TRY(hipMemcpy(out_start[c], k.out_start, sizeof(int) * (size_t)k.n_reads, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(out_end[c], k.out_end, sizeof(int) * (size_t)k.n_reads, hipMemcpyDeviceToHost));
    }
  return 0;
}
