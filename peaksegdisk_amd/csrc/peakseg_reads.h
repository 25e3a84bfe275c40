/* peakseg_reads.h -- the host side of coverage from aligned reads: the pile-up on the device
 * (kernels: reads_pileup.h) into a buffer the dense encoder reads in place, the creator from reads,
 * the probe of the pile-up alone.  From the encoder on a set made from reads is a dense set
 * (peakseg_dense.h). */

namespace {

struct ReadsInput { /* the read arguments of the C ABI, as they came */
  int n_contigs;
  const long long *n_reads;
  const int *const *start, *const *end, *const *count;
  int on_device;
  const int *lo, *hi;
  int bases_counted;
};

/* what the host can see of a call from reads (after the penalties, before the device) */
int reads_check_arguments(const ReadsInput &r) {
  if (r.n_contigs <= 0) {
    set_error("reads: no contig");
    return ERROR_NO_DATA;
  }
  if (!r.n_reads || !r.lo || !r.hi) {
    set_error("reads: the read counts or the extents are NULL");
    return ERROR_READS_ARGUMENTS;
  }
  if (r.bases_counted != 0 && r.bases_counted != 1) {
    set_error("reads: bases_counted is %d, neither 0 (each base of a read) nor 1 (its last base)",
              r.bases_counted);
    return ERROR_READS_ARGUMENTS;
  }
  for (int c = 0; c < r.n_contigs; c++) {
    const long long lo = r.lo[c], hi = r.hi[c];
    if (hi <= lo) {
      set_error("reads: contig %d: the extent [%lld, %lld) is empty", c, lo, hi);
      return ERROR_READS_ARGUMENTS;
    }
    if (lo < 0) {
      set_error("reads: contig %d: the extent starts at %lld, below 0", c, lo);
      return ERROR_READS_ARGUMENTS;
    }
    if (hi - lo >= (1ll << 31)) {
      set_error("reads: contig %d: the extent has %lld bases, 2^31 or more", c, hi - lo);
      return ERROR_READS_ARGUMENTS;
    }
    if (r.n_reads[c] < 0) {
      set_error("reads: contig %d has %lld reads", c, r.n_reads[c]);
      return ERROR_READS_ARGUMENTS;
    }
    const int *arrays[3] = {r.start ? r.start[c] : nullptr, r.end ? r.end[c] : nullptr,
                            r.count ? r.count[c] : nullptr};
    if (r.n_reads[c] > 0 && (!arrays[0] || !arrays[1])) {
      set_error("reads: contig %d: chromStart or chromEnd is NULL", c);
      return ERROR_READS_ARGUMENTS;
    }
    if (r.on_device)
      for (const int *a : arrays)
        if ((unsigned long long)a & 3ull) {
          set_error("reads: contig %d: a device address is not a multiple of 4", c);
          return ERROR_READS_ARGUMENTS;
        }
  }
  return 0;
}

struct ReadsPiled {
  DenseScratch scratch; /* the coverage buffer among it: freed with this object */
  std::vector<long long> n_bases;
  std::vector<const int *> coverage; /* per contig, device: what dense_encode takes */
  float ms[2] = {0.f, 0.f};          /* zeroing and scatter; the three scan launches */
  double upload_s = 0.0;
};

/* The pile-up alone.  The arguments are checked, the device is set. */
int reads_pileup(const ReadsInput &r, ReadsPiled &out) {
  namespace rd = psd::reads;
  DenseScratch &scratch = out.scratch;
  const auto t_upload = std::chrono::steady_clock::now();
  const int nc = r.n_contigs;
  std::vector<rd::Contig> contigs((size_t)nc);
  long long n_slices = 0, n_tiles = 0, slots = 0, read_ints = 0;
  for (int c = 0; c < nc; c++) {
    rd::Contig &k = contigs[(size_t)c];
    k.lo = r.lo[c];
    k.hi = r.hi[c];
    k.n_reads = r.n_reads[c];
    k.padded = ((long long)k.hi - k.lo + 3) & ~3ll;
    k.slice_first = n_slices;
    k.tile_first = n_tiles;
    n_slices += (k.n_reads + rd::SLICE - 1) / rd::SLICE;
    n_tiles += (k.padded + rd::TILE - 1) / rd::TILE;
    slots += k.padded;
    const bool counted = r.count && r.count[c];
    read_ints += k.n_reads * (counted ? 3 : 2);
    out.n_bases.push_back((long long)k.hi - k.lo);
  }
  /* (a grid dimension times the workgroup size stays below 2^32) */
  if (n_slices >= (1ll << 24) || n_tiles >= (1ll << 24)) {
    set_error("reads: %lld slices of %d reads and %lld tiles of %d bases in one call, 2^24 or more",
              n_slices, rd::SLICE, n_tiles, rd::TILE);
    return ERROR_READS_ARGUMENTS;
  }
  int *d_cov = nullptr, *d_reads = nullptr;
  int st = scratch.get(&d_cov, (size_t)slots);
  if (st) return st;
  if (!r.on_device && (st = scratch.get(&d_reads, (size_t)read_ints))) return st;
  long long cov_off = 0, read_off = 0;
  for (int c = 0; c < nc; c++) {
    rd::Contig &k = contigs[(size_t)c];
    k.cov = d_cov + cov_off;
    cov_off += k.padded;
    out.coverage.push_back(k.cov);
    const int *arrays[3] = {r.start ? r.start[c] : nullptr, r.end ? r.end[c] : nullptr,
                            r.count ? r.count[c] : nullptr};
    if (k.n_reads == 0) arrays[0] = arrays[1] = arrays[2] = nullptr;
    if (!r.on_device)
      for (auto &a : arrays) { /* the library's own copy, one array after the other */
        if (!a) continue;
        HIP_TRY(hipMemcpy(d_reads + read_off, a, sizeof(int) * (size_t)k.n_reads, hipMemcpyHostToDevice));
        a = d_reads + read_off;
        read_off += k.n_reads;
      }
    k.start = arrays[0];
    k.end = arrays[1];
    k.count = arrays[2];
  }
  std::vector<int> slice_contig((size_t)n_slices), tile_contig((size_t)n_tiles);
  for (int c = 0; c < nc; c++) {
    const bool last = c + 1 == nc;
    std::fill(slice_contig.begin() + contigs[(size_t)c].slice_first,
              slice_contig.begin() + (last ? n_slices : contigs[(size_t)c + 1].slice_first), c);
    std::fill(tile_contig.begin() + contigs[(size_t)c].tile_first,
              tile_contig.begin() + (last ? n_tiles : contigs[(size_t)c + 1].tile_first), c);
  }
  rd::Contig *d_contigs = nullptr;
  rd::Check *d_checks = nullptr;
  int *d_slice_contig = nullptr, *d_tile_contig = nullptr, *d_tile_sum = nullptr, *d_tile_carry = nullptr;
  if ((st = scratch.get(&d_contigs, (size_t)nc)) || (st = scratch.get(&d_checks, (size_t)nc)) ||
      (st = scratch.get(&d_slice_contig, (size_t)n_slices)) ||
      (st = scratch.get(&d_tile_contig, (size_t)n_tiles)) ||
      (st = scratch.get(&d_tile_sum, (size_t)n_tiles)) || (st = scratch.get(&d_tile_carry, (size_t)n_tiles)))
    return st;
  HIP_TRY(hipMemcpy(d_contigs, contigs.data(), sizeof(rd::Contig) * (size_t)nc, hipMemcpyHostToDevice));
  if (n_slices)
    HIP_TRY(hipMemcpy(d_slice_contig, slice_contig.data(), sizeof(int) * (size_t)n_slices, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_tile_contig, tile_contig.data(), sizeof(int) * (size_t)n_tiles, hipMemcpyHostToDevice));
  for (int k = 0; k < 3; k++) HIP_TRY(hipEventCreate(&scratch.ev[k]));
  hipStream_t stream = (hipStream_t) nullptr;
  out.upload_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_upload).count();
  HIP_TRY(hipEventRecord(scratch.ev[0], stream));
  HIP_TRY(hipMemsetAsync(d_cov, 0, sizeof(int) * (size_t)slots, stream));
  HIP_TRY(hipMemsetAsync(d_checks, 0, sizeof(rd::Check) * (size_t)nc, stream));
  if (n_slices) {
    hipLaunchKernelGGL(rd::scatter_kernel, dim3((unsigned)n_slices), dim3(rd::THREADS), 0, stream,
                       (const rd::Contig *)d_contigs, (const int *)d_slice_contig, r.bases_counted,
                       d_checks);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(scratch.ev[1], stream));
  std::vector<rd::Check> checks((size_t)nc);
  HIP_TRY(hipMemcpy(checks.data(), d_checks, sizeof(rd::Check) * (size_t)nc, hipMemcpyDeviceToHost));
  for (int c = 0; c < nc; c++) {
    const rd::Check &k = checks[(size_t)c];
    if (k.bad) {
      const long long i = (long long)~k.bad;
      if (r.on_device)
        set_error("reads: contig %d: read %lld has chromStart >= chromEnd or a negative count", c, i);
      else if (r.start[c][i] >= r.end[c][i])
        set_error("reads: contig %d: read %lld has chromStart %d >= chromEnd %d", c, i, r.start[c][i],
                  r.end[c][i]);
      else
        set_error("reads: contig %d: read %lld has the negative count %d", c, i, r.count[c][i]);
      return ERROR_READS_ARGUMENTS;
    }
  }
  for (int c = 0; c < nc; c++)
    if (checks[(size_t)c].sum >= (1ll << 31)) {
      set_error("reads: contig %d: the reads' counts sum to %lld, 2^31 or more", c, checks[(size_t)c].sum);
      return ERROR_READS_ARGUMENTS;
    }
  hipLaunchKernelGGL(rd::tile_sum_kernel, dim3((unsigned)n_tiles), dim3(rd::THREADS), 0, stream,
                     (const rd::Contig *)d_contigs, (const int *)d_tile_contig, d_tile_sum);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(rd::tile_scan_kernel, dim3((unsigned)nc), dim3(rd::THREADS), 0, stream,
                     (const rd::Contig *)d_contigs, (const int *)d_tile_sum, d_tile_carry);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(rd::apply_kernel, dim3((unsigned)n_tiles), dim3(rd::THREADS), 0, stream,
                     (const rd::Contig *)d_contigs, (const int *)d_tile_contig, (const int *)d_tile_carry);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(scratch.ev[2], stream));
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipEventElapsedTime(&out.ms[0], scratch.ev[0], scratch.ev[1]));
  HIP_TRY(hipEventElapsedTime(&out.ms[1], scratch.ev[1], scratch.ev[2]));
  return 0;
}

thread_local float g_reads_ms[2] = {0.f, 0.f};

}  // namespace

extern "C" int peakseg_hip_reads_last_pileup_ms(float *scatter_ms, float *scan_ms) {
  if (scatter_ms) *scatter_ms = g_reads_ms[0];
  if (scan_ms) *scan_ms = g_reads_ms[1];
  return 0;
}

extern "C" int peakseg_hip_reads_pileup_probe(int device, int n_contigs, const long long *n_reads,
                                              const int *const *read_start, const int *const *read_end,
                                              const int *const *read_count, int reads_on_device,
                                              const int *extent_start, const int *extent_end,
                                              int bases_counted, int *coverage_out, long long *runs_out,
                                              int *count_out, int *weight_out, int *run_end_out) {
  const ReadsInput in = {n_contigs, n_reads, read_start, read_end, read_count, reads_on_device,
                         extent_start, extent_end, bases_counted};
  int st = reads_check_arguments(in);
  if (st) return st;
  if (peakseg_hip_device_count() <= device || device < 0) {
    set_error("no HIP device %d visible (this library has no CPU fallback)", device);
    return ERROR_NO_HIP_DEVICE;
  }
  HIP_TRY(hipSetDevice(device));
  ReadsPiled piled;
  if ((st = reads_pileup(in, piled))) return st;
  for (int k = 0; k < 2; k++) g_reads_ms[k] = piled.ms[k];
  long long off = 0;
  for (int c = 0; c < n_contigs && coverage_out; c++) {
    HIP_TRY(hipMemcpy(coverage_out + off, piled.coverage[(size_t)c],
                      sizeof(int) * (size_t)piled.n_bases[(size_t)c], hipMemcpyDeviceToHost));
    off += piled.n_bases[(size_t)c];
  }
  if (!runs_out && !count_out && !weight_out && !run_end_out) return 0;
  DenseEncoded enc;
  if ((st = dense_encode(n_contigs, piled.n_bases.data(), piled.coverage.data(), 1, enc))) return st;
  for (int k = 0; k < 3; k++) g_dense_ms[k] = enc.ms[k];
  for (int c = 0; c < n_contigs && runs_out; c++) runs_out[c] = enc.stats[(size_t)c].runs;
  return dense_download_and_free(enc, count_out, weight_out, run_end_out);
}

extern "C" int peakseg_hip_problem_set_create_reads(
    int device, int n_contigs, const long long *n_reads, const int *const *read_start,
    const int *const *read_end, const int *const *read_count, int reads_on_device,
    const int *extent_start, const int *extent_end, int bases_counted, int n_problems,
    const int *problem_contig, const double *problem_penalty, unsigned long long arena_pieces,
    psd_problem_set **out) {
  *out = nullptr;
  const ReadsInput in = {n_contigs, n_reads, read_start, read_end, read_count, reads_on_device,
                         extent_start, extent_end, bases_counted};
  int st = dense_check_penalties(n_problems, problem_penalty);
  if (st) return st;
  if ((st = reads_check_arguments(in))) return st;
  if ((st = dense_check_device_problems(device, n_contigs, n_problems, problem_contig))) return st;
  HIP_TRY(hipSetDevice(device));
  CreateLaps lap;
  DenseEncoded enc;
  std::vector<long long> n_bases;
  {
    ReadsPiled piled; /* the coverage buffer lives until the encoding ends */
    if ((st = reads_pileup(in, piled))) return st;
    for (int k = 0; k < 2; k++) g_reads_ms[k] = piled.ms[k];
    if (lap.on) {
      fprintf(stderr, "peakseg_hip timing: create: %-26s %8.3f s\n",
              reads_on_device ? "reads: tables" : "reads: upload, tables", piled.upload_s);
      fprintf(stderr, "peakseg_hip timing: create: %-26s %8.3f s\n", "reads: scatter kernel", piled.ms[0] / 1e3);
      fprintf(stderr, "peakseg_hip timing: create: %-26s %8.3f s\n", "reads: scan kernels", piled.ms[1] / 1e3);
    }
    lap("reads: pile-up in all");
    n_bases = piled.n_bases;
    if ((st = dense_encode(n_contigs, n_bases.data(), piled.coverage.data(), 1, enc))) return st;
  }
  return dense_create_encoded(device, n_contigs, n_bases.data(), 1, enc, lap, n_problems, problem_contig,
                              problem_penalty, arena_pieces, out);
}
