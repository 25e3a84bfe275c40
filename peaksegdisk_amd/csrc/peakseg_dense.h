/* peakseg_dense.h -- the host side of dense coverage: the run-length encoding on the device
 * (kernels: dense_encode.h), the creator from dense counts and what it shares with the creator from
 * reads (peakseg_reads.h), the loss row of a solved problem. */

namespace {

struct DenseEncoded {
  int *count = nullptr, *weight = nullptr, *run_end = nullptr; /* device, total_runs entries */
  long long total_runs = 0;
  std::vector<psd::dense::ContigStats> stats;
  std::vector<long long> run_off;
  float ms[3] = {0.f, 0.f, 0.f}; /* count, scan, scatter */
  double upload_s = 0.0;
};

struct DenseScratch { /* device memory of one encoding, freed when it ends */
  std::vector<void *> mem;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  ~DenseScratch() {
    for (void *q : mem) (void)hipFree(q);
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  template <class T>
  int get(T **p, size_t n) {
    void *q = nullptr;
    const size_t bytes = (n ? n : 1) * sizeof(T);
    const hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) {
      set_error("dense counts: hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
      return ERROR_DEVICE_MEMORY;
    }
    mem.push_back(q);
    *p = (T *)q;
    return 0;
  }
};

/* what the host can see of a dense call (after the penalties, before the device) */
int dense_check_lengths(int n_contigs, const long long *n_bases) {
  if (n_contigs <= 0 || !n_bases) {
    set_error("dense counts: no contig");
    return ERROR_NO_DATA;
  }
  for (int c = 0; c < n_contigs; c++)
    if (n_bases[c] <= 0) {
      set_error("dense counts: contig %d has no data", c);
      return ERROR_NO_DATA;
    }
  for (int c = 0; c < n_contigs; c++)
    if (n_bases[c] >= (1ll << 31)) {
      set_error("dense counts: contig %d has %lld bases, 2^31 or more", c, n_bases[c]);
      return ERROR_DENSE_ARGUMENTS;
    }
  return 0;
}

/* Stage 1 alone.  The device is set.  On success the three output arrays belong to the caller. */
int dense_encode(int n_contigs, const long long *n_bases, const int *const *counts,
                 int counts_on_device, DenseEncoded &enc) {
  namespace dn = psd::dense;
  DenseScratch scratch;
  const auto t_upload = std::chrono::steady_clock::now();
  std::vector<dn::Contig> contigs((size_t)n_contigs);
  long long n_tiles = 0;
  if (counts_on_device) {
    for (int c = 0; c < n_contigs; c++) {
      const unsigned long long addr = (unsigned long long)counts[c];
      if (!counts[c] || (addr & 3ull)) {
        set_error("dense counts: contig %d: the device address is %s", c,
                  counts[c] ? "not a multiple of 4" : "NULL");
        return ERROR_DENSE_ARGUMENTS;
      }
      contigs[(size_t)c].lead = (int)((addr >> 2) & 3ull);
      contigs[(size_t)c].base = counts[c] - contigs[(size_t)c].lead;
    }
  } else {
    /* the library's own copy: the contigs one after the other, each at a multiple of 16 bytes */
    long long total = 0;
    for (int c = 0; c < n_contigs; c++) total += (n_bases[c] + 3) & ~3ll;
    int *d_in = nullptr;
    int st = scratch.get(&d_in, (size_t)total);
    if (st) return st;
    long long off = 0;
    for (int c = 0; c < n_contigs; c++) {
      if (!counts || !counts[c]) {
        set_error("dense counts: contig %d: NULL", c);
        return ERROR_DENSE_ARGUMENTS;
      }
      HIP_TRY(hipMemcpy(d_in + off, counts[c], sizeof(int) * (size_t)n_bases[c], hipMemcpyHostToDevice));
      contigs[(size_t)c].lead = 0;
      contigs[(size_t)c].base = d_in + off;
      off += (n_bases[c] + 3) & ~3ll;
    }
  }
  for (int c = 0; c < n_contigs; c++) {
    dn::Contig &k = contigs[(size_t)c];
    k.n = n_bases[c];
    k.tile_first = n_tiles;
    k.run_off = 0;
    k.pad = 0;
    n_tiles += (k.lead + k.n + dn::TILE - 1) / dn::TILE;
  }
  /* (a grid dimension times the workgroup size stays below 2^32) */
  if (n_tiles >= (1ll << 24)) {
    set_error("dense counts: %lld tiles of %d bases in one call, 2^24 or more", n_tiles, dn::TILE);
    return ERROR_DENSE_ARGUMENTS;
  }
  std::vector<int> tile_contig((size_t)n_tiles);
  for (int c = 0; c < n_contigs; c++) {
    const long long end = c + 1 < n_contigs ? contigs[(size_t)c + 1].tile_first : n_tiles;
    std::fill(tile_contig.begin() + contigs[(size_t)c].tile_first, tile_contig.begin() + end, c);
  }
  dn::Contig *d_contigs = nullptr;
  int *d_tile_contig = nullptr;
  dn::TileInfo *d_tiles = nullptr;
  dn::TileScan *d_scan = nullptr;
  dn::ContigStats *d_stats = nullptr;
  int st = 0;
  if ((st = scratch.get(&d_contigs, (size_t)n_contigs)) ||
      (st = scratch.get(&d_tile_contig, (size_t)n_tiles)) ||
      (st = scratch.get(&d_tiles, (size_t)n_tiles)) || (st = scratch.get(&d_scan, (size_t)n_tiles)) ||
      (st = scratch.get(&d_stats, (size_t)n_contigs)))
    return st;
  HIP_TRY(hipMemcpy(d_contigs, contigs.data(), sizeof(dn::Contig) * (size_t)n_contigs, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_tile_contig, tile_contig.data(), sizeof(int) * (size_t)n_tiles, hipMemcpyHostToDevice));
  for (auto &e : scratch.ev) HIP_TRY(hipEventCreate(&e));
  hipStream_t stream = (hipStream_t) nullptr;
  enc.upload_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_upload).count();
  HIP_TRY(hipEventRecord(scratch.ev[0], stream));
  hipLaunchKernelGGL(dn::count_kernel, dim3((unsigned)n_tiles), dim3(dn::THREADS), 0, stream,
                     (const dn::Contig *)d_contigs, (const int *)d_tile_contig, d_tiles);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(scratch.ev[1], stream));
  hipLaunchKernelGGL(dn::scan_kernel, dim3((unsigned)n_contigs), dim3(dn::THREADS), 0, stream,
                     (const dn::Contig *)d_contigs, (const dn::TileInfo *)d_tiles, d_scan, d_stats);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(scratch.ev[2], stream));
  enc.stats.resize((size_t)n_contigs);
  HIP_TRY(hipMemcpy(enc.stats.data(), d_stats, sizeof(dn::ContigStats) * (size_t)n_contigs,
                    hipMemcpyDeviceToHost));
  enc.run_off.assign((size_t)n_contigs, 0);
  long long total_runs = 0;
  for (int c = 0; c < n_contigs; c++) {
    const dn::ContigStats &cs = enc.stats[(size_t)c];
    if (cs.mn < 0) {
      set_error("dense counts: contig %d holds a negative count (minimum %d)", c, cs.mn);
      return ERROR_DENSE_ARGUMENTS;
    }
    if (cs.sum >= (1ll << 53)) {
      set_error("dense counts: contig %d: the counts sum to %lld, 2^53 or more", c, cs.sum);
      return ERROR_DENSE_ARGUMENTS;
    }
    if (cs.runs >= (1ll << 30)) {
      set_error("dense counts: contig %d has %lld runs, 2^30 or more", c, cs.runs);
      return ERROR_DENSE_ARGUMENTS;
    }
    enc.run_off[(size_t)c] = total_runs;
    contigs[(size_t)c].run_off = total_runs;
    total_runs += cs.runs;
  }
  enc.total_runs = total_runs;
  HIP_TRY(hipMemcpy(d_contigs, contigs.data(), sizeof(dn::Contig) * (size_t)n_contigs, hipMemcpyHostToDevice));
  int *out[3] = {nullptr, nullptr, nullptr};
  for (auto &q : out) {
    const hipError_t e = hipMalloc(&q, sizeof(int) * (size_t)total_runs);
    if (e != hipSuccess) {
      set_error("dense counts: hipMalloc(%lld runs) failed: %s", total_runs, hipGetErrorString(e));
      for (auto &f : out)
        if (f) (void)hipFree(f);
      return ERROR_DEVICE_MEMORY;
    }
  }
  hipError_t e = hipEventRecord(scratch.ev[3], stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(dn::scatter_kernel, dim3((unsigned)n_tiles), dim3(dn::THREADS), 0, stream,
                       (const dn::Contig *)d_contigs, (const int *)d_tile_contig,
                       (const dn::TileScan *)d_scan, out[0], out[1], out[2]);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(scratch.ev[4], stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e == hipSuccess) e = hipEventElapsedTime(&enc.ms[0], scratch.ev[0], scratch.ev[1]);
  if (e == hipSuccess) e = hipEventElapsedTime(&enc.ms[1], scratch.ev[1], scratch.ev[2]);
  if (e == hipSuccess) e = hipEventElapsedTime(&enc.ms[2], scratch.ev[3], scratch.ev[4]);
  if (e != hipSuccess) {
    set_error("dense counts: the encoder failed: %s", hipGetErrorString(e));
    for (auto &f : out) (void)hipFree(f);
    return ERROR_DEVICE_SOLVER;
  }
  enc.count = out[0];
  enc.weight = out[1];
  enc.run_end = out[2];
  return 0;
}

/* the probes' end: the encoded arrays to the host (any may be NULL), then freed */
int dense_download_and_free(DenseEncoded &enc, int *count_out, int *weight_out, int *run_end_out) {
  const size_t bytes = sizeof(int) * (size_t)enc.total_runs;
  hipError_t e = hipSuccess;
  if (count_out) e = hipMemcpy(count_out, enc.count, bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess && weight_out) e = hipMemcpy(weight_out, enc.weight, bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess && run_end_out) e = hipMemcpy(run_end_out, enc.run_end, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(enc.count);
  (void)hipFree(enc.weight);
  (void)hipFree(enc.run_end);
  if (e != hipSuccess) {
    set_error("dense counts: download failed: %s", hipGetErrorString(e));
    return ERROR_DEVICE_SOLVER;
  }
  return 0;
}

thread_local float g_dense_ms[3] = {0.f, 0.f, 0.f};

}  // namespace

extern "C" int peakseg_hip_dense_tile_bases(void) { return psd::dense::TILE; }

extern "C" int peakseg_hip_dense_last_encode_ms(float *count_ms, float *scan_ms, float *scatter_ms) {
  if (count_ms) *count_ms = g_dense_ms[0];
  if (scan_ms) *scan_ms = g_dense_ms[1];
  if (scatter_ms) *scatter_ms = g_dense_ms[2];
  return 0;
}

extern "C" int peakseg_hip_dense_encode_probe(int device, int n_contigs, const long long *n_bases,
                                              const int *const *counts, int counts_on_device,
                                              long long *runs_out, int *count_out, int *weight_out,
                                              int *run_end_out, int *min_out, int *max_out,
                                              long long *sum_out) {
  int st = dense_check_lengths(n_contigs, n_bases);
  if (st) return st;
  if (peakseg_hip_device_count() <= device || device < 0) {
    set_error("no HIP device %d visible (this library has no CPU fallback)", device);
    return ERROR_NO_HIP_DEVICE;
  }
  HIP_TRY(hipSetDevice(device));
  DenseEncoded enc;
  st = dense_encode(n_contigs, n_bases, counts, counts_on_device, enc);
  if (st) return st;
  for (int k = 0; k < 3; k++) g_dense_ms[k] = enc.ms[k];
  for (int c = 0; c < n_contigs; c++) {
    if (runs_out) runs_out[c] = enc.stats[(size_t)c].runs;
    if (min_out) min_out[c] = enc.stats[(size_t)c].mn;
    if (max_out) max_out[c] = enc.stats[(size_t)c].mx;
    if (sum_out) sum_out[c] = enc.stats[(size_t)c].sum;
  }
  return dense_download_and_free(enc, count_out, weight_out, run_end_out);
}

namespace {

/* penalties first: the reference validates them before it opens its input (drv:145-159) */
int dense_check_penalties(int n_problems, const double *problem_penalty) {
  for (int p = 0; p < n_problems; p++) {
    const double pen = problem_penalty[p];
    if (pen == INFINITY) continue;
    if (!std::isfinite(pen)) {
      set_error("problem %d: penalty is not finite", p);
      return ERROR_PENALTY_NOT_FINITE;
    }
    if (pen < 0) {
      set_error("problem %d: penalty is negative", p);
      return ERROR_PENALTY_NEGATIVE;
    }
  }
  return 0;
}

/* the device and the problem list, once the host has nothing left to say about the data */
int dense_check_device_problems(int device, int n_contigs, int n_problems, const int *problem_contig) {
  if (peakseg_hip_device_count() <= device || device < 0) {
    set_error("no HIP device %d visible (this library has no CPU fallback)", device);
    return ERROR_NO_HIP_DEVICE;
  }
  if (n_problems <= 0) {
    set_error("empty problem set");
    return ERROR_DEVICE_SOLVER;
  }
  for (int p = 0; p < n_problems; p++)
    if (problem_contig[p] < 0 || problem_contig[p] >= n_contigs) {
      set_error("problem %d names contig %d", p, problem_contig[p]);
      return ERROR_DEVICE_SOLVER;
    }
  return 0;
}

/* What every creator of a dense set does once dense_encode() has succeeded: the encoder's laps,
 * the set around the encoded arrays (which it owns from here on), create_common.  `lap` has been
 * running since the creator began. */
int dense_create_encoded(int device, int n_contigs, const long long *contig_n_bases,
                         int counts_on_device, DenseEncoded &enc, CreateLaps &lap, int n_problems,
                         const int *problem_contig, const double *problem_penalty,
                         unsigned long long arena_pieces, psd_problem_set **out) {
  int st = 0;
  for (int k = 0; k < 3; k++) g_dense_ms[k] = enc.ms[k];
  if (lap.on) {
    fprintf(stderr, "peakseg_hip timing: create: %-26s %8.3f s\n",
            counts_on_device ? "dense: tables" : "dense: upload, tables", enc.upload_s);
    fprintf(stderr, "peakseg_hip timing: create: %-26s %8.3f s\n", "dense: count kernel", enc.ms[0] / 1e3);
    fprintf(stderr, "peakseg_hip timing: create: %-26s %8.3f s\n", "dense: scan kernel", enc.ms[1] / 1e3);
    fprintf(stderr, "peakseg_hip timing: create: %-26s %8.3f s\n", "dense: scatter kernel", enc.ms[2] / 1e3);
  }
  lap("dense: encoder in all");
  SetOwner set(new psd_problem_set(), peakseg_hip_problem_set_destroy);
  psd_problem_set *s = set.get();
  s->device = device;
  s->n_contigs = n_contigs;
  s->n_problems = n_problems;
  s->dense = true;
  for (int *q : {enc.count, enc.weight, enc.run_end}) s->allocs.push_back(q);
  s->bytes += 12ull * (unsigned long long)enc.total_runs;
  s->d.count = enc.count;
  s->d.weight = enc.weight;
  s->d_run_end = enc.run_end;
  std::vector<double> min_lm((size_t)n_contigs), max_lm((size_t)n_contigs);
  for (int c = 0; c < n_contigs; c++) {
    const psd::dense::ContigStats &cs = enc.stats[(size_t)c];
    s->contig_n.push_back((int)cs.runs);
    s->contig_off.push_back(enc.run_off[(size_t)c]);
    s->contig_bases.push_back(contig_n_bases[c]);
    s->contig_sum.push_back(cs.sum);
    s->contig_constant.push_back(cs.mn == cs.mx);
    s->contig_max.push_back(cs.mx);
    /* psd_log is strictly increasing on the integers: the logs of the integer extremes are the
     * extremes of the logs (drv:198-204) */
    min_lm[(size_t)c] = psd_log((double)cs.mn);
    max_lm[(size_t)c] = psd_log((double)cs.mx);
  }
  if ((st = dev_alloc(s, &s->d_order_run, (size_t)n_problems))) return st;
  return create_common(std::move(set), lap, min_lm, max_lm, nullptr, nullptr, problem_contig, problem_penalty,
                       arena_pieces, out);
}

}  // namespace

extern "C" int peakseg_hip_problem_set_create_dense(int device, int n_contigs,
                                                    const long long *contig_n_bases,
                                                    const int *const *contig_counts,
                                                    int counts_on_device, int n_problems,
                                                    const int *problem_contig,
                                                    const double *problem_penalty,
                                                    unsigned long long arena_pieces,
                                                    psd_problem_set **out) {
  *out = nullptr;
  int st = dense_check_penalties(n_problems, problem_penalty);
  if (st) return st;
  if ((st = dense_check_lengths(n_contigs, contig_n_bases))) return st;
  if ((st = dense_check_device_problems(device, n_contigs, n_problems, problem_contig))) return st;
  HIP_TRY(hipSetDevice(device));
  CreateLaps lap;
  DenseEncoded enc;
  if ((st = dense_encode(n_contigs, contig_n_bases, contig_counts, counts_on_device, enc))) return st;
  return dense_create_encoded(device, n_contigs, contig_n_bases, counts_on_device, enc, lap, n_problems,
                              problem_contig, problem_penalty, arena_pieces, out);
}

/* the reference's loss row: write_dp_outputs and write_trivial in peakseg_files.h */
extern "C" int peakseg_hip_problem_set_loss(psd_problem_set *s, int p, double *out) {
  if (!s || !s->solved || !out || p < 0 || p >= s->n_problems) return -1;
  const psd::ProbResult &r = s->results[(size_t)p];
  if (r.status != 0) return -1;
  const int c = s->prob_contig[(size_t)p];
  const double cum_weight = (double)s->contig_bases[(size_t)c];
  const int n = s->contig_n[(size_t)c];
  const double penalty = s->prob_penalty[(size_t)p];
  out[0] = penalty;
  out[3] = (double)(int)cum_weight;
  out[4] = (double)n;
  if (trivial_model(s, p)) {
    const double best_cost = trivial_best_cost(s, c);
    out[1] = 1;
    out[2] = 0;
    out[5] = best_cost / cum_weight;
    out[6] = best_cost;
    out[7] = out[8] = out[9] = 0;
    return 0;
  }
  const int n_peaks = (r.n_segments - 1) / 2;
  const double total_intervals = (double)r.total_intervals;
  out[1] = (double)r.n_segments;
  out[2] = (double)n_peaks;
  out[5] = r.best_cost;
  out[6] = r.best_cost * cum_weight - penalty * n_peaks;
  out[7] = (double)r.n_equality;
  out[8] = total_intervals / (n * 2);
  out[9] = (double)r.max_intervals;
  return 0;
}
