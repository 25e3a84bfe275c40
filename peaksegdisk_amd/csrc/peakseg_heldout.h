/* peakseg_heldout.h -- the host side of the held-out loss (kernels: heldout_loss.h, and the fold of
 * region_stats.h through regions_fold of peakseg_regions.h): the checks of the pairs, the problems'
 * descriptors, the question whether the call fits, the launches between two events, the download.
 * Nothing here writes what a solve or another pack_* call leaves.  Below it, the creators of fold
 * sets (kernels: fold_units.h), which hand the folds to the stages of peakseg_dense.h and
 * peakseg_reads.h. */

namespace {

thread_local float g_heldout_ms = 0.f;

const char *heldout_reason_text(int why) {
  namespace ho = psd::heldout;
  switch (why) {
    case ho::BAD_PROBLEM: return "its problem is out of range";
    case ho::BAD_CONTIG: return "its contig is out of range";
    case ho::BAD_SCALE: return "its scale is not finite and positive";
    case ho::BAD_BASES: return "its contig has not the bases of its problem's contig";
    default: return "it cannot be scored";
  }
}

/* the bytes of the columns of n pairs, of the library's copy of host pairs, and of r rows */
unsigned long long heldout_pair_bytes(long long n) {
  return (unsigned long long)n * (4 + 8 + 4 + 8 + 8 + 4) +
         (unsigned long long)(n / psd::heldout::THREADS + 2) * 8;
}
unsigned long long heldout_copy_bytes(long long n) { return (unsigned long long)n * (4 + 4 + 8); }
unsigned long long heldout_row_bytes(long long r) { return (unsigned long long)r * 12; }

/* ERROR_DEVICE_MEMORY with its text when `more` bytes do not fit, else 0 */
int heldout_fits(const psd_problem_set *s, unsigned long long more, long long pairs, long long rows) {
  size_t free_b = 0, total_b = 0;
  const bool known = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
  /* (a call that needs nothing more fits, whatever other services' arrays have grown to) */
  if ((s->max_bytes && more > 0 && s->bytes + more > s->max_bytes) ||
      (known && more > (unsigned long long)free_b)) {
    set_error("pack_heldout_loss: %lld pairs of %lld rows need %llu more bytes, which do not fit "
              "(free HBM / PEAKSEG_HIP_MAX_BYTES)", pairs, rows, more);
    return ERROR_DEVICE_MEMORY;
  }
  return 0;
}

/* 0 or a status; the device is set, n > 0, and the arrays are not NULL */
int heldout_run(psd_problem_set *s, long long n, const int *problem, const int *contig,
                const double *scale, int on_device) {
  namespace ho = psd::heldout;
  namespace rg = psd::regions;
  HeldoutTable &t = s->heldout;
  RegionTable &ft = t.fold;
  const size_t np = (size_t)s->n_problems, nc = (size_t)s->n_contigs;
  int st = 0;
  /* (a grid dimension times the workgroup size stays below 2^32; a pair is a workgroup) */
  if (n >= (1ll << 31)) {
    set_error("pack_heldout_loss: %lld pairs in one call", n);
    return ERROR_HELDOUT_ARGUMENTS;
  }
  /* the problems as the kernels read them */
  std::vector<ho::Problem> problems(np);
  long long most_tiles = 1;
  for (size_t p = 0; p < np; p++) {
    const psd::ProbResult &r = s->results[p];
    const size_t c = (size_t)s->prob_contig[p];
    ho::Problem &q = problems[p];
    q.seg_off = s->prob_seg_off[p];
    q.run0 = s->contig_off[c];
    q.bases = s->contig_bases[c];
    q.rows = r.status == 0 ? r.n_segments : 0;
    q.pad = 0;
    /* (the scan of a workgroup's row counts is 32-bit) */
    if (q.rows >= (1 << 22)) {
      set_error("pack_heldout_loss: problem %d has %d rows, 2^22 or more", (int)p, q.rows);
      return ERROR_DEVICE_SOLVER;
    }
  }
  for (size_t c = 0; c < nc; c++) {
    const long long tiles = ((s->contig_off[c] & 3) + s->contig_n[c] + rg::TILE - 1) / rg::TILE;
    most_tiles = tiles > most_tiles ? tiles : most_tiles;
  }
  /* host arrays: checked here, and their rows counted, before anything is allocated */
  long long rows = -1;
  if (!on_device) {
    rows = 0;
    for (long long i = 0; i < n; i++) {
      const int p = problem[i], c = contig[i];
      const double a = scale[i];
      if (p < 0 || p >= s->n_problems) {
        set_error("pack_heldout_loss: pair %lld: problem %d is outside 0 .. %d", i, p, s->n_problems - 1);
        return ERROR_HELDOUT_ARGUMENTS;
      }
      if (c < 0 || c >= s->n_contigs) {
        set_error("pack_heldout_loss: pair %lld: contig %d is outside 0 .. %d", i, c, s->n_contigs - 1);
        return ERROR_HELDOUT_ARGUMENTS;
      }
      if (!(a > 0.0) || !(a < INFINITY)) {
        set_error("pack_heldout_loss: pair %lld: scale %g is not finite and positive", i, a);
        return ERROR_HELDOUT_ARGUMENTS;
      }
      if (s->contig_bases[(size_t)c] != problems[(size_t)p].bases) {
        set_error("pack_heldout_loss: pair %lld: contig %d has %lld bases, the contig of problem %d "
                  "has %lld", i, c, s->contig_bases[(size_t)c], p, problems[(size_t)p].bases);
        return ERROR_HELDOUT_ARGUMENTS;
      }
      rows += problems[(size_t)p].rows;
    }
  }
  /* does the call fit?  asked before anything is allocated (device arrays: the rows are known
   * after the first launch, and are asked about then) */
  auto more_for = [&](long long r) {
    unsigned long long more = 0;
    if (!t.d_problems) more += (np ? np : 1) * sizeof(ho::Problem) + (nc ? nc : 1) * 8 + sizeof(ho::Head);
    if (n > t.pair_capacity) more += heldout_pair_bytes(n) - (t.pair_capacity ? heldout_pair_bytes(t.pair_capacity) : 0ull);
    if (!on_device && n > t.copy_capacity) more += heldout_copy_bytes(n) - heldout_copy_bytes(t.copy_capacity);
    const long long rr = r > 0 ? r : 1;
    if (rr > t.row_capacity) more += heldout_row_bytes(rr) - heldout_row_bytes(t.row_capacity);
    return more + regions_room_bytes(s, ft, rr);
  };
  if ((st = heldout_fits(s, more_for(rows), n, rows > 0 ? rows : 0))) return st;
  for (auto &e : t.ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  /* (the set's geometry: their sizes never change) */
  if ((!t.d_problems && (st = dev_alloc(s, &t.d_problems, np))) ||
      (!t.d_contig_bases && (st = dev_alloc(s, &t.d_contig_bases, nc))) ||
      (!t.d_head && (st = dev_alloc(s, &t.d_head, 1))))
    return st;
  if (n > t.pair_capacity) {
    const long long have = t.pair_capacity;
    t.pair_capacity = 0;
    if ((st = label_room(s, t.off, have, n)) || (st = label_room(s, t.loss, have, n)) ||
        (st = label_room(s, t.rows, have, n)) || (st = label_room(s, t.bases, have, n)) ||
        (st = label_room(s, t.sum, have, n)) || (st = label_room(s, t.zero, have, n)) ||
        (st = label_room(s, t.block_sum, have ? have / ho::THREADS + 2 : 0, n / ho::THREADS + 2)))
      return st;
    t.pair_capacity = n;
  }
  if (!on_device && n > t.copy_capacity) {
    const long long have = t.copy_capacity;
    t.copy_capacity = 0;
    if ((st = label_room(s, t.d_pairs, 2 * have, 2 * n)) || (st = label_room(s, t.d_scale, have, n)))
      return st;
    t.copy_capacity = n;
  }
  if ((st = regions_room(s, ft, rows > 0 ? rows : 1))) return st;
  if (np > 0)
    HIP_TRY(hipMemcpy(t.d_problems, problems.data(), sizeof(ho::Problem) * np, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t.d_contig_bases, s->contig_bases.data(), sizeof(long long) * nc, hipMemcpyHostToDevice));
  {
    const std::vector<long long> no_regions(nc + 1, 0);
    const std::vector<const int *> none;
    if ((st = regions_contigs(s, ft, nullptr, no_regions, none, none, nullptr))) return st;
  }
  const int *d_problem = problem, *d_contig = contig;
  const double *d_scale = scale;
  if (!on_device) {
    HIP_TRY(hipMemcpy(t.d_pairs, problem, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t.d_pairs + n, contig, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t.d_scale, scale, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    d_problem = t.d_pairs;
    d_contig = t.d_pairs + n;
    d_scale = t.d_scale;
  } else {
    /* (device arrays: what the caller queued on the null stream -- torch's default -- has run) */
    HIP_TRY(hipStreamSynchronize((hipStream_t) nullptr));
  }
  const long long nb = (n + ho::THREADS - 1) / ho::THREADS;
  HIP_TRY(hipEventRecord(t.ev[0], s->stream));
  HIP_TRY(hipMemsetAsync(t.d_head, 0, sizeof(ho::Head), s->stream));
  hipLaunchKernelGGL(ho::pairs_kernel<>, dim3((unsigned)nb), dim3(ho::THREADS), 0, s->stream, n,
                     d_problem, d_contig, d_scale, (const ho::Problem *)t.d_problems, s->n_problems,
                     (const long long *)t.d_contig_bases, s->n_contigs, t.off, t.block_sum, t.d_head);
  HIP_TRY(hipGetLastError());
  if (on_device) { /* nothing further is launched after a bad pair */
    ho::Head head;
    HIP_TRY(hipMemcpyAsync(&head, t.d_head, sizeof head, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (head.check) {
      const int why = (int)(head.check & ((1ull << ho::REASON_BITS) - 1ull));
      const long long i = (long long)((~(head.check >> ho::REASON_BITS)) & ((1ull << (64 - ho::REASON_BITS)) - 1ull));
      set_error("pack_heldout_loss: pair %lld: %s", i, heldout_reason_text(why));
      return ERROR_HELDOUT_ARGUMENTS;
    }
    rows = head.rows;
    if ((st = heldout_fits(s, more_for(rows), n, rows))) return st;
  }
  if ((rows + ho::THREADS - 1) / ho::THREADS >= (1ll << 24)) {
    set_error("pack_heldout_loss: %lld rows in one call", rows);
    return ERROR_HELDOUT_ARGUMENTS;
  }
  {
    const long long need = rows > 0 ? rows : 1, have = t.row_capacity;
    if (need > have) {
      t.row_capacity = 0;
      if ((st = label_room(s, t.flat_start, have, need)) || (st = label_room(s, t.flat_end, have, need)) ||
          (st = label_room(s, t.flat_contig, have, need)))
        return st;
      t.row_capacity = need;
    }
    if ((st = regions_room(s, ft, need))) return st;
  }
  hipLaunchKernelGGL(rg::scan_top_kernel, dim3(1), dim3(rg::THREADS), 0, s->stream, t.block_sum, nb);
  HIP_TRY(hipGetLastError());
  if (rows > 0) {
    hipLaunchKernelGGL(ho::rows_kernel<>, dim3((unsigned)((rows + ho::THREADS - 1) / ho::THREADS)),
                       dim3(ho::THREADS), 0, s->stream, n, d_problem, d_contig,
                       (const ho::Problem *)t.d_problems, (const int *)t.off,
                       (const long long *)t.block_sum, (const ho::Head *)t.d_head,
                       (const int *)s->d.seg_start, (const int *)s->d_run_end, t.flat_start, t.flat_end,
                       t.flat_contig);
    HIP_TRY(hipGetLastError());
    if ((st = regions_fold(s, ft, rows, (const int *)t.flat_start, (const int *)t.flat_end,
                           (const int *)t.flat_contig, rows * most_tiles, false, []() { return 0; })))
      return st;
  }
  hipLaunchKernelGGL(ho::loss_kernel<>, dim3((unsigned)n), dim3(ho::THREADS), 0, s->stream, n, d_problem,
                     d_scale, (const ho::Problem *)t.d_problems, (const int *)t.off,
                     (const long long *)t.block_sum, (const double *)s->d.seg_mean, (const int *)ft.bases,
                     (const long long *)ft.sum, t.loss, t.rows, t.bases, t.sum, t.zero);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(t.ev[1], s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipEventElapsedTime(&g_heldout_ms, t.ev[0], t.ev[1]));
  return 0;
}

}  // namespace

extern "C" long long peakseg_hip_problem_set_pack_heldout_loss(
    psd_problem_set *s, long long n_pairs, const int *problem, const int *contig, const double *scale,
    int pairs_on_device, const double **loss_dev, const int **rows_dev, const long long **bases_dev,
    const long long **sum_dev, const int **zero_mean_rows_dev) {
  if (!s) return -1;
  if (!s->dense) {
    set_error("pack_heldout_loss: the set was not made from dense counts or reads and has no run_end[]");
    return -1;
  }
  if (!s->solved) {
    set_error("pack_heldout_loss: the set is not solved");
    return -1;
  }
  if (hipSetDevice(s->device) != hipSuccess) return -1;
  s->heldout.pairs = -1;
  if (n_pairs < 0) {
    set_error("pack_heldout_loss: %lld pairs", n_pairs);
    return -ERROR_HELDOUT_ARGUMENTS;
  }
  if (n_pairs > 0) {
    const void *arrays[3] = {problem, contig, scale};
    const char *const what[3] = {"problem", "contig", "scale"};
    for (int j = 0; j < 3; j++) {
      const unsigned long long align = j == 2 ? 7ull : 3ull;
      if (!arrays[j] || (pairs_on_device && ((unsigned long long)arrays[j] & align))) {
        set_error("pack_heldout_loss: the %s array is %s", what[j],
                  arrays[j] ? "at a misaligned device address" : "NULL");
        return -ERROR_HELDOUT_ARGUMENTS;
      }
    }
    g_heldout_ms = 0.f;
    const int st = heldout_run(s, n_pairs, problem, contig, scale, pairs_on_device);
    if (st) return st == ERROR_HELDOUT_ARGUMENTS || st == ERROR_DEVICE_MEMORY ? -st : -1;
  }
  const HeldoutTable &t = s->heldout;
  s->heldout.pairs = n_pairs;
  if (loss_dev) *loss_dev = t.loss;
  if (rows_dev) *rows_dev = t.rows;
  if (bases_dev) *bases_dev = t.bases;
  if (sum_dev) *sum_dev = t.sum;
  if (zero_mean_rows_dev) *zero_mean_rows_dev = t.zero;
  return n_pairs;
}

extern "C" int peakseg_hip_problem_set_packed_heldout_loss_download(psd_problem_set *s, double *loss_out,
                                                                    int *rows_out, long long *bases_out,
                                                                    long long *sum_out,
                                                                    int *zero_mean_rows_out) {
  if (!s || s->heldout.pairs < 0) return -1;
  const size_t n = (size_t)s->heldout.pairs;
  const HeldoutTable &t = s->heldout;
  const void *from[5] = {t.loss, t.rows, t.bases, t.sum, t.zero};
  void *to[5] = {loss_out, rows_out, bases_out, sum_out, zero_mean_rows_out};
  const size_t width[5] = {8, 4, 8, 8, 4};
  for (int k = 0; k < 5 && n > 0; k++)
    if (to[k] && hipMemcpy(to[k], from[k], n * width[k], hipMemcpyDeviceToHost) != hipSuccess) {
      set_error("download of the packed held-out losses failed");
      return -1;
    }
  return 0;
}

extern "C" int peakseg_hip_heldout_loss_last_ms(float *ms) {
  if (ms) *ms = g_heldout_ms;
  return 0;
}

/* ---- the folds: the units of every input contig split on the device (kernels: fold_units.h), and
 *      the set of their train and test contigs made by the creators' own stages ------------------ */

namespace {

thread_local float g_fold_units_ms = 0.f;

/* 0, or ERROR_HELDOUT_ARGUMENTS with its text; bits: log2 folds */
int folds_check(int folds, int *bits) {
  if (folds != 2 && folds != 4 && folds != 8) {
    set_error("folds is %d, not 2, 4 or 8", folds);
    return ERROR_HELDOUT_ARGUMENTS;
  }
  *bits = folds == 2 ? 1 : (folds == 4 ? 2 : 3);
  return 0;
}

/* the problems of a fold set: (i K + f) P + j is train contig (i K + f) 2 at penalties[j] */
int folds_problems(int n_contigs, int folds, int n_penalties, const double *penalties,
                   std::vector<int> &contig, std::vector<double> &penalty) {
  if (n_penalties <= 0 || !penalties) {
    set_error("empty problem set: no penalty");
    return ERROR_DEVICE_SOLVER;
  }
  const long long np = (long long)n_contigs * folds * n_penalties;
  if (np >= (1ll << 31) || (long long)n_contigs * folds * 2 >= (1ll << 31)) {
    set_error("folds: %d contigs x %d folds x %d penalties are 2^31 problems or more", n_contigs, folds,
              n_penalties);
    return ERROR_HELDOUT_ARGUMENTS;
  }
  contig.resize((size_t)np);
  penalty.resize((size_t)np);
  for (long long p = 0; p < np; p++) {
    contig[(size_t)p] = (int)(p / n_penalties) * 2;
    penalty[(size_t)p] = penalties[p % n_penalties];
  }
  return 0;
}

}  // namespace

extern "C" int peakseg_hip_fold_max_count(void) { return psd::folds::MAX_COUNT; }

extern "C" int peakseg_hip_fold_units_last_ms(float *ms) {
  if (ms) *ms = g_fold_units_ms;
  return 0;
}

extern "C" int peakseg_hip_problem_set_create_dense_folds(
    int device, int n_contigs, const long long *contig_n_bases, const int *const *contig_counts,
    int counts_on_device, int n_penalties, const double *penalties, unsigned long long arena_pieces,
    int folds, unsigned long long seed, psd_problem_set **out) {
  namespace fo = psd::folds;
  *out = nullptr;
  int bits = 0, st = folds_check(folds, &bits);
  if (st) return st;
  if (n_penalties > 0 && penalties && (st = dense_check_penalties(n_penalties, penalties))) return st;
  if ((st = dense_check_lengths(n_contigs, contig_n_bases))) return st;
  std::vector<int> problem_contig;
  std::vector<double> problem_penalty;
  if ((st = folds_problems(n_contigs, folds, n_penalties, penalties, problem_contig, problem_penalty)))
    return st;
  const int nc2 = n_contigs * folds * 2;
  if ((st = dense_check_device_problems(device, nc2, (int)problem_contig.size(), problem_contig.data())))
    return st;
  for (int c = 0; c < n_contigs; c++) {
    const int *v = contig_counts ? contig_counts[c] : nullptr;
    if (!v || (counts_on_device && ((unsigned long long)v & 3ull))) {
      set_error("dense counts: contig %d: %s", c, v ? "the device address is not a multiple of 4" : "NULL");
      return ERROR_DENSE_ARGUMENTS;
    }
    if (counts_on_device) continue;
    for (long long b = 0; b < contig_n_bases[c]; b++) {
      if (v[b] < 0) {
        set_error("dense counts: contig %d holds a negative count (%d at base %lld)", c, v[b], b);
        return ERROR_DENSE_ARGUMENTS;
      }
      if (v[b] > fo::MAX_COUNT) {
        set_error("folds: contig %d: base %lld has the count %d, above %d", c, b, v[b], fo::MAX_COUNT);
        return ERROR_HELDOUT_ARGUMENTS;
      }
    }
  }
  HIP_TRY(hipSetDevice(device));
  CreateLaps lap;
  DenseScratch scratch; /* the inputs' copy and the folds: freed when the encoding has ended */
  std::vector<fo::DenseContig> contigs((size_t)n_contigs);
  long long in_ints = 0, out_ints = 0, n_all = 0;
  for (int c = 0; c < n_contigs; c++) {
    fo::DenseContig &k = contigs[(size_t)c];
    k.first = n_all;
    k.n = contig_n_bases[c];
    k.stride = (k.n + 3) & ~3ll;
    n_all += k.n;
    in_ints += k.stride;
    out_ints += k.stride * 2 * folds;
  }
  /* (a grid dimension times the workgroup size stays below 2^32) */
  if ((n_all + fo::THREADS - 1) / fo::THREADS >= (1ll << 24)) {
    set_error("folds: %lld bases in one call", n_all);
    return ERROR_HELDOUT_ARGUMENTS;
  }
  int *d_in = nullptr, *d_out = nullptr;
  fo::DenseContig *d_contigs = nullptr;
  unsigned long long *d_check = nullptr;
  if ((!counts_on_device && (st = scratch.get(&d_in, (size_t)in_ints))) ||
      (st = scratch.get(&d_out, (size_t)out_ints)) || (st = scratch.get(&d_contigs, (size_t)n_contigs)) ||
      (st = scratch.get(&d_check, 1)))
    return st;
  std::vector<long long> n_bases2((size_t)nc2);
  std::vector<const int *> counts2((size_t)nc2);
  long long in_off = 0, out_off = 0;
  for (int c = 0; c < n_contigs; c++) {
    fo::DenseContig &k = contigs[(size_t)c];
    if (counts_on_device) {
      k.in = (const gint *)contig_counts[c];
    } else {
      HIP_TRY(hipMemcpy(d_in + in_off, contig_counts[c], sizeof(int) * (size_t)k.n, hipMemcpyHostToDevice));
      k.in = (const gint *)(d_in + in_off);
      in_off += k.stride;
    }
    k.out = (gint *)(d_out + out_off);
    for (int q = 0; q < 2 * folds; q++) {
      n_bases2[(size_t)(c * folds * 2 + q)] = k.n;
      counts2[(size_t)(c * folds * 2 + q)] = d_out + out_off + q * k.stride;
    }
    out_off += k.stride * 2 * folds;
  }
  HIP_TRY(hipMemcpy(d_contigs, contigs.data(), sizeof(fo::DenseContig) * (size_t)n_contigs, hipMemcpyHostToDevice));
  hipStream_t stream = (hipStream_t) nullptr;
  for (int k = 0; k < 2; k++) HIP_TRY(hipEventCreate(&scratch.ev[k]));
  HIP_TRY(hipMemsetAsync(d_check, 0, 8, stream));
  HIP_TRY(hipEventRecord(scratch.ev[0], stream));
  const dim3 grid((unsigned)((n_all + fo::THREADS - 1) / fo::THREADS)), block(fo::THREADS);
  if (bits == 1)
    hipLaunchKernelGGL(fo::dense_kernel<1>, grid, block, 0, stream, (const fo::DenseContig *)d_contigs,
                       n_contigs, n_all, seed, d_check);
  else if (bits == 2)
    hipLaunchKernelGGL(fo::dense_kernel<2>, grid, block, 0, stream, (const fo::DenseContig *)d_contigs,
                       n_contigs, n_all, seed, d_check);
  else
    hipLaunchKernelGGL(fo::dense_kernel<3>, grid, block, 0, stream, (const fo::DenseContig *)d_contigs,
                       n_contigs, n_all, seed, d_check);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(scratch.ev[1], stream));
  unsigned long long check = 0;
  HIP_TRY(hipMemcpy(&check, d_check, 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipEventElapsedTime(&g_fold_units_ms, scratch.ev[0], scratch.ev[1]));
  if (check) {
    const long long g = (long long)((~(check >> 1)) & ((1ull << 63) - 1ull));
    int c = n_contigs - 1;
    while (c > 0 && contigs[(size_t)c].first > g) c--;
    if (check & 1ull) {
      set_error("dense counts: contig %d holds a negative count (at base %lld)", c, g - contigs[(size_t)c].first);
      return ERROR_DENSE_ARGUMENTS;
    }
    set_error("folds: contig %d: base %lld has a count above %d", c, g - contigs[(size_t)c].first,
              fo::MAX_COUNT);
    return ERROR_HELDOUT_ARGUMENTS;
  }
  lap("folds: dense units");
  DenseEncoded enc;
  if ((st = dense_encode(nc2, n_bases2.data(), counts2.data(), 1, enc))) return st;
  return dense_create_encoded(device, nc2, n_bases2.data(), 1, enc, lap, (int)problem_contig.size(),
                              problem_contig.data(), problem_penalty.data(), arena_pieces, out);
}

extern "C" int peakseg_hip_problem_set_create_reads_folds(
    int device, int n_contigs, const long long *n_reads, const int *const *read_start,
    const int *const *read_end, const int *const *read_count, int reads_on_device,
    const int *extent_start, const int *extent_end, int bases_counted, int n_penalties,
    const double *penalties, unsigned long long arena_pieces, int folds, unsigned long long seed,
    psd_problem_set **out) {
  namespace fo = psd::folds;
  *out = nullptr;
  int bits = 0, st = folds_check(folds, &bits);
  if (st) return st;
  const ReadsInput in = {n_contigs, n_reads, read_start, read_end, read_count, reads_on_device,
                         extent_start, extent_end, bases_counted};
  if (n_penalties > 0 && penalties && (st = dense_check_penalties(n_penalties, penalties))) return st;
  if ((st = reads_check_arguments(in))) return st;
  std::vector<int> problem_contig;
  std::vector<double> problem_penalty;
  if ((st = folds_problems(n_contigs, folds, n_penalties, penalties, problem_contig, problem_penalty)))
    return st;
  const int nc2 = n_contigs * folds * 2;
  if ((st = dense_check_device_problems(device, nc2, (int)problem_contig.size(), problem_contig.data())))
    return st;
  long long n_all = 0, read_ints = 0;
  for (int c = 0; c < n_contigs; c++) {
    const bool counted = read_count && read_count[c] && n_reads[c] > 0;
    n_all += n_reads[c];
    read_ints += n_reads[c] * (counted ? 3 : 2);
    if (reads_on_device) continue;
    /* host arrays: checked here, where the input's contig can be named (the pile-up sees the folds') */
    for (long long i = 0; i < n_reads[c]; i++) {
      if (read_start[c][i] >= read_end[c][i]) {
        set_error("reads: contig %d: read %lld has chromStart %d >= chromEnd %d", c, i, read_start[c][i],
                  read_end[c][i]);
        return ERROR_READS_ARGUMENTS;
      }
      if (counted && read_count[c][i] < 0) {
        set_error("reads: contig %d: read %lld has the negative count %d", c, i, read_count[c][i]);
        return ERROR_READS_ARGUMENTS;
      }
    }
  }
  if ((n_all + fo::THREADS - 1) / fo::THREADS >= (1ll << 24)) {
    set_error("folds: %lld reads in one call", n_all);
    return ERROR_HELDOUT_ARGUMENTS;
  }
  HIP_TRY(hipSetDevice(device));
  CreateLaps lap;
  DenseScratch scratch; /* the reads' copy and the folds' count columns: freed after the pile-up */
  int *d_reads = nullptr, *d_cols = nullptr;
  fo::ReadsContig *d_contigs = nullptr;
  if ((!reads_on_device && (st = scratch.get(&d_reads, (size_t)read_ints))) ||
      (st = scratch.get(&d_cols, (size_t)(n_all * 2 * folds))) ||
      (st = scratch.get(&d_contigs, (size_t)n_contigs)))
    return st;
  std::vector<fo::ReadsContig> contigs((size_t)n_contigs);
  std::vector<long long> n_reads2((size_t)nc2);
  std::vector<const int *> start2((size_t)nc2), end2((size_t)nc2), count2((size_t)nc2);
  std::vector<int> lo2((size_t)nc2), hi2((size_t)nc2);
  long long read_off = 0, first = 0;
  for (int c = 0; c < n_contigs; c++) {
    const long long n = n_reads[c];
    const int *arrays[3] = {n ? read_start[c] : nullptr, n ? read_end[c] : nullptr,
                            n && read_count ? read_count[c] : nullptr};
    if (!reads_on_device)
      for (auto &a : arrays) { /* the library's own copy, one array after the other */
        if (!a) continue;
        HIP_TRY(hipMemcpy(d_reads + read_off, a, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
        a = d_reads + read_off;
        read_off += n;
      }
    fo::ReadsContig &k = contigs[(size_t)c];
    k.count = (const gint *)arrays[2];
    k.out = (gint *)(d_cols + first * 2 * folds);
    k.first = first;
    k.n = n;
    for (int q = 0; q < 2 * folds; q++) {
      const size_t c2 = (size_t)(c * folds * 2 + q);
      n_reads2[c2] = n;
      start2[c2] = arrays[0];
      end2[c2] = arrays[1];
      count2[c2] = n ? d_cols + first * 2 * folds + q * n : nullptr;
      lo2[c2] = extent_start[c];
      hi2[c2] = extent_end[c];
    }
    first += n;
  }
  HIP_TRY(hipMemcpy(d_contigs, contigs.data(), sizeof(fo::ReadsContig) * (size_t)n_contigs, hipMemcpyHostToDevice));
  hipStream_t stream = (hipStream_t) nullptr;
  for (int k = 0; k < 2; k++) HIP_TRY(hipEventCreate(&scratch.ev[k]));
  HIP_TRY(hipEventRecord(scratch.ev[0], stream));
  if (n_all > 0) {
    hipLaunchKernelGGL(fo::reads_kernel<>, dim3((unsigned)((n_all + fo::THREADS - 1) / fo::THREADS)),
                       dim3(fo::THREADS), 0, stream, (const fo::ReadsContig *)d_contigs, n_contigs, n_all,
                       bits, seed);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(scratch.ev[1], stream));
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipEventElapsedTime(&g_fold_units_ms, scratch.ev[0], scratch.ev[1]));
  lap("folds: read units");
  const ReadsInput in2 = {nc2, n_reads2.data(), start2.data(), end2.data(), count2.data(), 1,
                          lo2.data(), hi2.data(), bases_counted};
  DenseEncoded enc;
  std::vector<long long> n_bases;
  {
    ReadsPiled piled; /* the coverage buffer lives until the encoding ends */
    if ((st = reads_pileup(in2, piled))) return st;
    for (int k = 0; k < 2; k++) g_reads_ms[k] = piled.ms[k];
    lap("reads: pile-up in all");
    n_bases = piled.n_bases;
    if ((st = dense_encode(nc2, n_bases.data(), piled.coverage.data(), 1, enc))) return st;
  }
  return dense_create_encoded(device, nc2, n_bases.data(), 1, enc, lap, (int)problem_contig.size(),
                              problem_contig.data(), problem_penalty.data(), arena_pieces, out);
}
