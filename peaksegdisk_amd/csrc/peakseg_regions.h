/* peakseg_regions.h -- the host side of the coverage of regions (kernels: region_stats.h): the
 * checks of the regions, the descriptors, the three launches, the download.  regions_fold() is what
 * the cluster-by-member matrix of peakseg_clusters.h calls too.  Nothing here reads or writes what
 * a solve leaves: the call works on a set before or after it. */

namespace {

thread_local float g_regions_ms = 0.f;
thread_local long long g_fold_grid = 0; /* workgroups of the calling thread's last fold launch */

void region_error_text(int contig, long long index, long long rs, long long re, bool known) {
  if (known)
    set_error("pack_region_stats: contig %d: region %lld has chromStart %lld >= chromEnd %lld", contig,
              index, rs, re);
  else
    set_error("pack_region_stats: contig %d: region %lld has chromStart >= chromEnd", contig, index);
}

/* the 32-bit check of pack_segments: 0, or -1 with the error text */
int first_chromStart_check(const psd_problem_set *s, const int *first_chromStart, const char *who) {
  for (int c = 0; c < s->n_contigs; c++) {
    const long long first = first_chromStart ? first_chromStart[c] : 0;
    if (first < 0 || first + s->contig_bases[(size_t)c] > 2147483647ll) {
      set_error("%s: contig %d: chromStart %lld + %lld bases is no 32-bit coordinate", who, c, first,
                s->contig_bases[(size_t)c]);
      return -1;
    }
  }
  return 0;
}

/* The three launches over n regions on the set's stream (not waited for).  The regions are those of
 * `contigs` (already on the device, with reg_off) or, flat_contig != NULL, the flat device arrays.
 * with_check: the first launch keeps each contig's first bad region in its (zeroed) check word;
 * then_stop(): called after the first launch; nonzero: a bad region, nothing further is launched
 * and that is returned.  most_items: an upper bound on the (region, tile) items, which sizes the
 * fold's grid (at most eight workgroups per CU; the kernel reads the true number from HBM). */
template <class Stop>
int regions_fold(psd_problem_set *s, RegionTable &t, long long n, const int *flat_start,
                 const int *flat_end, const int *flat_contig, long long most_items, bool with_check,
                 Stop then_stop) {
  namespace rg = psd::regions;
  if (n <= 0) return 0;
  const long long nb = (n + rg::THREADS - 1) / rg::THREADS;
  hipLaunchKernelGGL(rg::locate_kernel, dim3((unsigned)nb), dim3(rg::THREADS), 0, s->stream,
                     (const rg::Contig *)t.d_contigs, (const long long *)t.d_reg_off, s->n_contigs, n,
                     flat_start, flat_end, flat_contig, (const int *)s->d_run_end,
                     (const int *)s->d.count, (const int *)s->d.weight, t.bases, t.sum, t.mx, t.span,
                     t.off, t.block_sum, with_check ? t.d_check : nullptr);
  HIP_TRY(hipGetLastError());
  const int st = then_stop();
  if (st) return st;
  hipLaunchKernelGGL(rg::scan_top_kernel, dim3(1), dim3(rg::THREADS), 0, s->stream, t.block_sum, nb);
  HIP_TRY(hipGetLastError());
  long long grid = 8ll * (s->n_cu > 0 ? s->n_cu : 256);
  if (most_items < grid) grid = most_items > 0 ? most_items : 1;
  g_fold_grid = grid;
  hipLaunchKernelGGL(rg::fold_kernel, dim3((unsigned)grid), dim3(rg::THREADS), 0, s->stream, n,
                     (const int *)t.off, (const long long *)t.block_sum, (const rg::Span *)t.span,
                     (const int *)s->d.count, (const int *)s->d.weight, t.sum, t.mx);
  HIP_TRY(hipGetLastError());
  return 0;
}

/* room for n regions, the contigs' descriptors (first call) and the events */
int regions_room(psd_problem_set *s, RegionTable &t, long long n) {
  namespace rg = psd::regions;
  const size_t nc = (size_t)s->n_contigs;
  int st = 0;
  for (auto &e : t.ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  if ((!t.d_contigs && (st = dev_alloc(s, &t.d_contigs, nc))) ||
      (!t.d_reg_off && (st = dev_alloc(s, &t.d_reg_off, nc + 1))) ||
      (!t.d_check && (st = dev_alloc(s, &t.d_check, nc))))
    return st;
  if (n > t.capacity || !t.bases) {
    const long long need = n > 0 ? n : 1, have = t.capacity;
    const long long nb_have = have / rg::THREADS + 2, nb_need = need / rg::THREADS + 2;
    t.capacity = 0;
    if ((st = label_room(s, t.bases, have, need)) || (st = label_room(s, t.sum, have, need)) ||
        (st = label_room(s, t.mx, have, need)) || (st = label_room(s, t.span, have, need)) ||
        (st = label_room(s, t.off, have, need)) ||
        (st = label_room(s, t.d_regions, 2 * have, 2 * need)) ||
        (st = label_room(s, t.block_sum, have ? nb_have : 0, nb_need)))
      return st;
    t.capacity = need;
  }
  return 0;
}

/* the bytes regions_room(s, t, n) would add to what the set holds */
unsigned long long regions_room_bytes(const psd_problem_set *s, const RegionTable &t, long long n) {
  namespace rg = psd::regions;
  const unsigned long long nc = (unsigned long long)s->n_contigs;
  auto columns = [](long long m) {
    return (unsigned long long)m * (4 + 8 + 4 + sizeof(rg::Span) + 4 + 2 * 4) +
           (unsigned long long)(m / rg::THREADS + 2) * 8;
  };
  unsigned long long more = 0;
  if (!t.d_contigs) more += (nc ? nc : 1) * sizeof(rg::Contig) + (nc + 1) * 8 + (nc ? nc : 1) * 8;
  if (n > t.capacity || !t.bases)
    more += columns(n > 0 ? n : 1) - (t.capacity > 0 ? columns(t.capacity) : 0ull);
  return more;
}

/* the contigs' descriptors of a call; start / end: per contig device addresses or NULL */
int regions_contigs(psd_problem_set *s, RegionTable &t, const int *first_chromStart,
                    const std::vector<long long> &reg_off, const std::vector<const int *> &start,
                    const std::vector<const int *> &end, long long *most_items) {
  namespace rg = psd::regions;
  const size_t nc = (size_t)s->n_contigs;
  std::vector<rg::Contig> contigs(nc);
  long long most = 0;
  for (size_t c = 0; c < nc; c++) {
    rg::Contig &k = contigs[c];
    k.start = (const gint *)(start.empty() ? nullptr : start[c]);
    k.end = (const gint *)(end.empty() ? nullptr : end[c]);
    k.reg0 = reg_off[c];
    k.run0 = s->contig_off[c];
    k.n_runs = s->contig_n[c];
    k.first = first_chromStart ? first_chromStart[c] : 0;
    k.bases = s->contig_bases[c];
    const long long tiles = ((k.run0 & 3) + k.n_runs + rg::TILE - 1) / rg::TILE;
    most += (reg_off[c + 1] - reg_off[c]) * tiles;
  }
  if (most_items) *most_items = most;
  HIP_TRY(hipMemcpy(t.d_contigs, contigs.data(), sizeof(rg::Contig) * nc, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t.d_reg_off, reg_off.data(), sizeof(long long) * (nc + 1), hipMemcpyHostToDevice));
  return 0;
}

/* 0 or a status; the device is set and the arguments' shape has been checked */
int regions_run(psd_problem_set *s, const int *first_chromStart, const long long *n_regions,
                const int *const *region_start, const int *const *region_end, int on_device,
                long long *rows_out, long long *total_out) {
  namespace rg = psd::regions;
  RegionTable &t = s->regions;
  const size_t nc = (size_t)s->n_contigs;
  int st = 0;
  std::vector<long long> reg_off(nc + 1, 0);
  for (size_t c = 0; c < nc; c++) {
    reg_off[c + 1] = reg_off[c] + n_regions[c];
    if (rows_out) rows_out[c] = n_regions[c];
  }
  const long long n = reg_off[nc];
  /* (a grid dimension times the workgroup size stays below 2^32) */
  if ((n + rg::THREADS - 1) / rg::THREADS >= (1ll << 24)) {
    set_error("pack_region_stats: %lld regions in one call", n);
    return ERROR_REGION_ARGUMENTS;
  }
  /* host arrays are checked here, before anything is allocated (locate_kernel checks what the host
   * cannot see) */
  for (size_t c = 0; c < nc && !on_device; c++)
    for (long long i = 0; i < n_regions[c]; i++)
      if (region_start[c][i] >= region_end[c][i]) {
        region_error_text((int)c, i, region_start[c][i], region_end[c][i], true);
        return ERROR_REGION_ARGUMENTS;
      }
  if ((st = regions_room(s, t, n))) return st;
  std::vector<const int *> start(nc, nullptr), end(nc, nullptr);
  std::vector<int> host_copy;
  if (!on_device) host_copy.resize((size_t)(2 * n));
  for (size_t c = 0; c < nc; c++) {
    const long long m = n_regions[c], at = reg_off[c];
    if (m == 0) continue;
    if (on_device) {
      start[c] = region_start[c];
      end[c] = region_end[c];
      continue;
    }
    memcpy(host_copy.data() + at, region_start[c], sizeof(int) * (size_t)m);
    memcpy(host_copy.data() + n + at, region_end[c], sizeof(int) * (size_t)m);
    start[c] = t.d_regions + at;
    end[c] = t.d_regions + n + at;
  }
  long long most_items = 0;
  if ((st = regions_contigs(s, t, first_chromStart, reg_off, start, end, &most_items))) return st;
  if (!on_device && n > 0)
    HIP_TRY(hipMemcpy(t.d_regions, host_copy.data(), sizeof(int) * host_copy.size(), hipMemcpyHostToDevice));
  /* (device arrays: what the caller queued on the null stream -- torch's default -- has run) */
  if (on_device) HIP_TRY(hipStreamSynchronize((hipStream_t) nullptr));
  HIP_TRY(hipEventRecord(t.ev[0], s->stream));
  if (on_device) HIP_TRY(hipMemsetAsync(t.d_check, 0, sizeof(unsigned long long) * nc, s->stream));
  st = regions_fold(s, t, n, nullptr, nullptr, nullptr, most_items, on_device != 0, [&]() -> int {
    if (!on_device) return 0; /* nothing further is launched after a bad region */
    std::vector<unsigned long long> check(nc);
    HIP_TRY(hipMemcpyAsync(check.data(), t.d_check, sizeof(unsigned long long) * nc,
                           hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (size_t c = 0; c < nc; c++)
      if (check[c]) {
        region_error_text((int)c, (long long)~check[c], 0, 0, false);
        return ERROR_REGION_ARGUMENTS;
      }
    return 0;
  });
  if (st) return st;
  HIP_TRY(hipEventRecord(t.ev[1], s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipEventElapsedTime(&g_regions_ms, t.ev[0], t.ev[1]));
  *total_out = n;
  return 0;
}

}  // namespace

extern "C" long long peakseg_hip_problem_set_pack_region_stats(
    psd_problem_set *s, const int *first_chromStart, const long long *n_regions,
    const int *const *region_start, const int *const *region_end, int regions_on_device,
    long long *rows_out, const int **bases_dev, const long long **sum_dev, const int **max_dev) {
  if (!s) return -1;
  if (!s->dense) {
    set_error("pack_region_stats: the set was not made from dense counts or reads and has no run_end[]");
    return -1;
  }
  if (hipSetDevice(s->device) != hipSuccess) return -1;
  s->regions.total = -1;
  if (first_chromStart_check(s, first_chromStart, "pack_region_stats")) return -1;
  if (!n_regions) {
    set_error("pack_region_stats: no region counts");
    return -ERROR_REGION_ARGUMENTS;
  }
  for (int c = 0; c < s->n_contigs; c++) {
    if (n_regions[c] < 0) {
      set_error("pack_region_stats: contig %d has %lld regions", c, n_regions[c]);
      return -ERROR_REGION_ARGUMENTS;
    }
    if (n_regions[c] == 0) continue;
    const int *const *arrays[2] = {region_start, region_end};
    for (int j = 0; j < 2; j++) {
      const int *a = arrays[j] ? arrays[j][c] : nullptr;
      if (!a || (regions_on_device && ((unsigned long long)a & 3ull))) {
        set_error("pack_region_stats: contig %d: the %s array is %s", c, LABEL_WHAT[j],
                  a ? "at a device address that is no multiple of 4" : "NULL");
        return -ERROR_REGION_ARGUMENTS;
      }
    }
  }
  long long total = 0;
  const int st = regions_run(s, first_chromStart, n_regions, region_start, region_end,
                             regions_on_device, rows_out, &total);
  if (st) return st == ERROR_REGION_ARGUMENTS ? -ERROR_REGION_ARGUMENTS : -1;
  s->regions.total = total;
  if (bases_dev) *bases_dev = s->regions.bases;
  if (sum_dev) *sum_dev = s->regions.sum;
  if (max_dev) *max_dev = s->regions.mx;
  return total;
}

extern "C" int peakseg_hip_problem_set_packed_region_stats_download(psd_problem_set *s, int *bases_out,
                                                                    long long *sum_out, int *max_out) {
  if (!s || s->regions.total < 0) return -1;
  const size_t n = (size_t)s->regions.total;
  const RegionTable &t = s->regions;
  const void *from[3] = {t.bases, t.sum, t.mx};
  void *to[3] = {bases_out, sum_out, max_out};
  const size_t width[3] = {4, 8, 4};
  for (int k = 0; k < 3 && n > 0; k++)
    if (to[k] && hipMemcpy(to[k], from[k], n * width[k], hipMemcpyDeviceToHost) != hipSuccess) {
      set_error("download of the packed region statistics failed");
      return -1;
    }
  return 0;
}

extern "C" int peakseg_hip_region_stats_tile_runs(void) { return psd::regions::TILE; }

extern "C" long long peakseg_hip_region_stats_last_fold_grid(void) { return g_fold_grid; }

extern "C" int peakseg_hip_region_stats_last_ms(float *ms) {
  if (ms) *ms = g_regions_ms;
  return 0;
}
