/* peakseg_features.h -- the host side of the coverage statistics (kernels: coverage_stats.h): the
 * checks of the ranks, the tiles and descriptors, the launches between two events, the download.
 * Nothing here reads or writes what a solve leaves: the call works on a set before or after it. */

namespace {

thread_local float g_features_ms = 0.f;
thread_local int g_features_passes = 0;

/* the digit passes a set needs: the 8-bit digits up to the highest one that is not zero everywhere */
int feature_passes(const psd_problem_set *s) {
  int largest = 0;
  for (int m : s->contig_max) largest = m > largest ? m : largest;
  int passes = 1;
  while (passes < 4 && ((unsigned)largest >> (8 * passes))) passes++;
  return passes;
}

/* the tiles over each contig's 16-byte aligned range and the contigs' descriptors: first call only */
int features_geometry(psd_problem_set *s) {
  namespace cv = psd::cover;
  FeatureTable &t = s->features;
  if (t.n_tiles >= 0) return 0;
  const size_t nc = (size_t)s->n_contigs;
  std::vector<long long> desc(nc * cv::DESC, 0);
  std::vector<int> tile_contig;
  long long n_tiles = 0;
  for (size_t c = 0; c < nc; c++) {
    const long long lead = s->contig_off[c] & 3, runs = s->contig_n[c];
    const long long tiles = runs > 0 ? (lead + runs + cv::TILE - 1) / cv::TILE : 0;
    long long *d = desc.data() + c * cv::DESC;
    d[cv::D_RUN0] = s->contig_off[c];
    d[cv::D_RUNS] = runs;
    d[cv::D_TILE0] = n_tiles;
    n_tiles += tiles;
    /* (a grid dimension times the workgroup size stays below 2^32) */
    if (n_tiles >= (1ll << 24)) {
      set_error("pack_coverage_stats: 2^24 or more tiles of %d runs in one call", cv::TILE);
      return ERROR_DENSE_ARGUMENTS;
    }
    tile_contig.insert(tile_contig.end(), (size_t)tiles, (int)c);
  }
  int st = 0;
  if ((st = dev_alloc(s, &t.d_desc, desc.size())) ||
      (st = dev_alloc(s, &t.d_tile_contig, tile_contig.size())) ||
      (st = dev_alloc(s, &t.moments, nc * cv::MOMENTS)))
    return st;
  HIP_TRY(hipMemcpy(t.d_desc, desc.data(), desc.size() * sizeof(long long), hipMemcpyHostToDevice));
  if (!tile_contig.empty())
    HIP_TRY(hipMemcpy(t.d_tile_contig, tile_contig.data(), tile_contig.size() * sizeof(int),
                      hipMemcpyHostToDevice));
  for (auto &e : t.ev) HIP_TRY(hipEventCreate(&e));
  t.n_tiles = n_tiles;
  return 0;
}

/* 0 or a status; the device is set and the ranks have been checked */
int features_run(psd_problem_set *s, int n_ranks, const long long *ranks) {
  namespace cv = psd::cover;
  FeatureTable &t = s->features;
  const size_t nc = (size_t)s->n_contigs;
  const long long entries = (long long)nc * n_ranks;
  int st = features_geometry(s);
  if (st) return st;
  if (entries > t.rank_capacity || !t.value) {
    const long long have = t.rank_capacity, need = entries > 0 ? entries : 1;
    t.rank_capacity = 0;
    if ((st = label_room(s, t.prefix, have, need)) || (st = label_room(s, t.leader, have, need)) ||
        (st = label_room(s, t.value, have, need)) || (st = label_room(s, t.resid, have, need)) ||
        (st = label_room(s, t.hist, have * cv::BINS, need * cv::BINS)))
      return st;
    t.rank_capacity = need;
  }
  const int passes = n_ranks > 0 ? feature_passes(s) : 0;
  if (entries > 0)
    HIP_TRY(hipMemcpy(t.resid, ranks, sizeof(long long) * (size_t)entries, hipMemcpyHostToDevice));
  HIP_TRY(hipEventRecord(t.ev[0], s->stream));
  HIP_TRY(hipMemsetAsync(t.moments, 0, sizeof(unsigned long long) * nc * cv::MOMENTS, s->stream));
  if (t.n_tiles > 0) {
    hipLaunchKernelGGL(cv::moments_kernel, dim3((unsigned)t.n_tiles), dim3(cv::THREADS), 0, s->stream,
                       (const long long *)t.d_desc, (const int *)t.d_tile_contig,
                       (const int *)s->d.count, (const int *)s->d.weight, t.moments);
    HIP_TRY(hipGetLastError());
  }
  if (entries > 0) {
    HIP_TRY(hipMemsetAsync(t.prefix, 0, sizeof(int) * (size_t)entries, s->stream));
    HIP_TRY(hipMemsetAsync(t.leader, 0, sizeof(int) * (size_t)entries, s->stream));
  }
  for (int pass = 0; pass < passes && entries > 0; pass++) {
    const int shift = 8 * (passes - 1 - pass);
    /* (every rank's leader is rank 0 in the first pass: one plane of the histograms) */
    HIP_TRY(hipMemsetAsync(t.hist, 0,
                           sizeof(unsigned long long) * (pass == 0 ? nc : (size_t)entries) * cv::BINS,
                           s->stream));
    if (t.n_tiles > 0) {
      hipLaunchKernelGGL(cv::hist_kernel, dim3((unsigned)t.n_tiles), dim3(cv::THREADS), 0, s->stream,
                         (const long long *)t.d_desc, (const int *)t.d_tile_contig,
                         (const int *)s->d.count, (const int *)s->d.weight, s->n_contigs, n_ranks, shift,
                         (const int *)t.prefix, (const int *)t.leader, t.hist);
      HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(cv::pick_kernel, dim3((unsigned)nc), dim3(psd::WAVE), 0, s->stream, n_ranks, shift,
                       (const unsigned long long *)t.hist, t.prefix, t.resid, t.leader, t.value);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(t.ev[1], s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipEventElapsedTime(&g_features_ms, t.ev[0], t.ev[1]));
  g_features_passes = passes;
  return 0;
}

}  // namespace

extern "C" long long peakseg_hip_problem_set_pack_coverage_stats(psd_problem_set *s, int n_ranks,
                                                                 const long long *ranks,
                                                                 const int **value_dev,
                                                                 const unsigned long long **moments_dev) {
  if (!s) return -1;
  if (!s->dense) {
    set_error("pack_coverage_stats: the set was not made from dense counts or reads: its bins are "
              "not the runs of a per-base coverage");
    return -1;
  }
  if (hipSetDevice(s->device) != hipSuccess) return -1;
  s->features.total = -1;
  g_features_passes = 0;
  if (n_ranks < 0 || n_ranks > psd::cover::MAX_RANKS || (n_ranks > 0 && !ranks)) {
    set_error("pack_coverage_stats: %d ranks per contig (0 to %d, and their array)", n_ranks,
              psd::cover::MAX_RANKS);
    return -ERROR_FEATURE_ARGUMENTS;
  }
  if ((long long)s->n_contigs >= (1ll << 24)) {
    set_error("pack_coverage_stats: 2^24 or more contigs in one call");
    return -1;
  }
  for (int c = 0; c < s->n_contigs; c++)
    for (int k = 0; k < n_ranks; k++) {
      const long long r = ranks[(size_t)c * (size_t)n_ranks + (size_t)k];
      if (r < 0 || r >= s->contig_bases[(size_t)c]) {
        set_error("pack_coverage_stats: contig %d: rank %lld is outside 0 .. %lld (its bases - 1)", c, r,
                  s->contig_bases[(size_t)c] - 1);
        return -ERROR_FEATURE_ARGUMENTS;
      }
    }
  if (features_run(s, n_ranks, ranks)) return -1;
  s->features.total = (long long)s->n_contigs * n_ranks;
  if (value_dev) *value_dev = s->features.value;
  if (moments_dev) *moments_dev = s->features.moments;
  return s->features.total;
}

extern "C" int peakseg_hip_problem_set_packed_coverage_stats_download(psd_problem_set *s, int *value_out,
                                                                      unsigned long long *moments_out) {
  if (!s || s->features.total < 0) return -1;
  const FeatureTable &t = s->features;
  if ((value_out && t.total > 0 &&
       hipMemcpy(value_out, t.value, sizeof(int) * (size_t)t.total, hipMemcpyDeviceToHost) != hipSuccess) ||
      (moments_out &&
       hipMemcpy(moments_out, t.moments,
                 sizeof(unsigned long long) * (size_t)s->n_contigs * psd::cover::MOMENTS,
                 hipMemcpyDeviceToHost) != hipSuccess)) {
    set_error("download of the packed coverage statistics failed");
    return -1;
  }
  return 0;
}

extern "C" int peakseg_hip_coverage_stats_tile_runs(void) { return psd::cover::TILE; }
extern "C" int peakseg_hip_coverage_stats_max_ranks(void) { return psd::cover::MAX_RANKS; }

extern "C" int peakseg_hip_coverage_stats_last_ms(float *ms) {
  if (ms) *ms = g_features_ms;
  return 0;
}

extern "C" int peakseg_hip_coverage_stats_last_passes(int *digit_passes) {
  if (digit_passes) *digit_passes = g_features_passes;
  return 0;
}
