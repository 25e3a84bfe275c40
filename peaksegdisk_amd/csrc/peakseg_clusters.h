/* peakseg_clusters.h -- the host side of the peak clusters (kernels: peak_clusters.h): the checks
 * of the groups, the members' layout, the launches, the one download of the groups' cluster counts,
 * the matrix (whose bases, sum and max come from regions_fold of peakseg_regions.h), the download,
 * and the probe that clusters caller-given peak lists. */

namespace {

thread_local float g_clusters_ms = 0.f;

/* the members of a call, group after group, as the kernels read them */
struct ClusterLayout {
  std::vector<long long> member_off; /* members + 1: the first flat peak of each */
  std::vector<int> member_group, member_contig;
  std::vector<int> group_member0;    /* groups + 1 */
  long long peaks() const { return member_off.back(); }
  size_t members() const { return member_group.size(); }
  size_t groups() const { return group_member0.size() - 1; }
};

/* room for the members, groups and peaks of a call, and the layout on the device */
int clusters_room(psd_problem_set *s, ClusterTable &t, const ClusterLayout &lay) {
  namespace rg = psd::regions;
  const long long nm = (long long)lay.members(), ng = (long long)lay.groups(), n = lay.peaks();
  int st = 0;
  if (nm + 1 > t.member_capacity || !t.member_off) {
    const long long have = t.member_capacity, need = nm + 1;
    t.member_capacity = 0;
    if ((st = label_room(s, t.members, have, need)) || (st = label_room(s, t.member_off, have, need)) ||
        (st = label_room(s, t.member_group, have, need)) ||
        (st = label_room(s, t.member_contig, have, need)))
      return st;
    t.member_capacity = need;
  }
  if (ng + 1 > t.group_capacity || !t.group_member0) {
    const long long have = t.group_capacity, need = ng + 1;
    t.group_capacity = 0;
    if ((st = label_room(s, t.group_member0, have, need)) ||
        (st = label_room(s, t.group_clusters, have, need)) ||
        (st = label_room(s, t.entry_off, have, need)) || (st = label_room(s, t.cluster_off, have, need)))
      return st;
    t.group_capacity = need;
  }
  if (n + 1 > t.peak_capacity || !t.peak_start) {
    const long long have = t.peak_capacity, need = n + 1;
    t.peak_capacity = 0;
    if ((st = label_room(s, t.peak_start, have, need)) || (st = label_room(s, t.peak_end, have, need)) ||
        (st = label_room(s, t.lead, have, need)) || (st = label_room(s, t.off, have, need)) ||
        (st = label_room(s, t.block_sum, have ? have / rg::THREADS + 2 : 0, need / rg::THREADS + 2)) ||
        (st = label_room(s, t.cluster_start, have, need)) ||
        (st = label_room(s, t.cluster_end, have, need)) ||
        (st = label_room(s, t.cluster_peaks, have, need)) ||
        (st = label_room(s, t.cluster_samples, have, need)))
      return st;
    t.peak_capacity = need;
  }
  HIP_TRY(hipMemcpy(t.member_off, lay.member_off.data(), sizeof(long long) * (size_t)(nm + 1),
                    hipMemcpyHostToDevice));
  if (nm > 0) {
    HIP_TRY(hipMemcpy(t.member_group, lay.member_group.data(), sizeof(int) * (size_t)nm,
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t.member_contig, lay.member_contig.data(), sizeof(int) * (size_t)nm,
                      hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(t.group_member0, lay.group_member0.data(), sizeof(int) * (size_t)(ng + 1),
                    hipMemcpyHostToDevice));
  return 0;
}

/* The clusters of the peaks in t.peak_start / t.peak_end: mark, scan, assign on `stream`, and the
 * download of the groups' cluster counts into counts[groups].  0 or a status. */
int clusters_find(ClusterTable &t, const ClusterLayout &lay, hipStream_t stream,
                  std::vector<long long> &counts) {
  namespace cl = psd::clusters;
  namespace rg = psd::regions;
  const long long n = lay.peaks(), ng = (long long)lay.groups();
  const int nm = (int)lay.members();
  counts.assign((size_t)ng, 0);
  if (n == 0) return 0;
  /* (a grid dimension times the workgroup size stays below 2^32) */
  if ((n + 1 + cl::THREADS - 1) / cl::THREADS >= (1ll << 24) || ng / cl::THREADS >= (1ll << 24)) {
    set_error("pack_peak_clusters: %lld peaks in %lld groups in one call", n, ng);
    return ERROR_REGION_ARGUMENTS;
  }
  /* (coordinates are not negative: 0x80808080 is below every one of them) */
  HIP_TRY(hipMemsetAsync(t.cluster_end, 0x80, sizeof(int) * (size_t)n, stream));
  HIP_TRY(hipMemsetAsync(t.cluster_start, 0, sizeof(int) * (size_t)n, stream));
  HIP_TRY(hipMemsetAsync(t.cluster_peaks, 0, sizeof(int) * (size_t)n, stream));
  HIP_TRY(hipMemsetAsync(t.cluster_samples, 0, sizeof(int) * (size_t)n, stream));
  const long long nb = (n + 1 + cl::THREADS - 1) / cl::THREADS;
  hipLaunchKernelGGL(cl::mark_kernel, dim3((unsigned)nb), dim3(cl::THREADS), 0, stream,
                     (const long long *)t.member_off, nm, (const int *)t.member_group,
                     (const int *)t.group_member0, n, (const int *)t.peak_start,
                     (const int *)t.peak_end, t.lead, t.off, t.block_sum);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(rg::scan_top_kernel, dim3(1), dim3(rg::THREADS), 0, stream, t.block_sum, nb);
  HIP_TRY(hipGetLastError());
  const long long threads = n > ng ? n : ng;
  hipLaunchKernelGGL(cl::assign_kernel, dim3((unsigned)((threads + cl::THREADS - 1) / cl::THREADS)),
                     dim3(cl::THREADS), 0, stream, (const long long *)t.member_off, nm,
                     (const int *)t.member_group, (const int *)t.group_member0, (int)ng, n,
                     (const int *)t.peak_start, (const int *)t.peak_end, (const int *)t.lead,
                     (const int *)t.off, (const long long *)t.block_sum, t.cluster_start,
                     t.cluster_end, t.cluster_peaks, t.group_clusters);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(counts.data(), t.group_clusters, sizeof(long long) * (size_t)ng,
                         hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return 0;
}

/* the first entry and the first cluster of every group; -> (entries, clusters) */
void clusters_offsets(const ClusterLayout &lay, const std::vector<long long> &counts,
                      std::vector<long long> &entry_off, std::vector<long long> &cluster_off) {
  const size_t ng = lay.groups();
  entry_off.assign(ng + 1, 0);
  cluster_off.assign(ng + 1, 0);
  for (size_t g = 0; g < ng; g++) {
    const long long members = lay.group_member0[g + 1] - lay.group_member0[g];
    entry_off[g + 1] = entry_off[g] + counts[g] * members;
    cluster_off[g + 1] = cluster_off[g] + counts[g];
  }
}

unsigned long long entry_bytes(long long entries) { return (unsigned long long)entries * 16ull; }

/* room for the entries, the offsets on the device, and matrix_kernel on `stream` (not waited for) */
int clusters_matrix(psd_problem_set *s, ClusterTable &t, const ClusterLayout &lay, hipStream_t stream,
                    const std::vector<long long> &entry_off, const std::vector<long long> &cluster_off,
                    bool with_regions) {
  namespace cl = psd::clusters;
  const long long ng = (long long)lay.groups(), entries = entry_off.back();
  int st = 0;
  if (entries > t.entry_capacity || !t.m_peaks) {
    const long long have = t.entry_capacity, need = entries > 0 ? entries : 1;
    t.entry_capacity = 0;
    if ((st = label_room(s, t.m_peaks, have, need)) || (st = label_room(s, t.region_start, have, need)) ||
        (st = label_room(s, t.region_end, have, need)) ||
        (st = label_room(s, t.region_contig, have, need)))
      return st;
    t.entry_capacity = need;
  }
  if (entries == 0) return 0;
  if ((entries + cl::THREADS - 1) / cl::THREADS >= (1ll << 24)) {
    set_error("pack_peak_clusters: %lld entries of the matrix in one call", entries);
    return ERROR_REGION_ARGUMENTS;
  }
  HIP_TRY(hipMemcpy(t.entry_off, entry_off.data(), sizeof(long long) * (size_t)(ng + 1),
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t.cluster_off, cluster_off.data(), sizeof(long long) * (size_t)(ng + 1),
                    hipMemcpyHostToDevice));
  hipLaunchKernelGGL(cl::matrix_kernel, dim3((unsigned)((entries + cl::THREADS - 1) / cl::THREADS)),
                     dim3(cl::THREADS), 0, stream, (const long long *)t.entry_off,
                     (const long long *)t.cluster_off, (int)ng, entries,
                     (const long long *)t.member_off, (const int *)t.group_member0,
                     (const int *)t.member_contig, (const int *)t.peak_start, (const int *)t.peak_end,
                     (const int *)t.cluster_start, (const int *)t.cluster_end, t.cluster_samples,
                     t.m_peaks, with_regions ? t.region_start : nullptr,
                     with_regions ? t.region_end : nullptr, with_regions ? t.region_contig : nullptr);
  HIP_TRY(hipGetLastError());
  return 0;
}

/* 0 or a status; the device is set and the groups have been checked.  *clusters_total: clusters */
int clusters_run(psd_problem_set *s, const int *first_chromStart, int n_groups, const int *group,
                 long long *clusters_out, long long *members_out, long long *clusters_total) {
  namespace cl = psd::clusters;
  namespace rg = psd::regions;
  ClusterTable &t = s->clusters;
  int st = 0;
  /* the members, group after group, in increasing problem index */
  ClusterLayout lay;
  std::vector<cl::Member> members;
  std::vector<std::vector<int>> of_group((size_t)n_groups);
  for (int p = 0; p < s->n_problems; p++)
    if (group[p] >= 0) of_group[(size_t)group[p]].push_back(p);
  lay.member_off.push_back(0);
  lay.group_member0.push_back(0);
  for (int g = 0; g < n_groups; g++) {
    for (int p : of_group[(size_t)g]) {
      const psd::ProbResult &r = s->results[(size_t)p];
      const int c = s->prob_contig[(size_t)p];
      cl::Member m;
      m.seg_from = s->prob_seg_off[(size_t)p];
      m.run0 = s->contig_off[(size_t)c];
      m.n_segments = r.status == 0 ? r.n_segments : 1;
      m.first = first_chromStart ? first_chromStart[c] : 0;
      members.push_back(m);
      lay.member_group.push_back(g);
      lay.member_contig.push_back(c);
      lay.member_off.push_back(lay.member_off.back() + (m.n_segments - 1) / 2);
    }
    lay.group_member0.push_back((int)lay.member_group.size());
    if (members_out) members_out[g] = (long long)of_group[(size_t)g].size();
  }
  const long long n = lay.peaks();
  for (auto &e : t.ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  if ((st = clusters_room(s, t, lay))) return st;
  if (!members.empty())
    HIP_TRY(hipMemcpy(t.members, members.data(), sizeof(cl::Member) * members.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipEventRecord(t.ev[0], s->stream));
  if (n > 0) {
    if ((n + cl::THREADS - 1) / cl::THREADS >= (1ll << 24)) {
      set_error("pack_peak_clusters: %lld peaks in one call", n);
      return ERROR_REGION_ARGUMENTS;
    }
    hipLaunchKernelGGL(cl::gather_kernel, dim3((unsigned)((n + cl::THREADS - 1) / cl::THREADS)),
                       dim3(cl::THREADS), 0, s->stream, (const cl::Member *)t.members,
                       (const long long *)t.member_off, (int)lay.members(), n,
                       (const int *)s->d.seg_start, (const int *)s->d_run_end, t.peak_start, t.peak_end);
    HIP_TRY(hipGetLastError());
  }
  std::vector<long long> counts, entry_off, cluster_off;
  if ((st = clusters_find(t, lay, s->stream, counts))) return st;
  clusters_offsets(lay, counts, entry_off, cluster_off);
  const long long entries = entry_off.back();
  /* does the matrix fit?  asked before anything of it is allocated or written */
  {
    unsigned long long more = regions_room_bytes(s, t.matrix, entries);
    if (entries > t.entry_capacity || !t.m_peaks)
      more += entry_bytes(entries > 0 ? entries : 1) - entry_bytes(t.entry_capacity);
    size_t free_b = 0, total_b = 0;
    const bool known = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    /* (a matrix that needs nothing more fits: the set may hold more than it is allowed by then,
     * through arrays that are not asked about, and still answers the calls it has room for) */
    if ((s->max_bytes && more > 0 && s->bytes + more > s->max_bytes) ||
        (known && more > (unsigned long long)free_b)) {
      set_error("pack_peak_clusters: the matrix of %lld entries needs %llu more bytes, which do not "
                "fit (free HBM / PEAKSEG_HIP_MAX_BYTES)", entries, more);
      return ERROR_DEVICE_MEMORY;
    }
  }
  RegionTable &mt = t.matrix;
  if ((st = regions_room(s, mt, entries))) return st;
  if ((st = clusters_matrix(s, t, lay, s->stream, entry_off, cluster_off, true))) return st;
  if (entries > 0) {
    const std::vector<long long> no_regions((size_t)s->n_contigs + 1, 0);
    const std::vector<const int *> none;
    if ((st = regions_contigs(s, mt, first_chromStart, no_regions, none, none, nullptr))) return st;
    long long most_items = 0;
    for (size_t g = 0; g < lay.groups(); g++) {
      long long tiles = 0;
      for (int m = lay.group_member0[g]; m < lay.group_member0[g + 1]; m++) {
        const size_t c = (size_t)lay.member_contig[(size_t)m];
        tiles += ((s->contig_off[c] & 3) + s->contig_n[c] + rg::TILE - 1) / rg::TILE;
      }
      most_items += counts[g] * tiles;
    }
    if ((st = regions_fold(s, mt, entries, (const int *)t.region_start, (const int *)t.region_end,
                           (const int *)t.region_contig, most_items, false, []() { return 0; })))
      return st;
  }
  HIP_TRY(hipEventRecord(t.ev[1], s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipEventElapsedTime(&g_clusters_ms, t.ev[0], t.ev[1]));
  for (int g = 0; g < n_groups && clusters_out; g++) clusters_out[g] = counts[(size_t)g];
  t.entries = entries;
  *clusters_total = cluster_off.back();
  return 0;
}

}  // namespace

extern "C" long long peakseg_hip_problem_set_pack_peak_clusters(
    psd_problem_set *s, const int *first_chromStart, int n_groups, const int *group,
    long long *clusters_out, long long *members_out, const int **clusterStart_dev,
    const int **clusterEnd_dev, const int **peaks_dev, const int **samples_dev, const int **m_peaks_dev,
    const int **m_bases_dev, const long long **m_sum_dev, const int **m_max_dev) {
  if (!s || !s->solved) return -1;
  if (!s->dense) {
    set_error("pack_peak_clusters: the set was not made from dense counts or reads and has no run_end[]");
    return -1;
  }
  if (hipSetDevice(s->device) != hipSuccess) return -1;
  s->clusters.clusters = s->clusters.entries = -1;
  if (first_chromStart_check(s, first_chromStart, "pack_peak_clusters")) return -1;
  if (n_groups < 0 || (!group && s->n_problems > 0)) {
    set_error("pack_peak_clusters: %d groups%s", n_groups, group ? "" : " and no group array");
    return -ERROR_REGION_ARGUMENTS;
  }
  for (int p = 0; p < s->n_problems; p++)
    if (group[p] < -1 || group[p] >= n_groups) {
      set_error("pack_peak_clusters: problem %d is in group %d, outside -1 .. %d", p, group[p],
                n_groups - 1);
      return -ERROR_REGION_ARGUMENTS;
    }
  long long total = 0;
  const int st = clusters_run(s, first_chromStart, n_groups, group, clusters_out, members_out, &total);
  if (st) return st == ERROR_REGION_ARGUMENTS || st == ERROR_DEVICE_MEMORY ? -st : -1;
  const ClusterTable &t = s->clusters;
  s->clusters.clusters = total;
  if (clusterStart_dev) *clusterStart_dev = t.cluster_start;
  if (clusterEnd_dev) *clusterEnd_dev = t.cluster_end;
  if (peaks_dev) *peaks_dev = t.cluster_peaks;
  if (samples_dev) *samples_dev = t.cluster_samples;
  if (m_peaks_dev) *m_peaks_dev = t.m_peaks;
  if (m_bases_dev) *m_bases_dev = t.matrix.bases;
  if (m_sum_dev) *m_sum_dev = t.matrix.sum;
  if (m_max_dev) *m_max_dev = t.matrix.mx;
  return total;
}

extern "C" int peakseg_hip_problem_set_packed_peak_clusters_download(
    psd_problem_set *s, int *clusterStart_out, int *clusterEnd_out, int *peaks_out, int *samples_out,
    int *m_peaks_out, int *m_bases_out, long long *m_sum_out, int *m_max_out) {
  if (!s || !s->solved || s->clusters.clusters < 0) return -1;
  const ClusterTable &t = s->clusters;
  const size_t k = (size_t)t.clusters, e = (size_t)t.entries;
  const void *from[8] = {t.cluster_start, t.cluster_end, t.cluster_peaks, t.cluster_samples,
                         t.m_peaks, t.matrix.bases, t.matrix.sum, t.matrix.mx};
  void *to[8] = {clusterStart_out, clusterEnd_out, peaks_out, samples_out,
                 m_peaks_out, m_bases_out, m_sum_out, m_max_out};
  const size_t bytes[8] = {k * 4, k * 4, k * 4, k * 4, e * 4, e * 4, e * 8, e * 4};
  for (int j = 0; j < 8; j++)
    if (to[j] && bytes[j] > 0 && hipMemcpy(to[j], from[j], bytes[j], hipMemcpyDeviceToHost) != hipSuccess) {
      set_error("download of the packed peak clusters failed");
      return -1;
    }
  return 0;
}

extern "C" int peakseg_hip_peak_clusters_last_ms(float *ms) {
  if (ms) *ms = g_clusters_ms;
  return 0;
}

extern "C" long long peakseg_hip_peak_clusters_probe(int device, int n_members, const long long *n_peaks,
                                                     const int *const *peak_start,
                                                     const int *const *peak_end, int *clusterStart_out,
                                                     int *clusterEnd_out, int *peaks_out,
                                                     int *samples_out, int *m_peaks_out) {
  if (n_members < 0 || (n_members > 0 && (!n_peaks || !peak_start || !peak_end))) {
    set_error("peak_clusters_probe: %d members, or no arrays", n_members);
    return -ERROR_REGION_ARGUMENTS;
  }
  ClusterLayout lay;
  lay.member_off.push_back(0);
  lay.group_member0.push_back(0);
  std::vector<int> starts, ends;
  for (int m = 0; m < n_members; m++) {
    const long long n = n_peaks[m];
    if (n < 0 || (n > 0 && (!peak_start[m] || !peak_end[m]))) {
      set_error("peak_clusters_probe: member %d has %lld peaks, or no arrays", m, n);
      return -ERROR_REGION_ARGUMENTS;
    }
    for (long long i = 0; i < n; i++) {
      const int ps = peak_start[m][i], pe = peak_end[m][i];
      if (ps < 0 || ps >= pe || (i > 0 && peak_end[m][i - 1] > ps)) {
        set_error("peak_clusters_probe: member %d: peak %lld [%d, %d) is negative, empty, or not "
                  "after the peak before it", m, i, ps, pe);
        return -ERROR_REGION_ARGUMENTS;
      }
      starts.push_back(ps);
      ends.push_back(pe);
    }
    lay.member_group.push_back(0);
    lay.member_contig.push_back(0);
    lay.member_off.push_back(lay.member_off.back() + n);
  }
  lay.group_member0.push_back(n_members);
  if (peakseg_hip_device_count() <= 0) {
    set_error("no HIP device visible (this library has no CPU fallback)");
    return -ERROR_NO_HIP_DEVICE;
  }
  if (hipSetDevice(device) != hipSuccess) return -1;
  /* a set that holds nothing but what this call allocates (on the null stream) */
  std::unique_ptr<psd_problem_set> tmp(new psd_problem_set);
  tmp->device = device;
  ClusterTable &t = tmp->clusters;
  long long total = -1;
  auto run = [&]() -> int {
    int st = clusters_room(tmp.get(), t, lay);
    if (st) return st;
    const size_t n = starts.size();
    if (n > 0) {
      HIP_TRY(hipMemcpy(t.peak_start, starts.data(), sizeof(int) * n, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(t.peak_end, ends.data(), sizeof(int) * n, hipMemcpyHostToDevice));
    }
    std::vector<long long> counts, entry_off, cluster_off;
    if ((st = clusters_find(t, lay, (hipStream_t) nullptr, counts))) return st;
    clusters_offsets(lay, counts, entry_off, cluster_off);
    if ((st = clusters_matrix(tmp.get(), t, lay, (hipStream_t) nullptr, entry_off, cluster_off, false)))
      return st;
    HIP_TRY(hipStreamSynchronize((hipStream_t) nullptr));
    const size_t k = (size_t)cluster_off.back(), e = (size_t)entry_off.back();
    const void *from[5] = {t.cluster_start, t.cluster_end, t.cluster_peaks, t.cluster_samples, t.m_peaks};
    void *to[5] = {clusterStart_out, clusterEnd_out, peaks_out, samples_out, m_peaks_out};
    for (int j = 0; j < 5; j++) {
      const size_t entries = j < 4 ? k : e;
      if (to[j] && entries > 0)
        HIP_TRY(hipMemcpy(to[j], from[j], entries * sizeof(int), hipMemcpyDeviceToHost));
    }
    total = (long long)k;
    return 0;
  };
  const int st = run();
  for (void *q : tmp->allocs) (void)hipFree(q);
  tmp->allocs.clear();
  if (st) return st == ERROR_REGION_ARGUMENTS || st == ERROR_DEVICE_MEMORY ? -st : -1;
  return total;
}
