/* peakseg_joint.h -- the host side of the joint peaks (kernels: joint_peaks.h): the checks of the
 * penalty, the groups and the windows, the members' layout and the groups' common extents, the
 * room, the launches level by level (whose folds are regions_fold of peakseg_regions.h), the one
 * download of the head, and the download of the columns.  With no windows given the clusters of
 * peakseg_clusters.h are the windows.  joint_check_groups() and joint_run() also serve the path of many
 * penalties (peakseg_joint_path.h; kernels: joint_path.h), which has a table of its own. */

namespace {

thread_local float g_joint_ms = 0.f, g_joint_path_ms = 0.f;

/* the path's launches after its setup (peakseg_joint_path.h) */
int joint_path_launches(psd_problem_set *s, JointTable &t, const psd::joint::Groups &groups,
                        const psd::joint::Windows &win, int n_groups, long long windows,
                        long long entries, int n_pen, const double *penalties, int max_levels,
                        long long most_items, long long most_items_path);

/* bytes of the call's tables by what they are counted in */
constexpr unsigned long long JOINT_GROUP_BYTES = 4 + 4 * 8 + 2 * 8, JOINT_MEMBER_BYTES = 4,
                             JOINT_WINDOW_BYTES = 2 * 4 + 8 * 4 + 8,
                             JOINT_ENTRY_BYTES = 8 + 8 + 4 + 4 + 8, JOINT_REGION_BYTES = 3 * 4;

/* the bytes joint_room() would add to what the set holds; windows, entries: rows (of every
 * penalty); regions: those of the level with most; carry: doubles (the path's level 0) */
unsigned long long joint_room_bytes(const psd_problem_set *s, const JointTable &t, long long groups,
                                    long long members, long long windows, long long entries,
                                    long long regions, long long carry) {
  auto grow = [](long long have, long long need, unsigned long long each) {
    return need > have ? (unsigned long long)(need - have) * each : 0ull;
  };
  unsigned long long more = regions_room_bytes(s, t.fold, regions);
  more += grow(t.group_capacity, groups + 1, JOINT_GROUP_BYTES);
  more += grow(t.member_capacity, members > 0 ? members : 1, JOINT_MEMBER_BYTES);
  more += grow(t.window_capacity, windows > 0 ? windows : 1, JOINT_WINDOW_BYTES);
  more += grow(t.entry_capacity, entries > 0 ? entries : 1, JOINT_ENTRY_BYTES);
  more += grow(t.region_capacity, regions > 0 ? regions : 1, JOINT_REGION_BYTES);
  more += grow(t.carry_capacity, carry, 8);
  if (!t.head) more += sizeof(psd::joint::Head);
  return more;
}

int joint_room(psd_problem_set *s, JointTable &t, long long groups, long long members,
               long long windows, long long entries, long long regions, long long carry) {
  int st = 0;
  for (auto &e : t.ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  if (!t.head && (st = dev_alloc(s, &t.head, 1))) return st;
  if (groups + 1 > t.group_capacity) {
    const long long have = t.group_capacity, need = groups + 1;
    t.group_capacity = 0;
    if ((st = label_room(s, t.member0, have, need)) || (st = label_room(s, t.win_off, have, need)) ||
        (st = label_room(s, t.entry_off, have, need)) || (st = label_room(s, t.lo, have, need)) ||
        (st = label_room(s, t.hi, have, need)) || (st = label_room(s, t.g_start, have, need)) ||
        (st = label_room(s, t.g_end, have, need)))
      return st;
    t.group_capacity = need;
  }
  if (members > t.member_capacity || !t.member_contig) {
    const long long have = t.member_capacity, need = members > 0 ? members : 1;
    t.member_capacity = 0;
    if ((st = label_room(s, t.member_contig, have, need))) return st;
    t.member_capacity = need;
  }
  if (windows > t.window_capacity || !t.ws) {
    const long long have = t.window_capacity, need = windows > 0 ? windows : 1;
    t.window_capacity = 0;
    if ((st = label_room(s, t.d_windows, 2 * have, 2 * need)) ||
        (st = label_room(s, t.w_group, have, need)) || (st = label_room(s, t.ws, have, need)) ||
        (st = label_room(s, t.we, have, need)) || (st = label_room(s, t.b, have, need)) ||
        (st = label_room(s, t.s, have, need)) || (st = label_room(s, t.e, have, need)) ||
        (st = label_room(s, t.levels, have, need)) || (st = label_room(s, t.samples_up, have, need)) ||
        (st = label_room(s, t.objective, have, need)))
      return st;
    t.window_capacity = need;
  }
  if (entries > t.entry_capacity || !t.total) {
    const long long have = t.entry_capacity, need = entries > 0 ? entries : 1;
    t.entry_capacity = 0;
    if ((st = label_room(s, t.total, have, need)) || (st = label_room(s, t.m_gain, have, need)) ||
        (st = label_room(s, t.m_up, have, need)) || (st = label_room(s, t.m_bases, have, need)) ||
        (st = label_room(s, t.m_sum, have, need)))
      return st;
    t.entry_capacity = need;
  }
  if (regions > t.region_capacity || !t.region_start) {
    const long long have = t.region_capacity, need = regions > 0 ? regions : 1;
    t.region_capacity = 0;
    if ((st = label_room(s, t.region_start, have, need)) ||
        (st = label_room(s, t.region_end, have, need)) ||
        (st = label_room(s, t.region_contig, have, need)))
      return st;
    t.region_capacity = need;
  }
  if (carry > t.carry_capacity) {
    const long long have = t.carry_capacity;
    t.carry_capacity = 0;
    if ((st = label_room(s, t.carry, have, carry))) return st;
    t.carry_capacity = carry;
  }
  return regions_room(s, t.fold, regions);
}

/* 0 or a status; the device is set, the groups and the shape of the windows have been checked.
 * n_windows == NULL: the clusters are the windows.  n_pen == 0: joint_peaks.h's kernels at
 * `penalty`, into t = s->joint; n_pen >= 1: joint_path.h's at penalties[0 .. n_pen), into
 * t = s->joint_path, every column penalty-major.  who: the call, for the messages. */
int joint_run(psd_problem_set *s, JointTable &t, const char *who, const int *first_chromStart,
              int n_groups, const int *group, double penalty, int n_pen, const double *penalties,
              const long long *n_windows, const int *const *window_start,
              const int *const *window_end, int on_device, long long *windows_out,
              long long *members_out, long long *windows_total) {
  namespace jn = psd::joint;
  namespace jp = psd::joint_path;
  namespace rg = psd::regions;
  const long long reps = n_pen > 0 ? n_pen : 1;
  const size_t ng = (size_t)n_groups;
  int st = 0;
  /* the members, group after group, in increasing problem index, and the groups' common extents */
  std::vector<int> member0(ng + 1, 0), member_contig;
  std::vector<long long> lo(ng + 1, 0), hi(ng + 1, -1);
  std::vector<std::vector<int>> of_group(ng);
  if (n_pen > 0) t.problem_member.assign((size_t)s->n_problems, 0);
  for (int p = 0; p < s->n_problems; p++)
    if (group[p] >= 0) {
      if (n_pen > 0) t.problem_member[(size_t)p] = (int)of_group[(size_t)group[p]].size();
      of_group[(size_t)group[p]].push_back(p);
    }
  for (size_t g = 0; g < ng; g++) {
    bool any = false;
    for (int p : of_group[g]) {
      const size_t c = (size_t)s->prob_contig[(size_t)p];
      const long long first = first_chromStart ? first_chromStart[c] : 0;
      const long long last = first + s->contig_bases[c];
      lo[g] = any && lo[g] > first ? lo[g] : first;
      hi[g] = any && hi[g] < last ? hi[g] : last;
      any = true;
      member_contig.push_back((int)c);
    }
    member0[g + 1] = (int)member_contig.size();
    if (members_out) members_out[g] = (long long)of_group[g].size();
  }
  /* the windows */
  std::vector<long long> counts(ng, 0);
  std::vector<const int *> g_start(ng + 1, nullptr), g_end(ng + 1, nullptr);
  if (!n_windows) {
    long long total = 0;
    s->clusters.clusters = s->clusters.entries = -1;
    if ((st = clusters_run(s, first_chromStart, n_groups, group, counts.data(), nullptr, &total)))
      return st;
    s->clusters.clusters = total;
    long long at = 0;
    for (size_t g = 0; g < ng; g++) {
      g_start[g] = s->clusters.cluster_start + at;
      g_end[g] = s->clusters.cluster_end + at;
      at += counts[g];
    }
  } else {
    for (size_t g = 0; g < ng; g++) counts[g] = n_windows[g];
  }
  std::vector<long long> win_off(ng + 1, 0), entry_off(ng + 1, 0);
  for (size_t g = 0; g < ng; g++) {
    win_off[g + 1] = win_off[g] + counts[g];
    entry_off[g + 1] = entry_off[g] + counts[g] * (member0[g + 1] - member0[g]);
    if (windows_out) windows_out[g] = counts[g];
  }
  const long long windows = win_off[ng], entries = entry_off[ng];
  const long long members = (long long)member_contig.size();
  /* (a grid dimension times the workgroup size stays below 2^32; a workgroup per window) */
  const long long most_slots = reps * jn::REFINE > jn::BINS ? reps * jn::REFINE : jn::BINS;
  int most_members = 0;
  for (size_t g = 0; g < ng; g++)
    if (counts[g] > 0 && member0[g + 1] - member0[g] > most_members) most_members = member0[g + 1] - member0[g];
  /* (level 0 of the path: groups of more than a slab of members keep their sums between slabs) */
  int pen_t = 1;
  while (pen_t < n_pen) pen_t <<= 1;
  const long long carry = n_pen > 0 && most_members > jn::SLAB ? windows * pen_t * jn::MAX_CAND : 0;
  if ((entries * most_slots + jn::THREADS - 1) / jn::THREADS >= (1ll << 24) || windows >= (1ll << 31) ||
      (windows * reps + jn::THREADS - 1) / jn::THREADS >= (1ll << 24)) {
    set_error("%s: %lld windows and %lld entries of the matrix in one call", who, windows, entries);
    return ERROR_REGION_ARGUMENTS;
  }
  /* given windows in host arrays are checked here, before anything is allocated (setup_kernel
   * checks what the host cannot see) */
  for (size_t g = 0; g < ng && n_windows && !on_device; g++)
    for (long long i = 0; i < counts[g]; i++)
      if (window_start[g][i] >= window_end[g][i]) {
        set_error("%s: group %d: window %lld has start %d >= end %d", who, (int)g, i,
                  window_start[g][i], window_end[g][i]);
        return ERROR_REGION_ARGUMENTS;
      }
  /* does it fit?  asked before anything of it is allocated or written */
  {
    const unsigned long long more = joint_room_bytes(s, t, n_groups, members, windows * reps,
                                                     entries * reps, entries * most_slots, carry);
    size_t free_b = 0, total_b = 0;
    const bool known = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    /* (a call that needs nothing more fits, whatever other services' arrays have grown to) */
    if ((s->max_bytes && more > 0 && s->bytes + more > s->max_bytes) ||
        (known && more > (unsigned long long)free_b)) {
      set_error("%s: the tables of %lld windows and %lld entries need %llu more bytes, "
                "which do not fit (free HBM / PEAKSEG_HIP_MAX_BYTES)", who, windows * reps,
                entries * reps, more);
      return ERROR_DEVICE_MEMORY;
    }
  }
  if ((st = joint_room(s, t, n_groups, members, windows * reps, entries * reps, entries * most_slots,
                       carry)))
    return st;
  /* given windows: where the caller has them, or the library's copy of host arrays */
  if (n_windows) {
    std::vector<int> host_copy;
    if (!on_device) host_copy.resize((size_t)(2 * windows));
    for (size_t g = 0; g < ng; g++) {
      const long long m = counts[g], at = win_off[g];
      if (m == 0) continue;
      if (on_device) {
        g_start[g] = window_start[g];
        g_end[g] = window_end[g];
        continue;
      }
      memcpy(host_copy.data() + at, window_start[g], sizeof(int) * (size_t)m);
      memcpy(host_copy.data() + windows + at, window_end[g], sizeof(int) * (size_t)m);
      g_start[g] = t.d_windows + at;
      g_end[g] = t.d_windows + windows + at;
    }
    if (!on_device && windows > 0)
      HIP_TRY(hipMemcpy(t.d_windows, host_copy.data(), sizeof(int) * host_copy.size(), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(t.member0, member0.data(), sizeof(int) * (ng + 1), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t.win_off, win_off.data(), sizeof(long long) * (ng + 1), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t.entry_off, entry_off.data(), sizeof(long long) * (ng + 1), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t.lo, lo.data(), sizeof(long long) * (ng + 1), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t.hi, hi.data(), sizeof(long long) * (ng + 1), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t.g_start, g_start.data(), sizeof(const int *) * (ng + 1), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t.g_end, g_end.data(), sizeof(const int *) * (ng + 1), hipMemcpyHostToDevice));
  if (members > 0)
    HIP_TRY(hipMemcpy(t.member_contig, member_contig.data(), sizeof(int) * (size_t)members,
                      hipMemcpyHostToDevice));
  float &ms = n_pen > 0 ? g_joint_path_ms : g_joint_ms;
  ms = 0.f;
  *windows_total = windows;
  t.entries = entries;
  if (windows == 0) return 0;
  RegionTable &ft = t.fold;
  {
    const std::vector<long long> no_regions((size_t)s->n_contigs + 1, 0);
    const std::vector<const int *> none;
    if ((st = regions_contigs(s, ft, first_chromStart, no_regions, none, none, nullptr))) return st;
  }
  /* an upper bound on the (region, tile) items of a level: a member's window meets at most its
   * contig's tiles, and its pieces share at most one tile with each neighbour */
  long long most_items = 0;
  for (size_t g = 0; g < ng; g++) {
    long long tiles = 0;
    for (int m = member0[g]; m < member0[g + 1]; m++) {
      const size_t c = (size_t)member_contig[(size_t)m];
      tiles += ((s->contig_off[c] & 3) + s->contig_n[c] + rg::TILE - 1) / rg::TILE + jn::BINS;
    }
    most_items += counts[g] * tiles;
  }
  const long long most_items_path = most_items * reps; /* (a piece per penalty) */
  jn::Groups groups;
  groups.member0 = t.member0;
  groups.win_off = t.win_off;
  groups.entry_off = t.entry_off;
  groups.lo = t.lo;
  groups.hi = t.hi;
  groups.start = (const gint *const *)(const void *)t.g_start;
  groups.end = (const gint *const *)(const void *)t.g_end;
  jn::Windows win;
  win.group = t.w_group;
  win.ws = t.ws;
  win.we = t.we;
  win.b = t.b;
  win.s = t.s;
  win.e = t.e;
  win.levels = t.levels;
  win.samples_up = t.samples_up;
  win.objective = t.objective;
  /* (device arrays: what the caller queued on the null stream -- torch's default -- has run) */
  if (on_device) HIP_TRY(hipStreamSynchronize((hipStream_t) nullptr));
  HIP_TRY(hipEventRecord(t.ev[0], s->stream));
  HIP_TRY(hipMemsetAsync(t.head, 0, sizeof(jn::Head), s->stream));
  if (n_pen > 0)
    hipLaunchKernelGGL(jp::setup_kernel<>,
                       dim3((unsigned)((windows * reps + jn::THREADS - 1) / jn::THREADS)),
                       dim3(jn::THREADS), 0, s->stream, groups, n_groups, windows, n_pen,
                       n_windows ? 0 : 1, win, t.head);
  else
    hipLaunchKernelGGL(jn::setup_kernel, dim3((unsigned)((windows + jn::THREADS - 1) / jn::THREADS)),
                       dim3(jn::THREADS), 0, s->stream, groups, n_groups, windows, n_windows ? 0 : 1,
                       win, t.head);
  HIP_TRY(hipGetLastError());
  jn::Head head;
  HIP_TRY(hipMemcpyAsync(&head, t.head, sizeof head, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (head.check) { /* nothing further is launched after a bad window */
    const long long w = (long long)~head.check;
    size_t g = 0;
    while (g + 1 < ng && win_off[g + 1] <= w) g++;
    set_error("%s: group %d: window %lld has start >= end", who, (int)g, w - win_off[g]);
    return ERROR_REGION_ARGUMENTS;
  }
  if (n_pen > 0) {
    if ((st = joint_path_launches(s, t, groups, win, n_groups, windows, entries, n_pen, penalties,
                                  head.max_levels, most_items, most_items_path)))
      return st;
    HIP_TRY(hipEventRecord(t.ev[1], s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipEventElapsedTime(&ms, t.ev[0], t.ev[1]));
    return 0;
  }
  auto pass = [&](int slots) -> int {
    const long long n = entries * slots;
    if (n == 0) return 0;
    hipLaunchKernelGGL(jn::bins_kernel, dim3((unsigned)((n + jn::THREADS - 1) / jn::THREADS)),
                       dim3(jn::THREADS), 0, s->stream, groups, n_groups, entries, slots, win,
                       (const int *)t.member_contig, t.region_start, t.region_end, t.region_contig);
    HIP_TRY(hipGetLastError());
    return regions_fold(s, ft, n, (const int *)t.region_start, (const int *)t.region_end,
                        (const int *)t.region_contig, most_items, false, []() { return 0; });
  };
  for (int level = 0; level < head.max_levels; level++) {
    if ((st = pass(level == 0 ? jn::BINS : jn::REFINE))) return st;
    hipLaunchKernelGGL(jn::search_kernel, dim3((unsigned)windows), dim3(jn::THREADS), 0, s->stream,
                       groups, level == 0 ? 1 : 0, win, penalty, (const long long *)ft.sum, t.total);
    HIP_TRY(hipGetLastError());
  }
  if ((st = pass(jn::FINAL))) return st;
  if (entries > 0) {
    hipLaunchKernelGGL(jn::report_kernel, dim3((unsigned)((entries + jn::THREADS - 1) / jn::THREADS)),
                       dim3(jn::THREADS), 0, s->stream, groups, n_groups, entries, win, penalty,
                       (const long long *)ft.sum, t.m_gain, t.m_up, t.m_sum, t.m_bases);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(t.ev[1], s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipEventElapsedTime(&g_joint_ms, t.ev[0], t.ev[1]));
  return 0;
}

/* the checks of the groups and of the windows' shape: 0 or what the call returns */
long long joint_check_groups(const psd_problem_set *s, const char *who, int n_groups, const int *group,
                             const long long *n_windows, const int *const *window_start,
                             const int *const *window_end, int windows_on_device) {
  if (n_groups < 0 || (!group && s->n_problems > 0)) {
    set_error("%s: %d groups%s", who, n_groups, group ? "" : " and no group array");
    return -ERROR_REGION_ARGUMENTS;
  }
  for (int p = 0; p < s->n_problems; p++)
    if (group[p] < -1 || group[p] >= n_groups) {
      set_error("%s: problem %d is in group %d, outside -1 .. %d", who, p, group[p], n_groups - 1);
      return -ERROR_REGION_ARGUMENTS;
    }
  for (int g = 0; g < n_groups && n_windows; g++) {
    if (n_windows[g] < 0) {
      set_error("%s: group %d has %lld windows", who, g, n_windows[g]);
      return -ERROR_REGION_ARGUMENTS;
    }
    if (n_windows[g] == 0) continue;
    const int *const *arrays[2] = {window_start, window_end};
    for (int j = 0; j < 2; j++) {
      const int *a = arrays[j] ? arrays[j][g] : nullptr;
      if (!a || (windows_on_device && ((unsigned long long)a & 3ull))) {
        set_error("%s: group %d: the window %s array is %s", who, g, j ? "end" : "start",
                  a ? "at a device address that is no multiple of 4" : "NULL");
        return -ERROR_REGION_ARGUMENTS;
      }
    }
  }
  return 0;
}

}  // namespace

extern "C" long long peakseg_hip_problem_set_pack_joint_peaks(
    psd_problem_set *s, const int *first_chromStart, int n_groups, const int *group, double penalty,
    const long long *n_windows, const int *const *window_start, const int *const *window_end,
    int windows_on_device, long long *windows_out, long long *members_out,
    const int **windowStart_dev, const int **windowEnd_dev, const int **peakStart_dev,
    const int **peakEnd_dev, const double **objective_dev, const int **samples_up_dev,
    const int **levels_dev, const double **m_gain_dev, const int **m_up_dev,
    const long long **m_sum_dev, const int **m_bases_dev) {
  if (!s || (!n_windows && !s->solved)) return -1;
  if (!s->dense) {
    set_error("pack_joint_peaks: the set was not made from dense counts or reads and has no run_end[]");
    return -1;
  }
  if (hipSetDevice(s->device) != hipSuccess) return -1;
  s->joint.windows = s->joint.entries = -1;
  if (first_chromStart_check(s, first_chromStart, "pack_joint_peaks")) return -1;
  if (!(penalty >= 0.0)) {
    set_error("pack_joint_peaks: the penalty %g is negative or not a number", penalty);
    return -ERROR_REGION_ARGUMENTS;
  }
  if (const long long bad = joint_check_groups(s, "pack_joint_peaks", n_groups, group, n_windows,
                                               window_start, window_end, windows_on_device))
    return bad;
  long long total = 0;
  const int st = joint_run(s, s->joint, "pack_joint_peaks", first_chromStart, n_groups, group, penalty,
                           0, nullptr, n_windows, window_start, window_end,
                           n_windows ? windows_on_device : 0, windows_out, members_out, &total);
  if (st) return st == ERROR_REGION_ARGUMENTS || st == ERROR_DEVICE_MEMORY ? -st : -1;
  const JointTable &t = s->joint;
  s->joint.windows = total;
  if (windowStart_dev) *windowStart_dev = t.ws;
  if (windowEnd_dev) *windowEnd_dev = t.we;
  if (peakStart_dev) *peakStart_dev = t.s;
  if (peakEnd_dev) *peakEnd_dev = t.e;
  if (objective_dev) *objective_dev = t.objective;
  if (samples_up_dev) *samples_up_dev = t.samples_up;
  if (levels_dev) *levels_dev = t.levels;
  if (m_gain_dev) *m_gain_dev = t.m_gain;
  if (m_up_dev) *m_up_dev = t.m_up;
  if (m_sum_dev) *m_sum_dev = t.m_sum;
  if (m_bases_dev) *m_bases_dev = t.m_bases;
  return total;
}

extern "C" int peakseg_hip_problem_set_packed_joint_peaks_download(
    psd_problem_set *s, int *windowStart_out, int *windowEnd_out, int *peakStart_out,
    int *peakEnd_out, double *objective_out, int *samples_up_out, int *levels_out, double *m_gain_out,
    int *m_up_out, long long *m_sum_out, int *m_bases_out) {
  if (!s || s->joint.windows < 0) return -1;
  const JointTable &t = s->joint;
  const size_t k = (size_t)t.windows, e = (size_t)t.entries;
  const void *from[11] = {t.ws, t.we, t.s, t.e, t.objective, t.samples_up, t.levels,
                          t.m_gain, t.m_up, t.m_sum, t.m_bases};
  void *to[11] = {windowStart_out, windowEnd_out, peakStart_out, peakEnd_out, objective_out,
                  samples_up_out, levels_out, m_gain_out, m_up_out, m_sum_out, m_bases_out};
  const size_t bytes[11] = {k * 4, k * 4, k * 4, k * 4, k * 8, k * 4, k * 4, e * 8, e * 4, e * 8, e * 4};
  for (int j = 0; j < 11; j++)
    if (to[j] && bytes[j] > 0 && hipMemcpy(to[j], from[j], bytes[j], hipMemcpyDeviceToHost) != hipSuccess) {
      set_error("download of the packed joint peaks failed");
      return -1;
    }
  return 0;
}

extern "C" int peakseg_hip_joint_peaks_last_ms(float *ms) {
  if (ms) *ms = g_joint_ms;
  return 0;
}
