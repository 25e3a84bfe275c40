/* peakseg_set.h -- the device problem set and its memory: struct psd_problem_set, its accounted
 * allocations, the block arena, the spill and overflow pools, the thread that grows the arena. */

/* What a solve launches on which kernel build (plan_solve in peakseg_solve.h) */
struct SolvePlan {
  bool throughput = false; /* which kernel build the last solve used */
  bool packed = false;     /* ... the packed build (pk) for the part that is not on the latency build */
  int n_lat_mixed = 0;     /* mixed launch: this many (longest) problems ran on the latency build */
  bool forced = false;     /* PEAKSEG_HIP_VARIANT named the build */
};

/* What the last solve decided and counted: reset as a whole when a solve starts, read by the
 * *_stats accessors and the packed-table downloads. */
struct SolveRun {
  SolvePlan plan;
  int widened = 0;         /* problems the packed build handed to the throughput build (a function
                              outgrew its 40-piece lists) */
  int launches = 0;                     /* kernel launches of the last solve */
  unsigned long long steps_run = 0;     /* data points the last solve's launches worked through */
  unsigned long long live_blocks_added = 0; /* blocks the last solve added under its kernels */
  int parks = 0;                          /* problems parked by the last solve's launches */
  unsigned long long park_pool_pieces = 0; /* ... and what they took from the overflow pool */
  long long pack_total = -1, segs_total = -1; /* rows of the packed tables (-1: not packed) */
  long long stats_total = -1;                 /* ... and of the packed segment statistics */
  long long labels_total = -1;                /* ... and of the packed label errors */
};

/* Segment tables packed at their exact sizes (peakseg_pack.h): up to three columns and, per
 * problem, first packed row, row count, source offset (pack_segments: and the contig's layout) */
struct PackedTable {
  void *col[3] = {nullptr, nullptr, nullptr};
  long long *d_rows = nullptr;
  long long capacity = 0;
};

/* The four columns of peakseg_hip_problem_set_pack_segment_stats, the keys they are decoded from,
 * and what the launches read: the per-problem descriptors (written by every call) and the problem
 * of every tile of the grid (the set's geometry: made by the first call, kept) */
struct StatsTable {
  long long *sum = nullptr;
  int *mx = nullptr, *summit_start = nullptr, *summit_end = nullptr;
  unsigned long long *key = nullptr;
  long long capacity = 0;
  long long *d_desc = nullptr;
  int *d_tile_problem = nullptr;
  long long n_tiles = 0;
  std::vector<long long> tile0; /* first tile of every problem */
  hipEvent_t ev[2] = {nullptr, nullptr};
};

/* What peakseg_hip_problem_set_pack_label_errors keeps (peakseg_labels.h): the labels of a call
 * with host arrays, the per-contig and per-problem descriptors, what translate_kernel leaves for
 * count_kernel, the contigs' check words, and the packed columns with the problems' totals.  Every
 * array grows to what the largest call so far needed. */
struct LabelTable {
  int *d_labels = nullptr;             /* 3 x labels: start, end, annotation (host arrays only) */
  psd::labels::Contig *d_contigs = nullptr; /* per contig */
  long long *d_lab_off = nullptr;      /* n_contigs + 1 */
  unsigned long long *d_check = nullptr; /* per contig */
  long long *d_desc = nullptr;         /* psd::labels::DESC per problem */
  int *totals = nullptr;               /* psd::labels::TOTALS per problem */
  psd::labels::Quad *where = nullptr;  /* per label: what translate_kernel leaves */
  int *count = nullptr, *fp = nullptr, *fn = nullptr; /* per packed row */
  long long label_capacity = 0, row_capacity = 0;
  hipEvent_t ev[2] = {nullptr, nullptr};
};

/* What peakseg_hip_problem_set_pack_coverage_stats keeps (peakseg_features.h): the tiles over the
 * contigs and their descriptors (the set's geometry: made by the first call, kept), the moments,
 * and the state of the selection, which grows to what the largest call so far needed. */
struct FeatureTable {
  long long *d_desc = nullptr;       /* psd::cover::DESC per contig */
  int *d_tile_contig = nullptr;
  long long n_tiles = -1;            /* (-1: no geometry yet) */
  unsigned long long *moments = nullptr; /* psd::cover::MOMENTS per contig */
  int *prefix = nullptr, *leader = nullptr, *value = nullptr; /* per contig and rank */
  long long *resid = nullptr;
  unsigned long long *hist = nullptr; /* psd::cover::BINS per contig and rank */
  long long rank_capacity = 0;       /* contigs x ranks the state has room for */
  long long total = -1;              /* entries of value[] after the last call (-1: none) */
  hipEvent_t ev[2] = {nullptr, nullptr};
};

/* What peakseg_hip_problem_set_pack_region_stats keeps (peakseg_regions.h): the regions of a call
 * with host arrays, the contigs' descriptors and check words, what locate_kernel leaves for
 * fold_kernel (spans and the two levels of prefix sums), and the packed columns.  Every array grows
 * to what the largest call so far needed.  The cluster-by-member matrix has a table of its own. */
struct RegionTable {
  int *d_regions = nullptr;                  /* 2 x regions: start, end (host arrays only) */
  psd::regions::Contig *d_contigs = nullptr; /* per contig */
  long long *d_reg_off = nullptr;            /* n_contigs + 1 */
  unsigned long long *d_check = nullptr;     /* per contig */
  psd::regions::Span *span = nullptr;        /* per region */
  int *off = nullptr;                        /* per region */
  long long *block_sum = nullptr;            /* per workgroup of locate_kernel, and the total */
  int *bases = nullptr, *mx = nullptr;       /* per region: the packed columns */
  long long *sum = nullptr;
  long long capacity = 0;
  long long total = -1; /* regions of the last call (-1: nothing packed) */
  hipEvent_t ev[2] = {nullptr, nullptr};
};

/* What peakseg_hip_problem_set_pack_peak_clusters keeps (peakseg_clusters.h): the members and
 * groups of a call, the members' peaks, the flags' prefix sums, the cluster table, the groups'
 * cluster counts, and the matrix with the regions its entries are.  Every array grows to what the
 * largest call so far needed. */
struct ClusterTable {
  psd::clusters::Member *members = nullptr;                     /* per member */
  long long *member_off = nullptr;                              /* members + 1 */
  int *member_group = nullptr, *member_contig = nullptr;        /* per member */
  int *group_member0 = nullptr;                                 /* groups + 1 */
  long long *group_clusters = nullptr, *entry_off = nullptr, *cluster_off = nullptr; /* groups + 1 */
  long long member_capacity = 0, group_capacity = 0;
  int *peak_start = nullptr, *peak_end = nullptr, *lead = nullptr, *off = nullptr; /* per peak (+ 1) */
  long long *block_sum = nullptr;
  int *cluster_start = nullptr, *cluster_end = nullptr, *cluster_peaks = nullptr,
      *cluster_samples = nullptr; /* per cluster: at most one per peak */
  long long peak_capacity = 0;
  int *m_peaks = nullptr, *region_start = nullptr, *region_end = nullptr, *region_contig = nullptr;
  long long entry_capacity = 0;
  RegionTable matrix;   /* bases, sum and max of the entries */
  long long clusters = -1, entries = -1; /* of the last call (-1: nothing packed) */
  hipEvent_t ev[2] = {nullptr, nullptr};
};

/* What peakseg_hip_problem_set_pack_joint_peaks keeps (peakseg_joint.h): the groups and members of a
 * call, the windows with their peaks, the regions of a level and their fold, and the matrix.  Every
 * array grows to what the largest call so far needed.  pack_joint_path keeps a table of its own of
 * the same kind, with a row per (penalty, window) and per (penalty, entry), and what
 * pack_joint_label_errors needs of the call: the penalties' number and every problem's group and
 * place among its members. */
struct JointTable {
  int *member0 = nullptr;                                        /* groups + 1 */
  long long *win_off = nullptr, *entry_off = nullptr, *lo = nullptr, *hi = nullptr; /* groups + 1 */
  const int **g_start = nullptr, **g_end = nullptr;              /* groups + 1 */
  long long group_capacity = 0;
  int *member_contig = nullptr;                                  /* per member */
  long long member_capacity = 0;
  int *d_windows = nullptr;                                      /* 2 x windows: as given (host arrays) */
  int *w_group = nullptr, *ws = nullptr, *we = nullptr, *b = nullptr, *s = nullptr, *e = nullptr,
      *levels = nullptr, *samples_up = nullptr;                  /* per window */
  double *objective = nullptr;
  long long window_capacity = 0;
  psd::joint::Head *head = nullptr;
  long long *total = nullptr;                                    /* per entry */
  double *m_gain = nullptr;
  int *m_up = nullptr, *m_bases = nullptr;
  long long *m_sum = nullptr;
  long long entry_capacity = 0;
  int *region_start = nullptr, *region_end = nullptr, *region_contig = nullptr; /* per region of a level */
  long long region_capacity = 0;
  RegionTable fold;     /* the fold of a level's regions */
  long long windows = -1, entries = -1; /* of the last call (-1: nothing packed) */
  hipEvent_t ev[2] = {nullptr, nullptr};
  /* the path only */
  double *carry = nullptr;               /* level 0's sums between slabs of members */
  long long carry_capacity = 0;
  int penalties = 0, groups = 0;         /* of the last call */
  std::vector<int> problem_group, problem_member; /* per problem: its group (-1: none), its place in it */
};

/* What peakseg_hip_problem_set_pack_joint_label_errors keeps (peakseg_joint_labels.h). */
struct JointLabelTable {
  psd::joint_labels::Problem *d_problems = nullptr; /* per problem */
  long long *d_lab_off = nullptr;                   /* problems + 1 */
  unsigned long long *d_check = nullptr;            /* per problem */
  int *d_labels = nullptr;                          /* 3 x labels (host arrays only) */
  long long label_capacity = 0;
  int *count = nullptr, *fp = nullptr, *fn = nullptr; /* per (penalty, label) */
  long long row_capacity = 0;
  int *totals = nullptr;                            /* TOTALS per (penalty, problem) */
  long long total_capacity = 0;
  long long *model = nullptr;                       /* TOTALS per penalty (MAX_PENALTIES of them) */
  long long labels = -1;                            /* of the last call (-1: nothing packed) */
  int penalties = 0;
  hipEvent_t ev[2] = {nullptr, nullptr};
};

/* What peakseg_hip_problem_set_pack_heldout_loss keeps (peakseg_heldout.h): the problems'
 * descriptors, the contigs' bases and the head of a call, the pairs of a call with host arrays, the
 * two levels of the pairs' row counts, the rows as flat regions with their fold, and the packed
 * columns.  Every array grows to what the largest call so far needed. */
struct HeldoutTable {
  psd::heldout::Problem *d_problems = nullptr; /* per problem */
  long long *d_contig_bases = nullptr;         /* per contig */
  psd::heldout::Head *d_head = nullptr;
  int *d_pairs = nullptr;                      /* 2 x pairs: problem, contig (host arrays only) */
  double *d_scale = nullptr;                   /* per pair (host arrays only) */
  long long copy_capacity = 0;
  int *off = nullptr;                          /* per pair */
  long long *block_sum = nullptr;              /* per workgroup of pairs_kernel, and the total */
  double *loss = nullptr;                      /* per pair: the packed columns */
  int *rows = nullptr, *zero = nullptr;
  long long *bases = nullptr, *sum = nullptr;
  long long pair_capacity = 0;
  int *flat_start = nullptr, *flat_end = nullptr, *flat_contig = nullptr; /* per row */
  long long row_capacity = 0;
  RegionTable fold;     /* the fold of the rows */
  long long pairs = -1; /* of the last call (-1: nothing packed) */
  hipEvent_t ev[2] = {nullptr, nullptr};
};

struct psd_problem_set {
  /* geometry: the contigs, the problems and where their tables start */
  int device = 0;
  int n_cu = 0;            /* compute units of the device */
  int n_contigs = 0, n_problems = 0;
  std::vector<int> contig_n;
  std::vector<long long> contig_off;
  /* what loss.tsv needs of a contig: its bases (the sum of its bins' widths) */
  std::vector<long long> contig_bases;
  std::vector<int> prob_contig;
  std::vector<double> prob_penalty;
  std::vector<long long> prob_fn_off, prob_seg_off;
  long long dp_bins = 0;
  std::vector<int> order;  /* problems, longest contig first */
  int ckpt_interval = 0;                 /* 0 = full store */
  unsigned long long ckpt_pieces_per_fn = 0; /* region sizing of the checkpointed store */
  bool can_park = false;   /* the set has a park slot per problem (full store) */

  /* The arena: blocks of 2^ar_block_log2 pieces, each a device allocation of its own (an
   * address range reserved, created, mapped and given access by the virtual-memory API; plain
   * hipMalloc without it).  Blocks can be added while a kernel runs (fpop_types.h), which is
   * what grow_arena_live() does from a second host thread during a solve. */
  struct ArenaBlock {
    void *base = nullptr;
    bool vmm = false;
#ifndef PSD_EMU
    hipMemGenericAllocationHandle_t handle{};
#endif
  };
  std::vector<ArenaBlock> arena_blocks;
  unsigned long long arena_pieces = 0;
  bool arena_auto = true;
  unsigned long long arena_used = 0;  /* pieces handed out by the last solve */
  bool arena_vmm = false;
  size_t table_cap = 0;              /* entries of the two block tables */
  size_t table_synced = 0;           /* blocks whose address is in the device table */
  unsigned long long *h_live = nullptr; /* pinned: [0] pieces mapped, [1] final, [2 + b] bases */
  unsigned long long *h_used = nullptr; /* pinned: pieces handed out (kernel -> host) */
  bool live_growth = false;          /* this set's arena grows while its kernel runs */

  /* pools (their arrays are in DeviceArgs) */
  int spill_slots = 0;

  /* launch resources */
  psd::DeviceArgs d{};
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipStream_t stream2 = nullptr;
  hipEvent_t ev2 = nullptr;
  int *started = nullptr; /* pinned host word: latency-build workgroups of a mixed launch */
  bool mixed_wait_timed_out = false; /* the wait for them ran into its bound once: recorded, not repeated */
  int *d_resume = nullptr; /* device copy of resume_t */
  int *d_order_sub = nullptr; /* launch order of a relaunch: the unfinished problems */
  std::vector<int> resume_t;  /* per problem: data point to resume at (0: from the start) */
  std::vector<psd::ProbResult> results;
  bool solved = false;

  /* packed outputs: the segment tables (peakseg_hip_problem_set_pack_tables: start, mean) and
   * the reference's segments table (peakseg_hip_problem_set_pack_segments: chromStart, chromEnd,
   * mean) */
  PackedTable pack, segs;
  StatsTable stats; /* (sets made from dense counts) */
  LabelTable labels; /* (sets made from dense counts) */
  FeatureTable features; /* (sets made from dense counts) */
  RegionTable regions; /* (sets made from dense counts) */
  ClusterTable clusters; /* (sets made from dense counts) */
  JointTable joint; /* (sets made from dense counts) */
  JointTable joint_path; /* (sets made from dense counts) */
  JointLabelTable joint_labels; /* (sets made from dense counts) */
  HeldoutTable heldout; /* (sets made from dense counts) */

  /* Sets made from dense counts (peakseg_hip_problem_set_create_dense): run_end[] next to count[]
   * and weight[], the sum of each contig's counts, and which contigs are constant.  Their trivial
   * models (penalty +Inf, constant contig) are served in closed form and never launched. */
  bool dense = false;
  int *d_run_end = nullptr;
  std::vector<long long> contig_sum;
  std::vector<char> contig_constant;
  std::vector<int> contig_max; /* each contig's largest count */
  int *d_order_run = nullptr; /* launch order of a solve that leaves trivial problems out */

  SolveRun run; /* per-solve state */

  /* device memory: what dev_alloc handed out, and its bytes with the arena's */
  std::vector<void *> allocs;
  unsigned long long bytes = 0;
  unsigned long long max_bytes = 0;   /* PEAKSEG_HIP_MAX_BYTES (0 = no cap besides free HBM) */
};

namespace {

template <class T>
int dev_alloc(psd_problem_set *s, T **p, size_t n) {
  void *q = nullptr;
  size_t bytes = (n ? n : 1) * sizeof(T);
  hipError_t e = hipMalloc(&q, bytes);
  if (e != hipSuccess) {
    set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    return ERROR_DEVICE_MEMORY;
  }
  s->allocs.push_back(q);
  s->bytes += bytes;
  *p = (T *)q;
  return 0;
}

template <class T>
int dev_upload(psd_problem_set *s, const T **p, const std::vector<T> &v) {
  T *q = nullptr;
  int st = dev_alloc(s, &q, v.size());
  if (st) return st;
  if (!v.empty()) HIP_TRY(hipMemcpy(q, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *p = q;
  return 0;
}

/* the reverse of dev_alloc for a pointer (NULL: nothing) that accounted for `bytes`; NULL after */
template <class T>
void dev_free(psd_problem_set *s, T *&p, unsigned long long bytes) {
  void *q = (void *)p;
  if (!q) return;
  p = nullptr;
  for (size_t i = 0; i < s->allocs.size(); i++) {
    if (s->allocs[i] == q) {
      s->allocs.erase(s->allocs.begin() + (long)i);
      break;
    }
  }
  (void)hipFree(q);
  s->bytes -= bytes;
}

unsigned long long env_bytes(const char *name) {
  const char *e = getenv(name);
  if (!e || !*e) return 0;
  char *end = nullptr;
  double v = strtod(e, &end);
  if (end == e || !(v > 0)) return 0;
  switch (*end) { /* optional K/M/G/T suffix */
    case 'k': case 'K': v *= 1024.0; break;
    case 'm': case 'M': v *= 1024.0 * 1024.0; break;
    case 'g': case 'G': v *= 1024.0 * 1024.0 * 1024.0; break;
    case 't': case 'T': v *= 1024.0 * 1024.0 * 1024.0 * 1024.0; break;
    default: break;
  }
  return (unsigned long long)v;
}

/* How many arena pieces may still be allocated: what the device has free (a tenth is left for
 * other processes sharing the GPU -- R's future workers are separate processes on one device,
 * SURVEY.md section 8b "Threading") and what PEAKSEG_HIP_MAX_BYTES leaves of this set's budget. */
unsigned long long arena_fit(psd_problem_set *s) {
  unsigned long long fit = ~0ull;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) fit = (unsigned long long)(free_b * 0.9) / 20ull;
  if (s->max_bytes) {
    unsigned long long room = s->max_bytes > s->bytes ? (s->max_bytes - s->bytes) / 20ull : 0ull;
    if (room < fit) fit = room;
  }
  return fit;
}


size_t arena_block_bytes(const psd_problem_set *s) { return (size_t)20 << s->d.ar_block_log2; }
unsigned long long arena_mapped(const psd_problem_set *s) {
  return (unsigned long long)s->arena_blocks.size() << s->d.ar_block_log2;
}

/* release the arena: every block, and the block tables */
void free_arena(psd_problem_set *s) {
  const size_t bytes = arena_block_bytes(s);
  for (auto &b : s->arena_blocks) {
#ifndef PSD_EMU
    if (b.vmm) {
      (void)hipMemUnmap(b.base, bytes);
      (void)hipMemRelease(b.handle);
      (void)hipMemAddressFree(b.base, bytes);
    } else
#endif
    {
      (void)hipFree(b.base);
    }
    s->bytes -= bytes;
  }
  s->arena_blocks.clear();
  dev_free(s, s->d.ar_block, s->table_cap * sizeof(char *));
  if (s->h_live) (void)hipHostFree(s->h_live);
  if (s->h_used) (void)hipHostFree(s->h_used);
  s->h_live = s->h_used = nullptr;
  s->table_cap = s->table_synced = 0;
  s->d.ar_cap = 0;
  s->arena_pieces = 0;
}

/* One more block.  Safe while a kernel of this set runs: nothing the kernel uses is touched,
 * the block is published through the pinned words (address first, then the capacity). */
int arena_add_block(psd_problem_set *s) {
  if (s->arena_blocks.size() >= s->table_cap) {
    set_error("cost-function arena: block table of %zu entries is full", s->table_cap);
    return ERROR_DEVICE_MEMORY;
  }
  const size_t bytes = arena_block_bytes(s);
  psd_problem_set::ArenaBlock b;
  const char *what = "hipMalloc";
  hipError_t e = hipSuccess;
#ifndef PSD_EMU
  if (s->arena_vmm) {
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = s->device;
    hipMemAccessDesc acc = {};
    acc.location.type = hipMemLocationTypeDevice;
    acc.location.id = s->device;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    b.vmm = true;
    what = "hipMemAddressReserve";
    e = hipMemAddressReserve(&b.base, bytes, (size_t)2 << 20, nullptr, 0);
    if (e == hipSuccess) {
      what = "hipMemCreate";
      e = hipMemCreate(&b.handle, bytes, &prop, 0);
      if (e == hipSuccess) {
        what = "hipMemMap";
        e = hipMemMap(b.base, bytes, 0, b.handle, 0);
        if (e == hipSuccess) {
          what = "hipMemSetAccess";
          e = hipMemSetAccess(b.base, bytes, &acc, 1);
          if (e != hipSuccess) (void)hipMemUnmap(b.base, bytes);
        }
        if (e != hipSuccess) (void)hipMemRelease(b.handle);
      }
      if (e != hipSuccess) (void)hipMemAddressFree(b.base, bytes);
    }
  } else
#endif
  {
    e = hipMalloc(&b.base, bytes);
  }
  if (e != hipSuccess) {
    set_error("cost-function arena: block %zu of %zu bytes failed in %s: %s", s->arena_blocks.size(),
              bytes, what, hipGetErrorString(e));
    (void)hipGetLastError();
    return ERROR_DEVICE_MEMORY;
  }
  s->arena_blocks.push_back(b);
  s->bytes += bytes;
  const size_t k = s->arena_blocks.size() - 1;
  __atomic_store_n(&s->h_live[2 + k], (unsigned long long)(uintptr_t)b.base, __ATOMIC_RELAXED);
  __atomic_store_n(&s->h_live[0], arena_mapped(s), __ATOMIC_RELEASE);
  return 0;
}

/* between launches: the device table learns the blocks added since, DeviceArgs the capacity */
int arena_sync_table(psd_problem_set *s) {
  const size_t n = s->arena_blocks.size();
  if (n > s->table_synced) {
    std::vector<char *> bases;
    for (size_t k = s->table_synced; k < n; k++) bases.push_back((char *)s->arena_blocks[k].base);
    HIP_TRY(hipMemcpy(s->d.ar_block + s->table_synced, bases.data(), bases.size() * sizeof(char *),
                      hipMemcpyHostToDevice));
    s->table_synced = n;
  }
  s->d.ar_cap = arena_mapped(s);
  s->arena_pieces = s->d.ar_cap;
  return 0;
}

/* Give the arena at least `pieces` pieces in all, never more than `limit` (0: no limit): the
 * first allocation, or growth between launches.  Growth adds blocks: no record moves, so a
 * solve that ran out of room is resumed, not repeated. */
int alloc_arena(psd_problem_set *s, unsigned long long pieces, unsigned long long limit = 0,
                bool starter_only = false) {
  const bool first = s->arena_blocks.empty() && s->d.ar_block == nullptr;
  const unsigned long long n_waves = 2ull * (unsigned long long)s->n_problems;
  if (first) {
    /* chunk size: about a sixteenth of what one wave will store, within [2^10, 2^16] pieces */
    int lg = psd::ARENA_CHUNK_LOG2_MIN;
    while (lg < psd::ARENA_CHUNK_LOG2_MAX && (pieces / n_waves) >> (lg + 5)) lg++;
    s->d.ar_chunk_log2 = lg;
    /* block size: about an eighth of the first estimate, within [2^19, 2^24] pieces (10 MB to
     * 336 MB; 2^19 pieces make the int array 2 MiB, the granularity the virtual-memory calls
     * accept on ROCm 7.2); the checkpointed store needs a wave's region inside one block */
    int blg = psd::ARENA_BLOCK_LOG2_MIN;
    while (blg < psd::ARENA_BLOCK_LOG2_MAX && (pieces >> (blg + 3))) blg++;
    if (const char *e = getenv("PEAKSEG_HIP_ARENA_BLOCK_LOG2")) {
      /* tests: blocks smaller than the virtual-memory granularity come from hipMalloc */
      const int v = atoi(e);
      if (v >= lg && v >= 10 && v <= psd::ARENA_BLOCK_LOG2_MAX) blg = v;
    }
#ifndef PSD_EMU
    int vmm = 0;
    s->arena_vmm = !getenv("PEAKSEG_HIP_NO_VMM") && blg >= psd::ARENA_BLOCK_LOG2_MIN &&
                   hipDeviceGetAttribute(&vmm, hipDeviceAttributeVirtualMemoryManagementSupported,
                                         s->device) == hipSuccess && vmm != 0;
#endif
    while (s->ckpt_interval > 0 && blg < psd::ARENA_BLOCK_LOG2_CKPT_MAX && (1ull << blg) < s->d.ckpt_region)
      blg++;
    s->d.ar_block_log2 = blg;
    /* tables for every block the device's memory could hold */
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || total_b == 0) total_b = (size_t)288 << 30;
    s->table_cap = (size_t)(((unsigned long long)total_b / 20ull) >> blg) + 8;
    int st = dev_alloc(s, &s->d.ar_block, s->table_cap);
    if (st) return st;
    hipError_t e = hipMemset(s->d.ar_block, 0, s->table_cap * sizeof(char *));
    if (e == hipSuccess)
      e = hipHostMalloc((void **)&s->h_live, (2 + s->table_cap) * sizeof(unsigned long long),
                        hipHostMallocCoherent | hipHostMallocMapped);
    if (e == hipSuccess)
      e = hipHostMalloc((void **)&s->h_used, 64, hipHostMallocCoherent | hipHostMallocMapped);
    if (e != hipSuccess) {
      set_error("cost-function arena: block tables: %s", hipGetErrorString(e));
      return ERROR_DEVICE_MEMORY;
    }
    memset(s->h_live, 0, (2 + s->table_cap) * sizeof(unsigned long long));
    s->h_live[1] = 1; /* final until a solve says otherwise */
    *s->h_used = 0;
    s->d.ar_live = s->h_live;
    s->d.ar_used = s->h_used;
    s->table_synced = 0;
  }
  const int blg = s->d.ar_block_log2;
  const unsigned long long chunk = 1ull << s->d.ar_chunk_log2;
  if (s->ckpt_interval > 0) {
    /* whole regions per block (the kernel's addressing, forward_body): the caller asks for
     * region x 2 x problems, the blocks hold a whole number of regions each */
    if ((1ull << blg) < s->d.ckpt_region) {
      set_error("checkpointed store: a region of %llu pieces exceeds the largest arena block (%llu)",
                s->d.ckpt_region, 1ull << blg);
      return ERROR_DEVICE_MEMORY;
    }
    const unsigned long long per_block = (1ull << blg) / s->d.ckpt_region;
    pieces = ((n_waves + per_block - 1) / per_block) << blg;
    if (limit && pieces > limit) {
      /* The kernel indexes region (2 p + chain) without looking at ar_cap: an arena clipped to
       * what fits would be written beyond its end.  The regions either fit or the set does not. */
      set_error("checkpointed store: %llu pieces per region x %llu regions (%llu bytes) do not "
                "fit (free HBM / PEAKSEG_HIP_MAX_BYTES)", s->d.ckpt_region, n_waves, pieces * 20ull);
      return ERROR_DEVICE_MEMORY;
    }
  } else {
    /* at least two chunks per wave so that nobody starves at start-up */
    const unsigned long long min_pieces = chunk * 2ull * n_waves;
    /* (live growth: just that and two blocks of headroom; the rest comes under the kernel) */
    if (starter_only) pieces = min_pieces + (2ull << blg);
    if (pieces < min_pieces) pieces = min_pieces;
  }
  unsigned long long want_blocks = (pieces + (1ull << blg) - 1) >> blg;
  if (limit) {
    /* a limit counts whole blocks, rounded DOWN: the cap is a hard bound for processes that
     * share a GPU (one block at least: without it there is no arena) */
    unsigned long long most = limit >> blg;
    if (most < 1) most = 1;
    if (want_blocks > most) want_blocks = most;
  }
  int st = 0;
  const size_t before = s->arena_blocks.size();
  while (s->arena_blocks.size() < want_blocks) {
    st = arena_add_block(s);
#ifndef PSD_EMU
    if (st && first && s->arena_vmm && s->arena_blocks.empty()) {
      /* the virtual-memory calls refuse on this system: plain allocations from here on */
      s->arena_vmm = false;
      continue;
    }
#endif
    if (st) break;
  }
  if (st && s->arena_blocks.size() == before) return st; /* keep what could be added otherwise */
  return arena_sync_table(s);
}

void free_spill(psd_problem_set *s) {
  const unsigned long long n = (unsigned long long)s->spill_slots * (unsigned long long)s->d.spill_cap;
  dev_free(s, s->d.spill_f64, n * 48ull * 8);
  dev_free(s, s->d.spill_i32, n * 12ull * 4);
  s->spill_slots = 0;
  s->d.spill_slots = 0;
}

/* Pool of HBM spill slots for problems whose functions outgrow LDS (adversarial data): 432
 * bytes per piece of capacity per slot; a problem takes a slot on its first overflow. */
int alloc_spill(psd_problem_set *s, int slots) {
  if (slots > s->n_problems) slots = s->n_problems;
  if (slots < 1) slots = 1;
  const size_t cap = (size_t)s->d.spill_cap;
  int st;
  if (cap == 0) return 0;
  if ((st = dev_alloc(s, &s->d.spill_f64, (size_t)slots * 48 * cap)) ||
      (st = dev_alloc(s, &s->d.spill_i32, (size_t)slots * 12 * cap)))
    return st;
  s->spill_slots = slots;
  s->d.spill_slots = slots;
  return 0;
}

void free_ckpt_overflow(psd_problem_set *s) {
  dev_free(s, s->d.ckpt_ovf_f64, s->d.ckpt_ovf_cap * 48ull);
  dev_free(s, s->d.ckpt_ovf_i32, s->d.ckpt_ovf_cap * 4ull);
  s->d.ckpt_ovf_cap = 0;
}

/* Overflow pool of the checkpointed store: checkpoints of functions too long for a slot. */
int alloc_ckpt_overflow(psd_problem_set *s, unsigned long long pieces) {
  if (pieces < 1024) pieces = 1024;
  int st;
  if ((st = dev_alloc(s, &s->d.ckpt_ovf_f64, (size_t)pieces * 6)) ||
      (st = dev_alloc(s, &s->d.ckpt_ovf_i32, (size_t)pieces)))
    return st;
  s->d.ckpt_ovf_cap = pieces;
  return 0;
}

/* Full store: a larger overflow pool that KEEPS what parked problems have in it (they read it
 * back when they are resumed). */
int grow_ckpt_overflow_keep(psd_problem_set *s, unsigned long long pieces) {
  double *f64 = nullptr;
  int *i32 = nullptr;
  int st;
  if ((st = dev_alloc(s, &f64, (size_t)pieces * 6)) || (st = dev_alloc(s, &i32, (size_t)pieces))) {
    dev_free(s, f64, pieces * 48ull);
    return st;
  }
  const size_t old = (size_t)s->d.ckpt_ovf_cap;
  /* a function of n pieces at offset off: 6 n doubles from 6 off, n ints from off -- offsets
   * are positions, not sizes, so the arrays are copied as they are */
  HIP_TRY(hipMemcpy(f64, s->d.ckpt_ovf_f64, old * 6 * sizeof(double), hipMemcpyDeviceToDevice));
  HIP_TRY(hipMemcpy(i32, s->d.ckpt_ovf_i32, old * sizeof(int), hipMemcpyDeviceToDevice));
  /* (device-to-device copies may return before they have run, and the set's streams do not wait
   * for the null stream) */
  HIP_TRY(hipStreamSynchronize((hipStream_t) nullptr));
  free_ckpt_overflow(s);
  s->d.ckpt_ovf_f64 = f64;
  s->d.ckpt_ovf_i32 = i32;
  s->d.ckpt_ovf_cap = pieces;
  return 0;
}

/* While the kernels of a solve run: a second host thread maps arena blocks AHEAD of what the
 * waves have taken (ar_used, a pinned word the waves add to whenever they take chunks), up to
 * what the device and PEAKSEG_HIP_MAX_BYTES allow.  A wave that needs a block that is not there
 * yet waits for it (arena_take); when no more can come the thread says so and the wave parks its
 * problem.  Mapping a block is 13-35 ms per GB where the memory has been used before: at the
 * 1.3 GB/s the 64-penalty grid stores, or the 14 GB/s of a full chip, the thread keeps ahead. */
struct LiveGrower {
  psd_problem_set *s = nullptr;
  unsigned long long limit = 0; /* pieces the arena may reach */
  std::atomic<bool> stop{false};
  std::thread th;
  unsigned long long added = 0;

  void start(psd_problem_set *set, unsigned long long limit_pieces) {
    s = set;
    limit = limit_pieces;
    __atomic_store_n(&s->h_live[0], arena_mapped(s), __ATOMIC_RELAXED);
    __atomic_store_n(&s->h_live[1], 0ull, __ATOMIC_RELEASE);
    th = std::thread([this]() { run(); });
  }
  void run() {
    (void)hipSetDevice(s->device);
    const unsigned long long B = 1ull << s->d.ar_block_log2;
    bool final = false;
    while (!stop.load(std::memory_order_acquire)) {
      bool progressed = false;
      for (;;) {
        const unsigned long long used = __atomic_load_n(s->h_used, __ATOMIC_ACQUIRE);
        unsigned long long ahead = used / 8ull;
        if (ahead < 2ull * B) ahead = 2ull * B;
        if (final || arena_mapped(s) >= used + ahead) break;
        if (arena_mapped(s) + B > limit || arena_add_block(s) != 0) {
          final = true; /* the capacity published so far is all there will be */
          __atomic_store_n(&s->h_live[1], 1ull, __ATOMIC_RELEASE);
          break;
        }
        added++;
        progressed = true;
      }
      if (!progressed) std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
  }
  void finish() {
    if (!th.joinable()) return;
    stop.store(true, std::memory_order_release);
    th.join();
    __atomic_store_n(&s->h_live[1], 1ull, __ATOMIC_RELEASE);
    s->run.live_blocks_added += added;
  }
  /* (whoever starts one lets it go out of scope before it returns: the thread works on *s) */
  ~LiveGrower() { finish(); }
};

}  // namespace
