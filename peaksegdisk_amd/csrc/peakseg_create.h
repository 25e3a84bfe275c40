/* peakseg_create.h -- creation of a problem set: what both creators share once the contigs' data is
 * known, step by step, and the creator from bins (the one from dense counts: peakseg_dense.h). */
namespace {

/* PEAKSEG_HIP_TIMING=1: where the creation of a set spends its time, on stderr */
struct CreateLaps {
  bool on = timing_on();
  std::chrono::steady_clock::time_point mark = std::chrono::steady_clock::now();
  void operator()(const char *what) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "peakseg_hip timing: create: %-26s %8.3f s\n", what,
            std::chrono::duration<double>(now - mark).count());
    mark = now;
  }
};

/* A creator owns its half-built set through this: every exit but the last destroys it */
typedef std::unique_ptr<psd_problem_set, void (*)(psd_problem_set *)> SetOwner;

/* Store mode.  Full store: every cost function's backtrack record stays in HBM, as the
 * reference keeps them on disk (about 24 + 40 P bytes per data point and penalty).
 * Checkpointed store: only a checkpoint every K data points and the
 * records of one block of K at a time; the decoding recomputes the blocks it walks through.
 * Chosen when the full store would not fit (free HBM / PEAKSEG_HIP_MAX_BYTES), or forced
 * with PEAKSEG_HIP_CHECKPOINT=K. */
void choose_store(psd_problem_set *s, unsigned long long arena_pieces) {
  s->max_bytes = env_bytes("PEAKSEG_HIP_MAX_BYTES");
  int K = 0;
  if (const char *e = getenv("PEAKSEG_HIP_CHECKPOINT")) K = atoi(e);
  if (K == 0 && arena_pieces == 0 && !getenv("PEAKSEG_HIP_NO_CHECKPOINT")) {
    /* what the full store needs at a typical 8 pieces per function, with the tables */
    const double need = (double)s->dp_bins * (2.0 * 8.0 * 20.0 + 16.0 + 12.0);
    size_t free_b = 0, total_b = 0;
    double room = 1e30;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) room = (double)free_b * 0.9;
    if (s->max_bytes && (double)s->max_bytes < room) room = (double)s->max_bytes;
    if (need > room) K = 2048;
  }
  if (K < 0) K = 0;
  if (K > 0 && K < 16) K = 16;
  s->ckpt_interval = K;
  /* Full store: one park slot per problem (13 KB), so that a solve that runs out of arena is
   * resumed after the arena has grown instead of repeated (PEAKSEG_HIP_NO_PARK=1: as rounds
   * 1-2, rerun the set; sets of more than 16384 problems do without, too). */
  s->can_park = K == 0 && s->n_problems <= 16384 && !getenv("PEAKSEG_HIP_NO_PARK");
}

/* The problems' tables and the launch order, on the host and on the device; the contig data is
 * uploaded here unless the dense encoder left it in HBM (count == nullptr).  *ckpt_slots: the
 * checkpoint slots the problems need in all (checkpointed store). */
int create_tables(psd_problem_set *s, const std::vector<double> &min_lm,
                  const std::vector<double> &max_lm, const std::vector<int> *count,
                  const std::vector<int> *weight, const int *problem_contig,
                  const double *problem_penalty, long long *ckpt_slots) {
  const int n_problems = s->n_problems, K = s->ckpt_interval;
  long long fn_off = 0, seg_off = 0, ckpt_off = 0;
  std::vector<long long> prob_ckpt_off;
  for (int p = 0; p < n_problems; p++) {
    int c = problem_contig[p];
    const long long n = s->contig_n[(size_t)c];
    s->prob_contig.push_back(c);
    s->prob_penalty.push_back(problem_penalty[p]);
    s->prob_fn_off.push_back(fn_off);
    s->prob_seg_off.push_back(seg_off);
    prob_ckpt_off.push_back(K > 0 ? ckpt_off : (s->can_park ? (long long)p : 0ll));
    fn_off += K > 0 ? 2ll * (K + 1) : 2ll * n;
    seg_off += n + 1;
    if (K > 0) ckpt_off += (n - 1) / K;
  }
  *ckpt_slots = ckpt_off;
  /* workgroups are dispatched in index order: start the longest problems first so that a
   * set of unequal contigs does not end with one long problem running alone */
  s->order.resize((size_t)n_problems);
  for (int p = 0; p < n_problems; p++) s->order[(size_t)p] = p;
  std::stable_sort(s->order.begin(), s->order.end(), [&](int x, int y) {
    return s->contig_n[(size_t)s->prob_contig[(size_t)x]] >
           s->contig_n[(size_t)s->prob_contig[(size_t)y]];
  });
  int st = 0;
  psd::DeviceArgs &d = s->d;
  d.n_problems = n_problems;
  if ((st = dev_upload(s, &d.prob_contig, s->prob_contig)) ||
      (st = dev_upload(s, &d.prob_penalty, s->prob_penalty)) ||
      (st = dev_upload(s, &d.prob_fn_off, s->prob_fn_off)) ||
      (st = dev_upload(s, &d.prob_seg_off, s->prob_seg_off)) ||
      (st = dev_upload(s, &d.prob_order, s->order)) ||
      (st = dev_upload(s, &d.contig_n, s->contig_n)) ||
      (st = dev_upload(s, &d.contig_off, s->contig_off)) ||
      (st = dev_upload(s, &d.contig_min_log_mean, min_lm)) ||
      (st = dev_upload(s, &d.contig_max_log_mean, max_lm)) ||
      (count && ((st = dev_upload(s, &d.count, *count)) ||
                 (st = dev_upload(s, &d.weight, *weight)))) ||
      (st = dev_alloc(s, &d.result, (size_t)n_problems)) ||
      (st = dev_alloc(s, &d.ar_next_chunk, (size_t)1)) ||
      (st = dev_alloc(s, &d.spill_next, (size_t)1)) ||
      (st = dev_alloc(s, const_cast<psd::DeviceArgs **>(&d.self), (size_t)1)) ||
      (st = dev_alloc(s, &d.fn_ref, (size_t)fn_off)) ||
      (st = dev_alloc(s, &d.seg_start, (size_t)seg_off)) ||
      (st = dev_alloc(s, &d.seg_mean, (size_t)seg_off)))
    return st;
  return dev_upload(s, &d.prob_ckpt_off, prob_ckpt_off);
}

/* Park slots or checkpoint slots with their overflow pool, the spill pool, the profile counters */
int create_pools(psd_problem_set *s, long long ckpt_slots) {
  const int n_problems = s->n_problems, K = s->ckpt_interval;
  const bool park = s->can_park;
  psd::DeviceArgs &d = s->d;
  int st = 0;
  d.ckpt_interval = K; /* (the rest of DeviceArgs starts zeroed: no slots, no pools, no counters) */
  d.ckpt_cap = psd::lat::LDS_CAP;
  s->resume_t.assign((size_t)n_problems, 0);
  if ((st = dev_alloc(s, &s->d_order_sub, (size_t)n_problems))) return st;
  if (park) {
    if ((st = dev_alloc(s, &s->d_resume, (size_t)n_problems))) return st;
    HIP_TRY(hipMemset(s->d_resume, 0, sizeof(int) * (size_t)n_problems));
    d.prob_resume = s->d_resume;
  }
  if (K > 0 || park) {
    const size_t cap = (size_t)d.ckpt_cap;
    const size_t slots = K > 0 ? (size_t)(ckpt_slots > 0 ? ckpt_slots : 1) : (size_t)n_problems;
    if ((st = dev_alloc(s, &d.ckpt_f64, slots * (6 + 12 * cap))) ||
        (st = dev_alloc(s, &d.ckpt_i32, slots * (8 + 2 * cap))) ||
        (st = dev_alloc(s, &d.ckpt_ovf_next, (size_t)1)) ||
        /* checkpoints of functions with more than ckpt_cap pieces (adversarial data):
         * PEAKSEG_HIP_CKPT_OVERFLOW pieces to start with (default 2^18 = 13 MB), four times as
         * many and a rerun whenever that proves too small */
        (st = alloc_ckpt_overflow(s, env_bytes("PEAKSEG_HIP_CKPT_OVERFLOW")
                                         ? env_bytes("PEAKSEG_HIP_CKPT_OVERFLOW")
                                         : (K > 0 ? (1ull << 18) : (1ull << 16)))))
      return st;
  }
  /* spill pool for functions that outgrow LDS (adversarial data): PEAKSEG_HIP_SPILL_CAP pieces
   * per list (default 16384, at most 32767: the interval table packs two indices into an int;
   * 0 disables spilling), PEAKSEG_HIP_SPILL_SLOTS slots to start with (default 16; the pool is
   * grown and the set rerun when more problems spill at once) */
  int cap = 16384;
  if (const char *e = getenv("PEAKSEG_HIP_SPILL_CAP")) cap = atoi(e);
  if (cap > psd::SPILL_CAP_MAX) cap = psd::SPILL_CAP_MAX;
  if (cap <= psd::lat::LDS_CAP) cap = 0;
  d.spill_cap = cap;
  int slots = 16;
  if (const char *e = getenv("PEAKSEG_HIP_SPILL_SLOTS")) slots = atoi(e);
  if ((st = alloc_spill(s, slots))) return st;
#ifdef PSD_PROFILE
  if ((st = dev_alloc(s, &d.prof, (size_t)n_problems * 2 * psd::N_PROF))) return st;
#endif
  return 0;
}

/* arena: the reference's store holds 2 functions per data point with, on typical coverage
 * data, 2-14 pieces each.  Sized from that estimate
 * (PEAKSEG_HIP_PIECES_PER_FUNCTION, default 7: growth is cheap, memory is not), never beyond
 * nine tenths of what is free on the device or what PEAKSEG_HIP_MAX_BYTES allows; solve()
 * maps more and resumes the parked problems if one reports PST_ARENA_FULL. */
int create_arena(psd_problem_set *s, unsigned long long arena_pieces, CreateLaps &lap) {
  const int K = s->ckpt_interval;
  /* pieces per stored function the arena is first sized for.  Typical coverage data needs 2-14
   * (the 1e6 x 64 grid: 5.2 on average); an estimate that proves too small costs one more
   * launch, not a repeated solve (the arena grows in place, parked problems go on), so the
   * default no longer has to be generous: 7 instead of rounds 1-2's 16. */
  double per_fn = 7.0;
  bool per_fn_given = false;
  if (const char *e = getenv("PEAKSEG_HIP_PIECES_PER_FUNCTION")) {
    double v = atof(e);
    if (v >= 1.0) {
      per_fn = v;
      per_fn_given = true;
    }
  }
  s->arena_auto = arena_pieces == 0;
  unsigned long long want = arena_pieces, first_limit = 0;
  if (K > 0) {
    /* one region per chain and problem: the records of K + 1 data points */
    /* The checkpointed store cannot park: a block whose records outgrow the region during the
     * decoding's recomputation costs the problem a second solve from its first data point
     * (measured with 14 per function: 42 of the 1536 problems of the scaled config 4, all at
     * large penalties, the set's time doubled).  So this estimate stays generous -- 32 per
     * function, the longest functions of the 1e6-1e7 grids have 25-27 -- and costs little:
     * regions are (K + 1) functions per chain, not the whole contig. */
    s->ckpt_pieces_per_fn = per_fn_given ? (unsigned long long)(per_fn * 2.0) : 32ull;
    if (s->ckpt_pieces_per_fn < 8) s->ckpt_pieces_per_fn = 8;
    s->d.ckpt_region = (unsigned long long)(K + 1) * s->ckpt_pieces_per_fn;
    want = s->d.ckpt_region * 2ull * (unsigned long long)s->n_problems;
    s->arena_auto = true;
  } else if (s->arena_auto) {
    want = (unsigned long long)((double)s->dp_bins * 2.0 * per_fn);
    unsigned long long fit = arena_fit(s);
    if (want > fit) want = fit;
    first_limit = fit;
  }
  if (s->max_bytes && s->bytes + want * 20ull > s->max_bytes) {
    set_error("problem set needs %llu bytes, PEAKSEG_HIP_MAX_BYTES allows %llu",
              s->bytes + want * 20ull, s->max_bytes);
    return ERROR_DEVICE_MEMORY;
  }
  /* Full store sized by the library: the arena grows WHILE the kernel runs (the host maps blocks
   * ahead of what the waves have taken, solve()), so only the first few blocks are mapped here
   * -- getting memory costs 13-35 ms per GB on a GPU whose memory has been used before, and
   * that time now passes under the kernel instead of in front of it.  The estimate still picks
   * the chunk and block sizes.  PEAKSEG_HIP_NO_LIVE_GROWTH=1: everything the estimate asks for
   * is mapped here, and a solve that needs more parks, grows and resumes (as round 3 did). */
  s->live_growth = K == 0 && s->arena_auto && !getenv("PEAKSEG_HIP_NO_LIVE_GROWTH");
  lap("park slots, pools");
  return alloc_arena(s, want, first_limit, s->live_growth);
}

/* the device's size, the two streams, the events and the pinned word of the mixed launch */
int create_streams(psd_problem_set *s) {
  if (hipDeviceGetAttribute(&s->n_cu, hipDeviceAttributeMultiprocessorCount, s->device) != hipSuccess ||
      s->n_cu <= 0)
    s->n_cu = 256;
  /* Streams that do NOT synchronise with the null stream: the virtual-memory calls that add an
   * arena block while a kernel runs wait for every stream the null stream waits for -- with
   * blocking streams the host would wait for the kernel that waits for the host (measured:
   * waves stalled for seconds until their bound, tools/vmm_block_probe.cpp cases F and G).
   * Nothing here relies on the null stream's implicit ordering: copies are either enqueued
   * on these streams or synchronous and issued after hipStreamSynchronize. */
#ifdef PSD_EMU
  hipError_t e = hipStreamCreate(&s->stream);
  if (e == hipSuccess) e = hipStreamCreate(&s->stream2);
#else
  hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
  if (e == hipSuccess) {
    /* the latency-build part of a mixed launch must get its CUs before the packed part does */
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    e = hipStreamCreateWithPriority(&s->stream2, hipStreamNonBlocking, hi);
  }
#endif
  if (e == hipSuccess) e = hipEventCreate(&s->ev2);
  if (e == hipSuccess)
    e = hipHostMalloc((void **)&s->started, sizeof(int), hipHostMallocCoherent | hipHostMallocMapped);
  for (auto &ev : s->ev)
    if (e == hipSuccess) e = hipEventCreate(&ev);
  if (e != hipSuccess) {
    set_error("stream/event creation failed: %s", hipGetErrorString(e));
    return ERROR_DEVICE_SOLVER;
  }
  s->results.resize((size_t)s->n_problems);
  /* the set's streams do not synchronise with the null stream (hipStreamNonBlocking, so that
   * arena blocks can be mapped under a running kernel): whatever the creation put on the null
   * stream -- the memsets of the tables above may return before they have run -- is complete
   * before a solve launches anything */
  if ((e = hipStreamSynchronize((hipStream_t) nullptr)) != hipSuccess) {
    set_error("creating the problem set: %s", hipGetErrorString(e));
    return ERROR_DEVICE_SOLVER;
  }
  return 0;
}

/* What both creators share, from the point where the contigs' data is known: store, tables,
 * arena, park slots, streams.  The contig data is either host arrays to upload (count, weight) or
 * arrays the dense encoder left in HBM (s->d.count, s->d.weight already set; count == nullptr).
 * Destroys the set when it fails. */
int create_common(SetOwner set, CreateLaps &lap, const std::vector<double> &min_lm,
                  const std::vector<double> &max_lm, const std::vector<int> *count,
                  const std::vector<int> *weight, const int *problem_contig,
                  const double *problem_penalty, unsigned long long arena_pieces,
                  psd_problem_set **out) {
  psd_problem_set *s = set.get();
  for (int p = 0; p < s->n_problems; p++) {
    int c = problem_contig[p];
    if (c < 0 || c >= s->n_contigs) {
      set_error("problem %d names contig %d", p, c);
      return ERROR_DEVICE_SOLVER;
    }
    s->dp_bins += s->contig_n[(size_t)c];
  }
  choose_store(s, arena_pieces);
  long long ckpt_slots = 0;
  int st = 0;
  if ((st = create_tables(s, min_lm, max_lm, count, weight, problem_contig, problem_penalty, &ckpt_slots)))
    return st;
  lap("upload, tables");
  if ((st = create_pools(s, ckpt_slots)) || (st = create_arena(s, arena_pieces, lap))) return st;
  lap("first arena blocks");
  if ((st = create_streams(s))) return st;
  lap("streams, events");
  *out = set.release();
  return 0;
}

}  // namespace

extern "C" int peakseg_hip_problem_set_create(int device, int n_contigs, const int *contig_n_bins,
                                              const int *const *contig_count,
                                              const int *const *contig_weight, int n_problems,
                                              const int *problem_contig,
                                              const double *problem_penalty,
                                              unsigned long long arena_pieces,
                                              psd_problem_set **out) {
  *out = nullptr;
  if (peakseg_hip_device_count() <= device) {
    set_error("no HIP device %d visible (this library has no CPU fallback)", device);
    return ERROR_NO_HIP_DEVICE;
  }
  if (n_contigs <= 0 || n_problems <= 0) {
    set_error("empty problem set");
    return ERROR_DEVICE_SOLVER;
  }
  HIP_TRY(hipSetDevice(device));
  CreateLaps lap;
  SetOwner set(new psd_problem_set(), peakseg_hip_problem_set_destroy);
  psd_problem_set *s = set.get();
  s->device = device;
  s->n_contigs = n_contigs;
  s->n_problems = n_problems;
  std::vector<int> count, weight;
  std::vector<double> min_lm(n_contigs), max_lm(n_contigs);
  long long off = 0;
  for (int c = 0; c < n_contigs; c++) {
    int n = contig_n_bins[c];
    if (n <= 0 || n >= (1 << 30)) {
      set_error("contig %d has %d bins", c, n);
      return ERROR_DEVICE_SOLVER;
    }
    s->contig_n.push_back(n);
    s->contig_off.push_back(off);
    off += n;
    count.insert(count.end(), contig_count[c], contig_count[c] + n);
    weight.insert(weight.end(), contig_weight[c], contig_weight[c] + n);
    double mn = INFINITY, mx = -INFINITY;
    long long width_sum = 0;
    for (int i = 0; i < n; i++) { /* drv:198-204 */
      double log_data = psd_log((double)contig_count[c][i]);
      if (log_data < mn) mn = log_data;
      if (mx < log_data) mx = log_data;
      width_sum += contig_weight[c][i];
    }
    /* (the kernels divide by cumulated widths with the hardware's division, which is the IEEE
     * quotient for whole-number divisors below 2^48, peakseg_detmath.h; chromosome coordinates
     * are 32-bit, so this never triggers on a bedGraph file) */
    if (width_sum >= (1ll << 48)) {
      set_error("contig %d: the bin widths sum to 2^48 or more", c);
      return ERROR_DEVICE_SOLVER;
    }
    min_lm[c] = mn;
    max_lm[c] = mx;
    s->contig_bases.push_back(width_sum);
  }
  lap("gather contigs, log range");
  return create_common(std::move(set), lap, min_lm, max_lm, &count, &weight, problem_contig,
                       problem_penalty, arena_pieces, out);
}
