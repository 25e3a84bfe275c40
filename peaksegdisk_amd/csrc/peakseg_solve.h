/* peakseg_solve.h -- one solve of a problem set: closed forms of trivial models, the planner, one
 * launch and what it left, the growth policies, peakseg_hip_problem_set_solve. */
namespace {

/* The reference solves these without a dynamic program (drv:224-243): penalty +Inf, or a contig
 * whose counts are all equal.  Only sets made from dense counts know the second without the
 * caller's help; the file path takes the same branch before it creates a set. */
bool trivial_model(const psd_problem_set *s, int p) {
  if (!s->dense) return false;
  return s->prob_penalty[(size_t)p] == INFINITY ||
         s->contig_constant[(size_t)s->prob_contig[(size_t)p]] != 0;
}

/* best_cost of the one-segment model (write_trivial in peakseg_files.h, drv:225-231) */
double trivial_best_cost(const psd_problem_set *s, int c) {
  const double cum_weighted_count = (double)s->contig_sum[(size_t)c];
  const double cum_weight = (double)s->contig_bases[(size_t)c];
  if (cum_weighted_count == 0) return 0;
  return cum_weighted_count * (1 - psd_log(cum_weighted_count) + psd_log(cum_weight));
}

/* results and one-row segment tables of the set's trivial models (copies, no launch) */
int serve_trivial_models(psd_problem_set *s) {
  for (int p = 0; p < s->n_problems; p++) {
    if (!trivial_model(s, p)) continue;
    const int c = s->prob_contig[(size_t)p];
    const double cum_weight = (double)s->contig_bases[(size_t)c];
    psd::ProbResult r{};
    r.best_cost = trivial_best_cost(s, c) / cum_weight;
    r.n_segments = 1;
    r.step_reached = s->contig_n[(size_t)c];
    s->results[(size_t)p] = r;
    const int start = -1;
    const double mean = (double)s->contig_sum[(size_t)c] / cum_weight;
    const long long off = s->prob_seg_off[(size_t)p];
    HIP_TRY(hipMemcpyAsync(s->d.seg_start + off, &start, sizeof start, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->d.seg_mean + off, &mean, sizeof mean, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream)); /* (the sources are locals) */
  }
  return 0;
}

/* what the mixed-launch planner assumes a problem advances at, refreshed by every solve that
 * ran on one build alone with every problem resident from the start (a clean measurement).
 * Defaults: an MI355X on contigs of 1e5-1e6 bins -- 96 k data points/s on the latency build;
 * 63 k on the throughput build with the chip full, 75 k with a CU to itself
 * (profiles/r04/thr_rate_long_contigs.log; rounds 2-3 assumed 27 k, the round-2 build's rate),
 * taken a little low: a problem the planner leaves on the throughput build must not end after
 * the longest one on the latency build. */
std::atomic<double> g_lat_rate{96e3}, g_thr_rate{58e3};
/* a problem on the packed build (a SIMD shared three ways) against one on the throughput build
 * (two ways): 6144 equal problems ran 18.2 % faster six to a CU than four to a CU */
constexpr double PK_RATE_OF_THR = 1.182 * 4.0 / 6.0;
/* The planner cannot know how long a set's functions get.  When the packed build had to hand
 * more than one problem in twenty to the wider builds (each of them waited for the end of the
 * first launch before it went on), this process's later sets -- more of the same data, as a
 * rule -- are planned without it. */
std::atomic<int> g_pk_handed_over_many{0};

/* what the environment and this process's earlier solves tell the planner, read once per solve */
struct PlanKnobs {
  const char *variant = getenv("PEAKSEG_HIP_VARIANT");
  /* data points per second of one problem on either build: measured by this process's own
   * earlier solves when there were any (g_lat_rate / g_thr_rate), else the figures of
   * an MI355X at 2.4 GHz */
  double lat_rate = g_lat_rate.load(), thr_rate = g_thr_rate.load();
  bool no_packed = getenv("PEAKSEG_HIP_NO_PACKED") || g_pk_handed_over_many.load();
  bool timing = timing_on();
  PlanKnobs() {
    if (const char *e = getenv("PEAKSEG_HIP_RATES")) { /* diagnostic: "lat,thr" data points per s */
      double a = 0.0, b = 0.0;
      if (sscanf(e, "%lf,%lf", &a, &b) == 2 && a > 0.0 && b > 0.0) lat_rate = a, thr_rate = b;
    }
  }
};

/* The builds of one solve, from the lengths of the contigs of its problems in launch order
 * (longest first).  No device is touched. */
SolvePlan plan_solve(const std::vector<double> &len, int n_cu, bool can_park, const PlanKnobs &k) {
  const int n_run = (int)len.size();
  SolvePlan pl;
  /* the latency build wants a CU per problem: beyond that, problems would queue behind each
   * other and a build that packs several problems on a CU (throughput: 4, packed: 6) finishes
   * the set sooner.  PEAKSEG_HIP_VARIANT=lat|thr|pk overrides (tests, A/B runs). */
  pl.throughput = n_run > n_cu;
  if (const char *e = k.variant) {
    if (!strcmp(e, "lat")) pl.throughput = false, pl.forced = true;
    if (!strcmp(e, "thr")) pl.throughput = true, pl.forced = true;
    if (!strcmp(e, "pk")) pl.throughput = true, pl.packed = true, pl.forced = true;
  }
  /* the packed build hands functions of more than 40 pieces to the throughput build through
   * the park slots; without them (checkpointed store, very large sets) it is not used */
  if (pl.packed && !can_park) pl.packed = false;
  /* Mixed launch for sets of unequal contigs that oversubscribe the chip: a problem on the
   * throughput build advances about 60 k data points per second, on the latency build (a CU of
   * its own) about 96 k, so the longest problems would decide when the set ends.  The L longest
   * problems go to the latency build -- launched first, on a stream of its own, one CU each --
   * and the rest is packed on what is left; L minimises the later of the two predicted ends.
   * (Equal contigs: L = 0.)  The same prediction chooses between the throughput and the packed
   * build for the rest: six problems per CU at 0.79 of the speed each (measured on 6144 equal
   * problems: +18 %; on 24 unequal contigs x 64 penalties, which end with their longest packed
   * problems: -10 %, profiles/r04/ab_thr_occupancy_*.log). */
  if (!pl.throughput || pl.forced) return pl;
  const double lat_rate = k.lat_rate, thr_rate = k.thr_rate;
  double rest = 0.0;
  for (int i = 0; i < n_run; i++) rest += len[(size_t)i];
  const int l_max = std::max(0, n_cu - 16 < n_run ? n_cu - 16 : n_run - 1);
  /* the predicted end of the set with problems [0, l) on the latency build and [l, n) packed
   * per_cu to a CU at `rate` each, minimised over l */
  auto plan = [&](double per_cu, double rate, int &best_l) -> double {
    double best = 1e300, sum_lat = 0.0;
    best_l = 0;
    for (int l = 0; l <= l_max; l++) {
      const double t_lat = l > 0 ? len[0] / lat_rate : 0.0;
      const double cus = (double)(n_cu - l);
      const double t_work = (rest - sum_lat) / (cus * per_cu * rate);
      const double t_long = len[(size_t)l] / rate;
      const double t = std::max(t_lat, std::max(t_work, t_long));
      if (t < best * 0.98) { /* prefer fewer latency problems unless it clearly pays */
        best = t;
        best_l = l;
      }
      sum_lat += len[(size_t)l];
    }
    return best;
  };
  int l_thr = 0, l_pk = 0;
  const double t_thr = plan(4.0, thr_rate, l_thr);
  const double t_pk = plan(6.0, thr_rate * PK_RATE_OF_THR, l_pk);
  pl.packed = can_park && !k.no_packed && t_pk < 0.97 * t_thr;
  pl.n_lat_mixed = pl.packed ? l_pk : l_thr;
  if (k.timing) {
    const int L = pl.n_lat_mixed;
    const double per_cu = pl.packed ? 6.0 : 4.0;
    const double rate = pl.packed ? thr_rate * PK_RATE_OF_THR : thr_rate;
    double on_lat = 0.0;
    for (int i = 0; i < L; i++) on_lat += len[(size_t)i];
    fprintf(stderr, "peakseg_hip timing: plan: %d problems, %d on the latency build (predicted end "
                    "%.2f s), the rest %s (work %.2f s, longest %.2f s); rates %.0f / %.0f per s; "
                    "all on thr %.2f s, all on pk %.2f s\n", n_run, L,
            L > 0 ? len[0] / lat_rate : 0.0, pl.packed ? "pk" : "thr",
            (rest - on_lat) / ((double)(n_cu - L) * per_cu * rate), len[(size_t)L] / rate,
            lat_rate, thr_rate, t_thr, t_pk);
  }
  return pl;
}

enum Build { BUILD_LAT, BUILD_THR, BUILD_PK };
struct ForwardKernel {
  void (*fn)(psd::DeviceArgs);
  int threads;
};

/* the forward kernel of a build, [1]: for the checkpointed store (which has no pk kernel) */
const ForwardKernel FORWARD_KERNEL[3][2] = {
    {{psd::lat::fpop_forward_kernel, psd::lat::FORWARD_THREADS},
     {psd::lat::fpop_forward_ckpt_kernel, psd::lat::FORWARD_THREADS}},
    {{psd::thr::fpop_forward_kernel, psd::thr::FORWARD_THREADS},
     {psd::thr::fpop_forward_ckpt_kernel, psd::thr::FORWARD_THREADS}},
    {{psd::pk::fpop_forward_kernel, psd::pk::FORWARD_THREADS},
     {psd::thr::fpop_forward_ckpt_kernel, psd::thr::FORWARD_THREADS}}};

/* the build a launch of n_todo problems runs on (of a mixed launch: its packed part) */
Build launch_build(const SolvePlan &pl, bool relaunch, int n_todo, int n_cu) {
  if (!relaunch) return !pl.throughput ? BUILD_LAT : pl.packed ? BUILD_PK : BUILD_THR;
  /* (a relaunch after the packed build: the problems it parked need the wider lists of the
   * throughput build, or a CU each when they are few; it holds what the packed build handed
   * over and never runs on it) */
  const bool thr_now = (pl.forced && !pl.packed) ? pl.throughput : n_todo > n_cu;
  return thr_now ? BUILD_THR : BUILD_LAT;
}

void enqueue_forward(psd_problem_set *s, Build b, hipStream_t stream, const psd::DeviceArgs &a) {
  const ForwardKernel &k = FORWARD_KERNEL[b][s->ckpt_interval > 0];
  hipLaunchKernelGGL(k.fn, dim3((unsigned)a.n_problems), dim3((unsigned)k.threads), 0, stream, a);
}

/* Mixed launch: the L longest problems on the latency build (stream2), the rest on `rest_build`;
 * both kernels index prob_order by their own blockIdx.x.  *ev_packed_end (diagnostic,
 * PEAKSEG_HIP_TIMING): records the end of the packed part. */
int enqueue_mixed(psd_problem_set *s, Build rest_build, const int *d_order, int n_run,
                  hipEvent_t *ev_packed_end) {
  const int L = s->run.plan.n_lat_mixed;
  psd::DeviceArgs d_lat = s->d, d_thr = s->d;
  d_lat.n_problems = L;
  d_lat.prob_order = d_order;
  d_thr.n_problems = n_run - L;
  d_thr.prob_order = d_order + L;
  HIP_TRY(hipStreamWaitEvent(s->stream2, s->ev[0], 0));
  /* A latency-build workgroup needs every register of a CU: once the packed part has put
   * a workgroup on each CU it would find none free before the packed part has drained,
   * and the two kernels would run one after the other.  So its workgroups report in (one
   * system-scope atomic each, on a pinned host word) and the packed part is launched when
   * all of them have started -- or after half a second, whatever they are waiting for. */
  __atomic_store_n(s->started, 0, __ATOMIC_RELEASE);
  d_lat.started = s->started;
  enqueue_forward(s, BUILD_LAT, s->stream2, d_lat);
  HIP_TRY(hipGetLastError());
  (void)hipStreamQuery(s->stream2); /* submit now */
  if (!s->mixed_wait_timed_out) { /* later solves after a time-out do not wait again */
    const auto t0 = std::chrono::steady_clock::now();
    while (__atomic_load_n(s->started, __ATOMIC_ACQUIRE) < L &&
           std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(500))
      std::this_thread::yield();
    if (__atomic_load_n(s->started, __ATOMIC_ACQUIRE) < L) {
      s->mixed_wait_timed_out = true;
      set_warning("mixed launch: %d of %d latency-build workgroups had not started after 0.5 s; "
                  "the packed part was launched anyway",
                  L - __atomic_load_n(s->started, __ATOMIC_ACQUIRE), L);
    }
  }
  enqueue_forward(s, rest_build, s->stream, d_thr);
  HIP_TRY(hipGetLastError());
  if (timing_on() && !*ev_packed_end && hipEventCreate(ev_packed_end) != hipSuccess)
    *ev_packed_end = nullptr;
  if (*ev_packed_end) HIP_TRY(hipEventRecord(*ev_packed_end, s->stream));
  HIP_TRY(hipEventRecord(s->ev2, s->stream2));
  HIP_TRY(hipStreamWaitEvent(s->stream, s->ev2, 0));
  return 0;
}

/* One launch of the problems `todo` (launch order: longest contig first) and the wait for its
 * end; a relaunch holds the unfinished problems of the launch before.  Adds its kernel time to
 * *total_ms. */
int run_launch(psd_problem_set *s, const std::vector<int> &todo, bool relaunch, const int *d_order,
               int n_run, float *total_ms) {
  if (s->ckpt_interval > 0) {
    const unsigned long long B = 1ull << s->d.ar_block_log2;
    const unsigned long long per_block = s->d.ckpt_region ? B / s->d.ckpt_region : 0ull;
    const unsigned long long n_regions = 2ull * (unsigned long long)s->n_problems;
    if (per_block == 0 || s->arena_blocks.size() < (n_regions + per_block - 1) / per_block) {
      set_error("checkpointed store: arena of %llu pieces is smaller than its %d regions of %llu",
                s->d.ar_cap, 2 * s->n_problems, s->d.ckpt_region);
      return ERROR_DEVICE_MEMORY;
    }
  }
  const int n_todo = (int)todo.size();
  hipEvent_t ev_packed_end = nullptr; /* (diagnostic, PEAKSEG_HIP_TIMING) */
  {
    /* the arena may grow under this launch's kernels; the grower's scope ends after the stream
     * has synchronised and before anything returns from here (its thread works on *s) */
    LiveGrower grower;
    const bool live = s->live_growth && s->ckpt_interval == 0 && s->arena_auto;
    s->d.ar_live = live ? s->h_live : nullptr;
    s->d.ar_used = s->h_used;
    psd::DeviceArgs d_run = s->d;
    d_run.prob_order = d_order;
    d_run.n_problems = n_todo;
    if (relaunch) {
      /* only the unfinished problems, in their original order */
      HIP_TRY(hipMemcpyAsync(s->d_order_sub, todo.data(), sizeof(int) * (size_t)n_todo,
                             hipMemcpyHostToDevice, s->stream));
      d_run.prob_order = s->d_order_sub;
      if (s->can_park)
        HIP_TRY(hipMemcpyAsync(s->d_resume, s->resume_t.data(), sizeof(int) * (size_t)s->n_problems,
                               hipMemcpyHostToDevice, s->stream));
    }
    if (s->ckpt_interval > 0)
      HIP_TRY(hipMemsetAsync(s->d.ar_next_chunk, 0, sizeof(unsigned long long), s->stream));
    HIP_TRY(hipMemsetAsync(s->d.spill_next, 0, sizeof(int), s->stream));
    /* Overflow pool.  Checkpointed store: every relaunched problem starts over and saves its
     * checkpoints again, so the pool starts empty.  Full store: the pool holds the functions of
     * PARKED problems (those longer than a park slot) from the launch that parked them until the
     * workgroup that resumes them has read them back -- which, in a grid larger than the chip
     * holds resident, can be long after other workgroups of the same launch have parked again:
     * the pool is emptied once per solve, never between its launches. */
    if (s->d.ckpt_ovf_next && (s->ckpt_interval > 0 || !relaunch))
      HIP_TRY(hipMemsetAsync(s->d.ckpt_ovf_next, 0, sizeof(unsigned long long), s->stream));
    HIP_TRY(hipMemcpyAsync(const_cast<psd::DeviceArgs *>(s->d.self), &d_run, sizeof(psd::DeviceArgs),
                           hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipEventRecord(s->ev[0], s->stream));
    if (live) grower.start(s, arena_mapped(s) + arena_fit(s));
    const Build build = launch_build(s->run.plan, relaunch, n_todo, s->n_cu);
    if (!relaunch && s->run.plan.throughput && s->run.plan.n_lat_mixed > 0) {
      int st = enqueue_mixed(s, build, d_order, n_run, &ev_packed_end);
      if (st) return st;
    } else {
      enqueue_forward(s, build, s->stream, d_run);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev[1], s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  int st = arena_sync_table(s);
  if (st) return st;
  float f_ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&f_ms, s->ev[0], s->ev[1]));
  *total_ms += f_ms;
  if (ev_packed_end) { /* PEAKSEG_HIP_TIMING: when each part of a mixed launch ended */
    float lat_ms = 0.f, packed_ms = 0.f;
    if (hipEventElapsedTime(&lat_ms, s->ev[0], s->ev2) == hipSuccess &&
        hipEventElapsedTime(&packed_ms, s->ev[0], ev_packed_end) == hipSuccess)
      fprintf(stderr, "peakseg_hip timing: mixed launch: latency part ended at %.2f s, packed part "
                      "at %.2f s\n", lat_ms / 1e3, packed_ms / 1e3);
    (void)hipEventDestroy(ev_packed_end);
  }
  s->run.launches++;
  return 0;
}

/* what a launch's problems ran short of, and which of them have to run again */
struct Unfinished {
  bool arena_full = false, spill_full = false, ckpt_full = false, park_pool_full = false;
  int widen = 0; /* problems the packed build parked because a function outgrew its lists */
  int longest_function = 0;
  std::vector<int> again;
};

/* Fetches what the launch of `todo` left, counts it, and sorts its problems into finished and
 * unfinished (u.again; resume_t: where each of those goes on) */
int collect(psd_problem_set *s, const std::vector<int> &todo, Unfinished &u) {
  /* results of the problems this launch ran (the others keep theirs) */
  std::vector<psd::ProbResult> all((size_t)s->n_problems);
  HIP_TRY(hipMemcpy(all.data(), s->d.result, sizeof(psd::ProbResult) * (size_t)s->n_problems,
                    hipMemcpyDeviceToHost));
  for (int p : todo) {
    const psd::ProbResult &r = all[(size_t)p];
    const int n = s->contig_n[(size_t)s->prob_contig[(size_t)p]];
    const int reached = r.status == 0 ? n : r.step_reached;
    if (reached > s->resume_t[(size_t)p])
      s->run.steps_run += (unsigned long long)(reached - s->resume_t[(size_t)p]);
    s->results[(size_t)p] = r;
  }
  unsigned long long chunks = 0;
  HIP_TRY(hipMemcpy(&chunks, s->d.ar_next_chunk, sizeof chunks, hipMemcpyDeviceToHost));
  s->arena_used = chunks << s->d.ar_chunk_log2;
  if (s->arena_used > s->d.ar_cap) s->arena_used = s->d.ar_cap;
  for (int p : todo) {
    const psd::ProbResult &r = s->results[(size_t)p];
    u.arena_full = u.arena_full || r.status == psd::PST_ARENA_FULL;
    /* out of arena beyond data point 0 and not parked although the set has park slots: its
     * functions were too long for a slot and the overflow pool had no room for them */
    u.park_pool_full = u.park_pool_full || (r.status == psd::PST_ARENA_FULL && s->can_park &&
                                            !r.parked && r.step_reached > 0);
    u.spill_full = u.spill_full || r.status == psd::PST_SPILL_FULL;
    u.ckpt_full = u.ckpt_full || r.status == psd::PST_CKPT_FULL;
    if (r.max_intervals > u.longest_function) u.longest_function = r.max_intervals;
    const bool to_wider = r.status == psd::PST_LDS_OVERFLOW && r.parked && s->can_park;
    if (r.status == psd::PST_ARENA_FULL || r.status == psd::PST_SPILL_FULL ||
        r.status == psd::PST_CKPT_FULL || to_wider) {
      u.again.push_back(p);
      if (r.status == psd::PST_ARENA_FULL && r.parked && s->can_park) s->run.parks++;
      if (to_wider) u.widen++;
      /* parked: go on where it stopped; anything else starts over */
      s->resume_t[(size_t)p] = ((r.status == psd::PST_ARENA_FULL || to_wider ||
                                 r.status == psd::PST_SPILL_FULL) &&
                                r.parked && s->can_park)
                                   ? r.step_reached
                                   : 0;
    }
  }
  if (s->ckpt_interval == 0 && s->d.ckpt_ovf_next) { /* the parks' share of the overflow pool */
    unsigned long long used = 0;
    HIP_TRY(hipMemcpy(&used, s->d.ckpt_ovf_next, sizeof used, hipMemcpyDeviceToHost));
    s->run.park_pool_pieces = used;
  }
  s->run.widened += u.widen;
  return 0;
}

/* Park pool (full store): such problems start over this time; with four times the pool (what
 * other parked problems keep in it is preserved) the next exhaustion parks them */
int grow_park_pool(psd_problem_set *s) {
  const unsigned long long bigger = s->d.ckpt_ovf_cap * 4ull;
  if (bigger > arena_fit(s) * 20ull / 52ull) return 0;
  return grow_ckpt_overflow_keep(s, bigger);
}

/* Checkpoint overflow pool: four times as many pieces, empty (its problems start over) */
int regrow_ckpt_pool(psd_problem_set *s) {
  unsigned long long bigger = s->d.ckpt_ovf_cap * 4ull;
  free_ckpt_overflow(s);
  const unsigned long long fit = arena_fit(s) * 20ull / 52ull;
  if (bigger > fit) {
    set_error("checkpointed store: an overflow pool of %llu pieces does not fit (free HBM / "
              "PEAKSEG_HIP_MAX_BYTES)", bigger);
    return ERROR_DEVICE_MEMORY;
  }
  return alloc_ckpt_overflow(s, bigger);
}

/* more problems spilled at once than the pool has slots: four times the slots */
int regrow_spill_pool(psd_problem_set *s) {
  int slots = s->spill_slots * 4;
  if (s->spill_slots >= s->n_problems) {
    set_error("spill pool exhausted with one slot per problem");
    return ERROR_DEVICE_SOLVER;
  }
  free_spill(s);
  return alloc_spill(s, slots);
}

/* checkpointed store: a block's records outgrew a wave's region -- twice the region,
 * or at once what the longest function of the forward pass asks for (K + 1 functions of
 * that length always fit then) when that is more.  The regions are scratch for the
 * decoding's recomputation: re-allocated, never kept. */
int regrow_ckpt_regions(psd_problem_set *s, int longest_function) {
  const unsigned long long old_ppf = s->ckpt_pieces_per_fn;
  s->ckpt_pieces_per_fn *= 2ull;
  if (s->ckpt_pieces_per_fn < (unsigned long long)longest_function)
    s->ckpt_pieces_per_fn = (unsigned long long)longest_function;
  s->d.ckpt_region = (unsigned long long)(s->ckpt_interval + 1) * s->ckpt_pieces_per_fn;
  const unsigned long long bigger = s->d.ckpt_region * 2ull * (unsigned long long)s->n_problems;
  free_arena(s);
  const unsigned long long fit = arena_fit(s);
  int st = alloc_arena(s, bigger, fit); /* (refuses, never clips, what does not fit) */
  if (st) {
    const std::string why = g_last_error;
    s->ckpt_pieces_per_fn = old_ppf;
    s->d.ckpt_region = (unsigned long long)(s->ckpt_interval + 1) * s->ckpt_pieces_per_fn;
    if (s->arena_blocks.empty() && s->d.ar_block == nullptr)
      (void)alloc_arena(s, s->d.ckpt_region * 2ull * (unsigned long long)s->n_problems, fit);
    g_last_error = why;
  }
  return st;
}

/* Full store: the arena GROWS by whole blocks (problems come here parked when the live
 * growth could not keep up or was switched off).  How much more: what the unfinished
 * problems' progress says the rest of the set needs (pieces handed out so far x data
 * points left / data points done, x 1.3); at least a quarter of what the arena has.
 * arena_rounds: launches of this solve that ran out of arena, this one included. */
int grow_arena(psd_problem_set *s, int arena_rounds, size_t n_again) {
  /* (a problem that could not be parked starts over and stores all its records again;
   * those of its first attempt stay where they are, unused) */
  double done = 0.0, rest = 0.0;
  for (int p = 0; p < s->n_problems; p++) {
    const double n = (double)s->contig_n[(size_t)s->prob_contig[(size_t)p]];
    const psd::ProbResult &r = s->results[(size_t)p];
    done += r.status == 0 ? n : (double)r.step_reached;
    if (r.status != 0) rest += n - (double)s->resume_t[(size_t)p];
  }
  /* (functions that get longer with t -- adversarial counts -- need more per data point
   * the further they get: the linear estimate falls short every time, so from the second
   * exhaustion of a solve on the arena at least doubles) */
  unsigned long long more = arena_rounds >= 2 ? s->arena_pieces : s->arena_pieces / 4ull;
  if (done > 0.0) {
    const double left = (double)(s->d.ar_cap - s->arena_used);
    const double need = (double)s->arena_used / done * rest * 1.3 - left;
    if (need > (double)more) more = (unsigned long long)need;
  }
  /* (at least four chunks for every problem that comes back: a set that ran out with
   * all its problems nearly done estimates less than their next requests take) */
  const unsigned long long fit = arena_fit(s);
  const unsigned long long chunk = 1ull << s->d.ar_chunk_log2;
  const unsigned long long least = chunk * 4ull * (unsigned long long)n_again;
  if (more < least) more = least;
  if (more > fit) more = fit;
  if (more < least) {
    set_error("cost-function arena cannot grow beyond %llu pieces (free HBM / "
              "PEAKSEG_HIP_MAX_BYTES)", s->arena_pieces);
    return ERROR_DEVICE_MEMORY;
  }
  return alloc_arena(s, s->arena_pieces + more, s->arena_pieces + fit);
}

/* the four policies, in this order, for what `u` says was short */
int grow_what_was_short(psd_problem_set *s, const Unfinished &u, int *arena_rounds) {
  int st = 0;
  if (u.park_pool_full && s->ckpt_interval == 0 && (st = grow_park_pool(s))) return st;
  if (u.ckpt_full && (st = regrow_ckpt_pool(s))) return st;
  if (u.spill_full && (st = regrow_spill_pool(s))) return st;
  if (!u.arena_full) return 0;
  if (!s->arena_auto) {
    set_error("cost-function arena of %llu pieces is too small", s->arena_pieces);
    return ERROR_DEVICE_MEMORY;
  }
  if (s->ckpt_interval > 0) return regrow_ckpt_regions(s, u.longest_function);
  return grow_arena(s, ++*arena_rounds, u.again.size());
}

/* What this solve teaches the planner of later ones */
void planner_feedback(const psd_problem_set *s, [[maybe_unused]] int n_run,
                      [[maybe_unused]] float total_ms) {
  const SolvePlan &pl = s->run.plan;
  if (pl.packed && !pl.forced && (long long)s->run.widened * 20 > (long long)s->n_problems)
    g_pk_handed_over_many.store(1);
#ifndef PSD_EMU /* (the emulator's timings say nothing about the hardware) */
  if (s->run.launches == 1 && pl.n_lat_mixed == 0 && s->ckpt_interval == 0 && total_ms > 500.f &&
      n_run == s->n_problems) {
    /* a clean single launch: the longest problem's data points / kernel time is the rate of
     * that build (the throughput build only while every workgroup was resident at once) */
    int longest = 0;
    bool spilled = false;
    for (int p = 0; p < s->n_problems; p++) {
      longest = std::max(longest, s->contig_n[(size_t)s->prob_contig[(size_t)p]]);
      spilled = spilled || s->results[(size_t)p].spill_steps > 0;
    }
    const double rate = (double)longest / ((double)total_ms / 1e3);
    if (!spilled && rate > 1e3 && rate < 1e7) {
      /* latency build: a CU per problem; throughput build: only a chip that was full (four
       * workgroups on nearly every CU) shows the packed rate the planner reasons with */
      if (!pl.throughput && s->n_problems <= s->n_cu) g_lat_rate.store(rate);
      if (pl.throughput && !pl.packed && s->n_problems <= 4 * s->n_cu &&
          s->n_problems >= 7 * s->n_cu / 2)
        g_thr_rate.store(rate);
    }
  }
#endif
}

}  // namespace

/* plan -> reset -> loop { launch, collect, classify, grow } -> feedback -> status */
extern "C" int peakseg_hip_problem_set_solve(psd_problem_set *s, float *forward_ms,
                                             float *backtrack_ms) {
  HIP_TRY(hipSetDevice(s->device));
  g_last_warning.clear();
  /* What is launched: every problem, longest contig first -- but for the trivial models of a set
   * made from dense counts, which have a closed form (n_run == n_problems for every other set). */
  std::vector<int> todo; /* launch order: longest contig first */
  std::vector<double> len; /* ... and the lengths of their contigs */
  for (int p : s->order) {
    if (trivial_model(s, p)) continue;
    todo.push_back(p);
    len.push_back((double)s->contig_n[(size_t)s->prob_contig[(size_t)p]]);
  }
  const int n_run = (int)todo.size();
  const int *d_order_first = s->d.prob_order; /* the first launch's order, on the device */
  int st = 0;
  if (n_run < s->n_problems) {
    if ((st = serve_trivial_models(s))) return st;
    if (n_run > 0)
      HIP_TRY(hipMemcpyAsync(s->d_order_run, todo.data(), sizeof(int) * (size_t)n_run,
                             hipMemcpyHostToDevice, s->stream));
    d_order_first = s->d_order_run;
  }
  s->run = SolveRun();
  /* ... and with it what the other pack_* services packed of the models before: their downloads
   * say "nothing packed" until they are called again (region and coverage stats read no model) */
  s->clusters.clusters = s->clusters.entries = -1;
  s->joint.windows = s->joint.entries = -1;
  s->joint_path.windows = s->joint_path.entries = -1;
  s->joint_labels.labels = -1;
  s->heldout.pairs = -1;
  s->run.plan = plan_solve(len, s->n_cu, s->can_park, PlanKnobs());
  /* Launches.  The first one runs every problem.  When problems come back unfinished for
   * want of room (arena, spill pool, checkpoint overflow pool) the host enlarges what was short
   * and launches THOSE problems again: a problem that ran out of arena was parked by the kernel
   * and goes on at the data point it had reached (the arena grows by a segment, its records
   * stay in place); the others start over.  Finished problems are never computed twice. */
  std::fill(s->resume_t.begin(), s->resume_t.end(), 0);
  if (s->can_park) HIP_TRY(hipMemsetAsync(s->d_resume, 0, sizeof(int) * (size_t)s->n_problems, s->stream));
  HIP_TRY(hipMemsetAsync(s->d.ar_next_chunk, 0, sizeof(unsigned long long), s->stream));
  __atomic_store_n(s->h_used, 0ull, __ATOMIC_RELEASE); /* follows ar_next_chunk */
  float total_ms = 0.f;
  int arena_rounds = 0; /* launches of this solve that ran out of arena */
  for (int attempt = 0; n_run > 0; attempt++) {
    const int n_todo = (int)todo.size();
    if ((st = run_launch(s, todo, attempt > 0, d_order_first, n_run, &total_ms))) return st;
    if (forward_ms) *forward_ms = total_ms;
    if (backtrack_ms) *backtrack_ms = 0.f; /* decoding happens inside the forward kernel */
    Unfinished u;
    if ((st = collect(s, todo, u))) return st;
    if (u.again.empty()) break;
    if (timing_on()) {
      fprintf(stderr, "peakseg_hip timing: launch %d: %d of %d problems unfinished (arena %d, spill "
                      "pool %d, checkpoint pool %d, to wider lists %d):", s->run.launches,
              (int)u.again.size(), n_todo, (int)u.arena_full, (int)u.spill_full, (int)u.ckpt_full,
              u.widen);
      for (size_t k = 0; k < u.again.size() && k < 8; k++)
        fprintf(stderr, " p%d@%d%s", u.again[k], s->results[(size_t)u.again[k]].step_reached,
                s->resume_t[(size_t)u.again[k]] ? "(parked)" : "");
      fprintf(stderr, "\n");
    }
    if (attempt >= 12) {
      set_error("cost-function arena (%llu pieces) / spill pool (%d slots) still too small after "
                "%d relaunches", s->arena_pieces, s->spill_slots, attempt);
      return ERROR_DEVICE_MEMORY;
    }
    if ((st = grow_what_was_short(s, u, &arena_rounds))) return st;
    todo.swap(u.again);
  }
  if (n_run == 0) { /* nothing but closed forms: no launch */
    if (forward_ms) *forward_ms = 0.f;
    if (backtrack_ms) *backtrack_ms = 0.f;
  }
  planner_feedback(s, n_run, total_ms);
  s->solved = true;
  for (int p = 0; p < s->n_problems; p++) {
    const psd::ProbResult &r = s->results[(size_t)p];
    if (r.status == 0) continue;
    set_error("problem %d: kernel status %d (wave error bits %d) at data point %d", p, r.status,
              r.wave_err, r.step_reached);
    return ERROR_DEVICE_SOLVER;
  }
  return 0;
}
