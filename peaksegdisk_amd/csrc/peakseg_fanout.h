/* peakseg_fanout.h -- the dynamic programs of a file-level call on the devices: one problem set on
 * one device from creation to destruction (solve_on_device), and PEAKSEG_HIP_DEVICES: work dealt
 * to one shard per listed device, one host thread per shard (deal_lpt, run_shards, solve_shards).
 * The per-thread state of a shard is in peakseg_devices.h. */
namespace {

/* the device programs of a call: contigs (pointers into the caller's parsed coverage, not
 * copies) and (contig, penalty) problems */
struct DevicePrograms {
  std::vector<int> contig_n, prob_contig;
  std::vector<const int *> cnt_ptr, wt_ptr;
  std::vector<double> prob_pen;
};

/* one problem's results, copied off the device */
struct DpFetched {
  int status = 0;
  psd_result r{};
  std::vector<int> seg_start;
  std::vector<double> seg_mean;
};

void fetch_dp(int dp_index, psd_problem_set *set, DpFetched &f) {
  if (peakseg_hip_problem_set_result(set, dp_index, &f.r) != 0 || f.r.status != 0) {
    f.status = ERROR_DEVICE_SOLVER;
    return;
  }
  f.seg_start.resize((size_t)f.r.n_segments);
  f.seg_mean.resize((size_t)f.r.n_segments);
  if (peakseg_hip_problem_set_segments(set, dp_index, f.r.n_segments, f.seg_start.data(),
                                       f.seg_mean.data()) != f.r.n_segments)
    f.status = ERROR_DEVICE_SOLVER;
}

/* the phases of a file-level call on stderr (PEAKSEG_HIP_TIMING=1) */
struct Lap {
  const bool on = timing_on();
  double t_mark = wall_now();
  void operator()(const char *what) {
    if (!on) return;
    const double now = wall_now();
    fprintf(stderr, "peakseg_hip timing: %-28s %8.3f s\n", what, now - t_mark);
    t_mark = now;
  }
};

/* All of `progs` in one problem set on `device`: create, solve, results into
 * fetched[0 .. problems), destroy.  The three phases are added to `clock` and, where the caller
 * has one, reported as laps.  Returns true when any problem failed. */
bool solve_on_device(int device, const DevicePrograms &progs, DpFetched *fetched, ShardClock &clock,
                     Lap *lap) {
  double t = wall_now();
  auto phase = [&](double &seconds, const char *what) {
    seconds += wall_now() - t;
    t = wall_now();
    if (lap) (*lap)(what);
  };
  const size_t P = progs.prob_contig.size();
  psd_problem_set *set = nullptr;
  int st = peakseg_hip_problem_set_create(device, (int)progs.contig_n.size(), progs.contig_n.data(),
                                          progs.cnt_ptr.data(), progs.wt_ptr.data(), (int)P,
                                          progs.prob_contig.data(), progs.prob_pen.data(), 0, &set);
  phase(clock.create_s, "upload + allocate");
  if (st == 0) {
    st = peakseg_hip_problem_set_solve(set, nullptr, nullptr);
    if (st == ERROR_DEVICE_SOLVER) st = 0; /* per-problem statuses decide below */
  }
  phase(clock.solve_s, "kernel");
  /* results leave the device one problem after the other; the text files (the segment tables
   * of a penalty grid are hundreds of MB) are formatted later, by a few threads */
  bool failed = st != 0;
  for (size_t k = 0; k < P; k++) {
    if (st) {
      fetched[k].status = st;
    } else {
      fetch_dp((int)k, set, fetched[k]);
    }
    failed = failed || fetched[k].status != 0;
  }
  if (set) peakseg_hip_problem_set_destroy(set);
  phase(clock.fetch_s, "download results + free");
  clock.programs += (int)P;
  return failed;
}

/* Longest-processing-time-first dealing, as parallel.shard_problems: by cost descending (ties
 * by index), each item to the least-loaded shard (ties by shard index); each shard ascending. */
std::vector<std::vector<int>> deal_lpt(const std::vector<double> &cost, int n_shards) {
  std::vector<int> order(cost.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = (int)i;
  std::sort(order.begin(), order.end(), [&](int a, int b) {
    return cost[(size_t)a] != cost[(size_t)b] ? cost[(size_t)a] > cost[(size_t)b] : a < b;
  });
  std::vector<double> load((size_t)n_shards, 0.0);
  std::vector<std::vector<int>> shards((size_t)n_shards);
  for (int i : order) {
    size_t r = 0;
    for (size_t k = 1; k < load.size(); k++)
      if (load[k] < load[r]) r = k;
    shards[r].push_back(i);
    load[r] += cost[(size_t)i];
  }
  for (auto &s : shards) std::sort(s.begin(), s.end());
  return shards;
}

/* what a shard thread leaves for the calling thread */
struct ShardResult {
  bool failed = false;
  std::string error, warning;
  ShardClock clock;
};

/* work(s) for every non-empty shard s, each on a host thread of its own pinned to devices[s];
 * the calling thread prints their text while it waits.  Afterwards the calling thread reports
 * the first failing shard's error and the first warning, in shard order, and the fan-out. */
template <class Work>
void run_shards(const std::vector<int> &devices, const std::vector<std::vector<int>> &shards,
                std::vector<ShardResult> &results, Work work) {
  const size_t S = devices.size();
  results.assign(S, ShardResult());
  ShardText text;
  text.buf.resize(S);
  std::vector<std::thread> threads;
  for (size_t s = 0; s < S; s++) {
    if (shards[s].empty()) continue;
    text.running++;
    threads.emplace_back([&, s]() {
      g_shard_text = &text;
      g_shard_index = (int)s;
      g_shard_device = devices[s];
      g_shard_clock = &results[s].clock;
      work((int)s);
      results[s].error = g_last_error;
      results[s].warning = g_last_warning;
      g_shard_clock = nullptr;
      g_shard_device = -1;
      g_shard_text = nullptr;
      text.shard_done();
    });
  }
  text.drain();
  for (auto &th : threads) th.join();
  bool have_error = false, have_warning = false;
  g_last_warning.clear();
  for (size_t s = 0; s < S; s++) {
    if (results[s].failed && !have_error) {
      g_last_error = results[s].error;
      have_error = true;
    }
    if (!results[s].warning.empty() && !have_warning) {
      g_last_warning = results[s].warning;
      have_warning = true;
    }
  }
  g_fanout.device = devices;
  g_fanout.programs.clear();
  g_fanout.seconds.clear();
  for (size_t s = 0; s < S; s++) {
    g_fanout.programs.push_back(results[s].clock.programs);
    g_fanout.seconds.push_back(results[s].clock.seconds());
    if (timing_on())
      fprintf(stderr, "peakseg_hip timing: shard %zu on device %d: %d programs, create %.3f s, "
                      "solve %.3f s, fetch %.3f s\n", s, devices[s], results[s].clock.programs,
              results[s].clock.create_s, results[s].clock.solve_s, results[s].clock.fetch_s);
  }
}

/* solve_files under PEAKSEG_HIP_DEVICES: the device programs (first appearance order) dealt to
 * one shard per listed device by predicted cost -- bins x the default ramp of
 * parallel.predicted_cost over the program's penalty rank -- and each shard's programs solved in
 * a problem set of its own that uploads only its own contigs.  The set lives under its device's
 * mutex, so the shards of distinct devices run concurrently and those of one device one after the
 * other.  Results land in fetched[program]; returns the shard of each program. */
std::vector<int> solve_shards(const std::vector<int> &devices, const DevicePrograms &all,
                              std::vector<DpFetched> &fetched) {
  const size_t P = all.prob_contig.size();
  std::vector<double> pens(all.prob_pen);
  std::sort(pens.begin(), pens.end());
  pens.erase(std::unique(pens.begin(), pens.end()), pens.end());
  const double span = std::max(1.0, (double)pens.size() - 1.0);
  std::vector<double> cost(P);
  for (size_t k = 0; k < P; k++) {
    const double rank =
        (double)(std::lower_bound(pens.begin(), pens.end(), all.prob_pen[k]) - pens.begin());
    cost[k] = (double)all.contig_n[(size_t)all.prob_contig[k]] * (19000.0 + 9000.0 * rank / span);
  }
  const std::vector<std::vector<int>> shards = deal_lpt(cost, (int)devices.size());
  std::vector<int> shard_of(P, -1);
  for (size_t s = 0; s < shards.size(); s++)
    for (int k : shards[s]) shard_of[(size_t)k] = (int)s;
  std::vector<ShardResult> results;
  run_shards(devices, shards, results, [&](int s) {
    const std::vector<int> &mine = shards[(size_t)s];
    DevicePrograms own;
    std::vector<int> local_of(all.contig_n.size(), -1);
    for (int k : mine) {
      const size_t c = (size_t)all.prob_contig[(size_t)k];
      if (local_of[c] < 0) {
        local_of[c] = (int)own.contig_n.size();
        own.contig_n.push_back(all.contig_n[c]);
        own.cnt_ptr.push_back(all.cnt_ptr[c]);
        own.wt_ptr.push_back(all.wt_ptr[c]);
      }
      own.prob_contig.push_back(local_of[c]);
      own.prob_pen.push_back(all.prob_pen[(size_t)k]);
    }
    std::vector<DpFetched> got(mine.size());
    {
      std::lock_guard<std::mutex> hold(device_mutex(devices[(size_t)s]));
      results[(size_t)s].failed =
          solve_on_device(devices[(size_t)s], own, got.data(), results[(size_t)s].clock, nullptr);
    }
    for (size_t j = 0; j < mine.size(); j++) fetched[(size_t)mine[j]] = std::move(got[j]);
  });
  return shard_of;
}

}  // namespace
