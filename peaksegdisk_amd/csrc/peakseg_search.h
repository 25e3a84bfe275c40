/* peakseg_search.h -- the penalty searches for a target number of peaks, over PeakSegFPOP_dir's
 * protocol (peakseg_dir.h):
 *
 *   place_penalties                  where a round looks besides its secant penalty
 *   PenaltySearch                    the decisions of one directory's search: sequentialSearch_dir's
 *                                    (/root/reference/R/sequentialSearch_dir.R:22-103; f2) with
 *                                    `width` models per round; width 1 is the reference's sequence
 *   search_rounds, search_run        the searches of many directories in lockstep, every round one
 *                                    PeakSegFPOP_dir_batch call; the directories dealt over
 *                                    PEAKSEG_HIP_DEVICES
 *   PeakSegFPOP_sequential_search    width 1 on a resident contig (parsed and uploaded once)
 *   PeakSegFPOP_sequential_search_batch, PeakSegFPOP_parallel_search, _parallel_search_batch
 *                                    argument checks and search_run
 */
namespace {

const int PARALLEL_SEARCH_DEFAULT_WIDTH = 8; /* DESIGN.md section 8 has the A/B */
const int PARALLEL_SEARCH_MAX_WIDTH = 256;

/* Where a round looks besides its secant penalty: a pure function of the bracket rows and the
 * number of penalties wanted, so a search can be replayed.  Between two finite penalties: a
 * ladder of equal steps in log(penalty) from one bracket end to the other.  (Aiming the ladder at
 * the penalty where a straight line in (log penalty, log peaks) reaches the target saved a round
 * on Mono27ac and cost one or two on the synthetic contigs, whose peak counts fall off a cliff
 * and then hardly move: DESIGN.md section 8 has the table.)  An end at 0 or Inf has no logarithm:
 * there the ladder is anchored on the secant penalty, steps by powers of 4 on the open side and
 * by the fractions (j/(n+1))^2 of the log distance on a finite one.  The caller drops what does
 * not survive the 15-digit string strictly inside the bracket. */
void place_penalties(const psd_search_row &under, const psd_search_row &over, double secant,
                     int extras, std::vector<double> &out) {
  const double lo = over.penalty, hi = under.penalty;
  const bool lo_open = !(lo > 0), hi_open = !std::isfinite(hi);
  if (!lo_open && !hi_open) {
    for (int j = 1; j <= extras; j++)
      out.push_back(lo * exp(log(hi / lo) * (double)j / (double)(extras + 1)));
    return;
  }
  const double anchor = secant;
  if (!(anchor > 0) || !std::isfinite(anchor)) return;
  const int n_up = (extras + 1) / 2, n_down = extras - n_up;
  for (int side = 1; side >= -1; side -= 2) {
    const int n = side > 0 ? n_up : n_down;
    const bool open = side > 0 ? hi_open : lo_open;
    const double span = open ? log(4.0) : (side > 0 ? log(hi / anchor) : log(anchor / lo));
    for (int j = 1; j <= n; j++) {
      const double x = (double)j / (double)(n + 1);
      out.push_back(anchor * exp((double)side * span * (open ? (double)j : x * x)));
    }
  }
}

}  // namespace

extern "C" int peakseg_hip_search_place_penalties(double under_penalty, double over_penalty,
                                                  double secant, int extras, double *out) {
  if (extras <= 0 || !out) return 0;
  psd_search_row under{}, over{};
  under.penalty = under_penalty;
  over.penalty = over_penalty;
  std::vector<double> more;
  place_penalties(under, over, secant, extras, more);
  int n = 0;
  for (double pen : more)
    if (n < extras) out[n++] = pen;
  return n;
}

namespace {

/* What tells the sequential entries from the parallel ones: the words of their error texts and
 * of their PEAKSEG_HIP_TIMING lines. */
struct SearchWords {
  const char *name, *round_label, *run_label;
  bool round_says_width;
};
const SearchWords SEQUENTIAL_SEARCH = {"sequential", "search batch round", "sequential search batch",
                                       false};
const SearchWords PARALLEL_SEARCH = {"parallel", "parallel search round", "parallel search", true};

int search_bad_arguments(const SearchWords &words) {
  set_error("%s search: bad arguments", words.name);
  return ERROR_SEARCH_ARGUMENTS;
}

/* The decisions of sequentialSearch_dir (R/sequentialSearch_dir.R:39-99) for one problem
 * directory, apart from how a model is computed, with `width` models per round after the first:
 * the secant model decides as the reference's one model does, every model of the round may narrow
 * the bracket.  With width 1 this is the reference's sequence of penalties. */
struct PenaltySearch {
  const SearchWords *words = nullptr;
  int peaks_int = 0, row_capacity = 0, width = 1;
  psd_search_row *rows = nullptr;
  int n = 0, under = -1, over = -1, candidate = -1, iteration = 0, first_new = 0;
  int status = 0;
  bool finished = false, narrow = false;
  double secant = 0.0;
  /* the round in flight: rows[first_new + k] holds its k-th penalty string */
  int round_size = 0;
  std::vector<char> solved, was_cached;

  bool active() const { return status == 0 && !finished; }
  bool in_round() const { return round_size > 0; }

  bool reserve(const std::string &pen_str) {
    if (first_new + round_size >= row_capacity) {
      set_error("%s search: more than %d models", words->name, row_capacity);
      status = ERROR_SEARCH_ARGUMENTS;
      return false;
    }
    psd_search_row &r = rows[first_new + round_size];
    memset(&r, 0, sizeof r);
    snprintf(r.penalty_str, sizeof r.penalty_str, "%s", pen_str.c_str());
    round_size++;
    return true;
  }

  /* the penalty strings of the next round, into the rows from rows[n] on; verbose: the
   * reference's "Next =" line, behind the directory's name where the caller gives one */
  void begin_round(int verbose, const char *dir_name) {
    iteration++;
    first_new = n;
    round_size = 0;
    if (iteration == 1) {
      if (reserve("0")) reserve("Inf");
    } else if (reserve(r_paste_double(secant)) && width > 1) {
      std::vector<double> more;
      place_penalties(rows[under], rows[over], secant, width - 1, more);
      for (double pen : more) {
        if (round_size >= width) break;
        const std::string s = r_paste_double(pen);
        const double v = strtod(s.c_str(), nullptr);
        if (!(rows[over].penalty < v && v < rows[under].penalty)) continue;
        bool seen = false; /* a string this search has asked for already, in this round or before */
        for (int k = 0; k < first_new + round_size && !seen; k++) seen = s == rows[k].penalty_str;
        if (seen) continue;
        if (!reserve(s)) break;
      }
    }
    solved.assign((size_t)round_size, 0);
    was_cached.assign((size_t)round_size, 0);
    if (status || !verbose) return;
    std::string line = "Next =";
    for (int k = 0; k < round_size; k++)
      line += std::string(k ? ", " : " ") + rows[first_new + k].penalty_str;
    if (dir_name) emit_text("%s: ", dir_name);
    emit_text("%s \n", line.c_str());
  }

  /* ERROR_DEVICE_MEMORY in this round: half the width from here on; the round keeps what fits */
  void narrow_round() {
    narrow = false;
    width = std::max(1, width / 2);
    if (iteration > 1 && round_size > width) {
      round_size = width;
      solved.resize((size_t)round_size);
      was_cached.resize((size_t)round_size);
    }
  }

  bool round_solved() const {
    for (char s : solved)
      if (!s) return false;
    return true;
  }

  /* the k-th model of the round, and the models before it, are there: n counts them */
  void record(int k, const LossRow &lr, bool cached) {
    const int NA = INT_MIN;
    psd_search_row &r = rows[first_new + k];
    r.iteration = iteration;
    r.under_peaks = under < 0 ? NA : rows[under].peaks;
    r.over_peaks = over < 0 ? NA : rows[over].peaks;
    r.penalty = lr.penalty;
    r.peaks = (int)lr.peaks;
    r.segments = (int)lr.segments;
    r.bases = (int)lr.bases;
    r.total_loss = lr.total_loss;
    r.cached = cached ? 1 : 0;
    n = first_new + k + 1;
  }

  /* after every model of the round has been recorded: the new bracket, or the end */
  void end_round() {
    const int last = first_new + round_size;
    n = last;
    round_size = 0;
    if (iteration == 1) {
      over = first_new;      /* penalty 0 */
      under = first_new + 1; /* penalty Inf */
      const int max_peaks = (rows[over].bases - 1) / 2;
      if (max_peaks < peaks_int) {
        set_error("peaks.int=%d but max=%d peaks for N=%d data", peaks_int, max_peaks,
                  rows[over].bases);
        status = ERROR_SEARCH_TOO_MANY_PEAKS;
        return;
      }
    } else {
      int hit = -1; /* a model with the target: the one with the largest penalty */
      for (int m = first_new; m < last; m++)
        if (rows[m].peaks == peaks_int && (hit < 0 || rows[m].penalty > rows[hit].penalty)) hit = m;
      const int m = first_new; /* the secant model */
      if (hit >= 0) {
        candidate = hit;
        finished = true;
        return;
      }
      if (rows[m].peaks == rows[under].peaks || rows[m].peaks == rows[over].peaks) {
        candidate = under; /* no hull vertex inside the bracket: pick the simpler model */
        finished = true;
        return;
      }
      if (rows[m].peaks < peaks_int) {
        under = m;
      } else {
        over = m;
      }
      /* the others narrow the bracket where they can; near penalty 0 peaks are not always
       * monotone in the penalty, and a model out of order stays a row only */
      for (int e = first_new + 1; e < last; e++) {
        const psd_search_row &r = rows[e], &u = rows[under], &o = rows[over];
        if (r.peaks < peaks_int) {
          const bool closer = r.peaks > u.peaks || (r.peaks == u.peaks && r.penalty < u.penalty);
          if (closer && r.penalty > o.penalty) under = e;
        } else {
          const bool closer = r.peaks < o.peaks || (r.peaks == o.peaks && r.penalty > o.penalty);
          if (closer && r.penalty < u.penalty) over = e;
        }
      }
    }
    if (peaks_int == rows[under].peaks) {
      candidate = under;
      finished = true;
    }
    if (peaks_int == rows[over].peaks) {
      candidate = over;
      finished = true;
    }
    if (finished) return;
    secant = (rows[over].total_loss - rows[under].total_loss) /
             (double)(rows[under].peaks - rows[over].peaks);
    if (secant < 0) {
      candidate = under; /* numerically unstable region: return the simpler model */
      finished = true;
    }
  }
};

/* The round of s is complete, or a model of it has failed: its models are read back from their
 * files and recorded -- after a failure those before the failing one, which n then counts, so
 * that rows[n] names the failure -- and the round ends. */
void close_round(PenaltySearch &s, const char *problem_dir) {
  const std::string bedGraph = dir_bedGraph(problem_dir);
  for (int k = 0; k < s.round_size && s.solved[(size_t)k]; k++) {
    LossRow lr;
    const std::string pre = penalty_prefix(bedGraph, s.rows[s.first_new + k].penalty_str);
    if (!dir_cache_ok(bedGraph, pre, lr)) {
      set_error("%s search: result files of %s are not consistent", s.words->name, pre.c_str());
      s.status = ERROR_DEVICE_SOLVER;
      break;
    }
    s.record(k, lr, s.was_cached[(size_t)k] != 0);
  }
  if (s.status) {
    s.round_size = 0;
  } else {
    s.end_round();
  }
}

/* The lockstep rounds of the searches of the directories dirs_of (all of them, or one shard's
 * under PEAKSEG_HIP_DEVICES): every model every active directory wants in a round goes into one
 * PeakSegFPOP_dir_batch call.  A round whose call reports ERROR_DEVICE_MEMORY is taken up again at
 * half the width, for the models still missing. */
void search_rounds(const std::vector<int> &dirs_of, char **problem_dirs,
                   std::vector<PenaltySearch> &ps, int verbose, bool name_dirs, double t0,
                   int &round, int &launches) {
  const SearchWords &words = *ps[(size_t)dirs_of[0]].words;
  for (;;) {
    std::vector<int> who, index;
    for (int d : dirs_of) {
      PenaltySearch &s = ps[(size_t)d];
      if (!s.active()) continue;
      if (!s.in_round()) {
        s.begin_round(verbose, name_dirs ? problem_dirs[d] : nullptr);
        if (s.status) continue;
      }
      for (int k = 0; k < s.round_size; k++) {
        if (s.solved[(size_t)k]) continue;
        who.push_back(d);
        index.push_back(k);
      }
    }
    if (who.empty()) break;
    round++;
    std::vector<char *> dirs, pens;
    for (size_t j = 0; j < who.size(); j++) {
      PenaltySearch &s = ps[(size_t)who[j]];
      dirs.push_back(problem_dirs[who[j]]);
      pens.push_back(s.rows[s.first_new + index[j]].penalty_str);
    }
    std::vector<int> st(dirs.size(), 0), cached(dirs.size(), 0);
    PeakSegFPOP_dir_batch((int)dirs.size(), dirs.data(), pens.data(), st.data(), cached.data());
    launches++;
    for (size_t j = 0; j < who.size(); j++) {
      PenaltySearch &s = ps[(size_t)who[j]];
      if (s.status) continue;
      if (st[j] == 0) {
        s.solved[(size_t)index[j]] = 1;
        s.was_cached[(size_t)index[j]] = cached[j] != 0;
      } else if (st[j] == ERROR_DEVICE_MEMORY && s.width > 1) {
        s.narrow = true;
      } else {
        s.status = st[j];
      }
    }
    size_t widest = 0;
    for (int d : dirs_of) {
      PenaltySearch &s = ps[(size_t)d];
      if (!s.in_round()) continue;
      if (!s.status) widest = std::max(widest, (size_t)s.round_size);
      if (s.narrow) s.narrow_round();
      if (s.status || s.round_solved()) close_round(s, problem_dirs[d]);
    }
    if (timing_on()) {
      char width_text[32] = "";
      if (words.round_says_width) snprintf(width_text, sizeof width_text, " width %zu,", widest);
      fprintf(stderr, "peakseg_hip timing: %s %d: %zu models,%s %.1f s so far\n",
              words.round_label, round, dirs.size(), width_text, wall_now() - t0);
    }
  }
}

/* the directories whose search can start, dealt to n_shards by the byte size of their
 * coverage.bedGraph */
std::vector<std::vector<int>> deal_dirs_by_size(const std::vector<PenaltySearch> &ps,
                                                const std::vector<std::string> &bedGraph,
                                                int n_shards) {
  std::vector<int> live;
  std::vector<double> cost;
  for (size_t d = 0; d < ps.size(); d++) {
    if (ps[d].status) continue;
    struct stat sb;
    live.push_back((int)d);
    cost.push_back(stat(bedGraph[d].c_str(), &sb) == 0 ? (double)sb.st_size : 0.0);
  }
  std::vector<std::vector<int>> shards = deal_lpt(cost, n_shards);
  for (auto &sh : shards)
    for (int &j : sh) j = live[(size_t)j];
  return shards;
}

/* The searches of n_dirs directories.  deal_dirs: under PEAKSEG_HIP_DEVICES the directories go
 * to one shard per device, dealt by the byte size of their coverage.bedGraph, and each shard runs
 * the rounds of its own directories on a thread pinned to its device (the batch entries);
 * otherwise every round's PeakSegFPOP_dir_batch deals its models over the devices itself (the
 * single entry).  (A bad PEAKSEG_HIP_DEVICES: no shards, and the rounds' calls fail the dynamic
 * programs.)  width 0: the default width. */
int search_run(const SearchWords &words, int n_dirs, char **problem_dirs, const int *peaks_int,
               int width, int verbose, int row_capacity, psd_search_row *rows, int *n_rows,
               int *chosen_row, int *status_out, bool deal_dirs) {
  std::vector<PenaltySearch> ps((size_t)n_dirs);
  std::vector<std::string> bedGraph((size_t)n_dirs);
  for (int d = 0; d < n_dirs; d++) {
    PenaltySearch &s = ps[(size_t)d];
    s.words = &words;
    s.peaks_int = peaks_int[d];
    s.row_capacity = row_capacity;
    s.width = width ? width : PARALLEL_SEARCH_DEFAULT_WIDTH;
    s.rows = rows + (size_t)d * (size_t)row_capacity;
    if (peaks_int[d] < 0 || !problem_dirs[d]) s.status = ERROR_SEARCH_ARGUMENTS;
    if (problem_dirs[d]) bedGraph[(size_t)d] = real_path(dir_bedGraph(problem_dirs[d]));
  }
  /* a directory listed twice would have two searches write the same files in the same launch */
  for (int d = 0; d < n_dirs; d++)
    for (int e = 0; e < d; e++)
      if (ps[(size_t)d].status == 0 && bedGraph[(size_t)d] == bedGraph[(size_t)e]) {
        set_error("%s search: problem directory %s is listed twice", words.name, problem_dirs[d]);
        ps[(size_t)d].status = ERROR_SEARCH_ARGUMENTS;
      }
  const double t0 = wall_now();
  int round = 0, launches = 0;
  std::vector<int> devices;
  if (deal_dirs && g_shard_device < 0) env_devices(devices);
  if (devices.empty()) {
    std::vector<int> all((size_t)n_dirs);
    for (int d = 0; d < n_dirs; d++) all[(size_t)d] = d;
    search_rounds(all, problem_dirs, ps, verbose, deal_dirs, t0, round, launches);
    if (deal_dirs) g_fanout.clear(n_dirs);
  } else {
    const std::vector<std::vector<int>> shards =
        deal_dirs_by_size(ps, bedGraph, (int)devices.size());
    std::vector<int> rounds(devices.size(), 0), shard_launches(devices.size(), 0);
    std::vector<ShardResult> results;
    run_shards(devices, shards, results, [&](int sh) {
      search_rounds(shards[(size_t)sh], problem_dirs, ps, verbose, true, t0, rounds[(size_t)sh],
                    shard_launches[(size_t)sh]);
      for (int d : shards[(size_t)sh])
        if (ps[(size_t)d].status) results[(size_t)sh].failed = true;
    });
    g_fanout.entry_shard.assign((size_t)n_dirs, -1);
    for (size_t sh = 0; sh < shards.size(); sh++) {
      for (int d : shards[sh]) g_fanout.entry_shard[(size_t)d] = (int)sh;
      round = std::max(round, rounds[sh]);
      launches += shard_launches[sh];
    }
  }
  int first = 0;
  for (int d = 0; d < n_dirs; d++) {
    const PenaltySearch &s = ps[(size_t)d];
    if (n_rows) n_rows[d] = s.n;
    if (chosen_row) chosen_row[d] = s.status ? -1 : s.candidate;
    if (status_out) status_out[d] = s.status;
    if (s.status && !first) first = s.status;
  }
  if (timing_on())
    fprintf(stderr, "peakseg_hip timing: %s: %d directories, %d rounds, %d launches, %.3f s\n",
            words.run_label, n_dirs, round, launches, wall_now() - t0);
  return first;
}

}  // namespace

/* sequentialSearch_dir on one directory: the reference's loop with the contig parsed and uploaded
 * once and the arena reused from one penalty to the next (ResidentDir); the models of a round are
 * computed one after the other. */
extern "C" int PeakSegFPOP_sequential_search(const char *problem_dir, int peaks_int, int verbose,
                                             int row_capacity, psd_search_row *rows, int *n_rows,
                                             int *chosen_row) {
  g_fanout.clear(1);
  if (n_rows) *n_rows = 0;
  if (chosen_row) *chosen_row = -1;
  if (!problem_dir || peaks_int < 0 || !rows || row_capacity < 2)
    return search_bad_arguments(SEQUENTIAL_SEARCH);
  ResidentDir rd;
  rd.dir = problem_dir;
  PenaltySearch s;
  s.words = &SEQUENTIAL_SEARCH;
  s.peaks_int = peaks_int;
  s.row_capacity = row_capacity;
  s.rows = rows;
  while (s.active()) {
    s.begin_round(verbose, nullptr);
    for (int k = 0; k < s.round_size && !s.status; k++) {
      const psd_search_row &r = rows[s.first_new + k];
      LossRow lr;
      bool cached = false;
      s.status = rd.model(r.penalty_str, lr, cached);
      if (s.status) break;
      s.record(k, lr, cached);
      if (timing_on()) /* progress of a long search (stderr is unbuffered) */
        fprintf(stderr, "peakseg_hip timing: search model %d: penalty=%s peaks=%d%s, %.1f s so far "
                        "in the kernel\n", s.n, r.penalty_str, r.peaks, cached ? " (cached)" : "",
                rd.kernel_s);
    }
    if (n_rows) *n_rows = s.n;
    if (s.status) return s.status;
    s.end_round();
  }
  if (s.status) return s.status;
  if (chosen_row) *chosen_row = s.candidate;
  if (timing_on())
    fprintf(stderr, "peakseg_hip timing: sequential search: %d models, %d dynamic programs, "
                    "%.3f s in the kernel\n", s.n, rd.solves, rd.kernel_s);
  return 0;
}

/* sequentialSearch_dir over several problem directories at once (additive entry): every
 * directory follows its own search, exactly as PeakSegFPOP_sequential_search would, but the
 * models the searches ask for in the same iteration are computed in ONE launch
 * (PeakSegFPOP_dir_batch: one problem per directory, the chip shared between them).  One
 * search keeps four wave slots of 8192 busy; a genome's worth of contigs searched together
 * costs about what its longest search costs.  rows: n_dirs x row_capacity; n_rows, chosen_row,
 * status_out: per directory.  Returns the first non-zero status (0: every search ended). */
extern "C" int PeakSegFPOP_sequential_search_batch(int n_dirs, char **problem_dirs,
                                                   const int *peaks_int, int verbose,
                                                   int row_capacity, psd_search_row *rows,
                                                   int *n_rows, int *chosen_row,
                                                   int *status_out) {
  g_fanout.clear(n_dirs);
  if (n_dirs <= 0) return 0;
  if (!problem_dirs || !peaks_int || !rows || row_capacity < 2)
    return search_bad_arguments(SEQUENTIAL_SEARCH);
  return search_run(SEQUENTIAL_SEARCH, n_dirs, problem_dirs, peaks_int, 1, verbose, row_capacity,
                    rows, n_rows, chosen_row, status_out, true);
}

/* A penalty search of its own choosing: `width` models per round (0: the default width), every
 * round one PeakSegFPOP_dir_batch call. */
extern "C" int PeakSegFPOP_parallel_search(const char *problem_dir, int peaks_int, int width,
                                           int verbose, int row_capacity, psd_search_row *rows,
                                           int *n_rows, int *chosen_row) {
  g_fanout.clear(1);
  if (n_rows) *n_rows = 0;
  if (chosen_row) *chosen_row = -1;
  if (!problem_dir || peaks_int < 0 || !rows || row_capacity < 2 || width < 0 ||
      width > PARALLEL_SEARCH_MAX_WIDTH)
    return search_bad_arguments(PARALLEL_SEARCH);
  char *dir = const_cast<char *>(problem_dir);
  return search_run(PARALLEL_SEARCH, 1, &dir, &peaks_int, width, verbose, row_capacity, rows,
                    n_rows, chosen_row, nullptr, false);
}

extern "C" int PeakSegFPOP_parallel_search_batch(int n_dirs, char **problem_dirs,
                                                 const int *peaks_int, int width, int verbose,
                                                 int row_capacity, psd_search_row *rows,
                                                 int *n_rows, int *chosen_row, int *status_out) {
  g_fanout.clear(n_dirs);
  if (n_dirs <= 0) return 0;
  if (!problem_dirs || !peaks_int || !rows || row_capacity < 2 || width < 0 ||
      width > PARALLEL_SEARCH_MAX_WIDTH)
    return search_bad_arguments(PARALLEL_SEARCH);
  return search_run(PARALLEL_SEARCH, n_dirs, problem_dirs, peaks_int, width, verbose, row_capacity,
                    rows, n_rows, chosen_row, status_out, true);
}
