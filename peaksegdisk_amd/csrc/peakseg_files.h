/* peakseg_files.h -- the reference's file boundary (included by peakseg_hip.cpp).
 *
 *   FileProblem                      one (bedGraph, penalty, db) problem and what its loss file says
 *   the writers                      the two output files and the database placeholder
 *   solve_files                      many such problems in one call, as named steps
 *   PeakSegFPOP_disk / _disk_batch   the reference's native boundary
 *                                    (/root/reference/src/PeakSegFPOPLog.cpp:143-463, "drv")
 *
 * Every dynamic program runs on the GPU (peakseg_fanout.h); this file only parses, formats and
 * moves files.  The layers above it: peakseg_dir.h (PeakSegFPOP_dir's cache protocol),
 * peakseg_search.h (the penalty searches).
 */
#include <limits.h>
#include <sys/stat.h>

namespace {

/* ---- one (bedGraph, penalty, db) problem of the file-level boundary -------------------- */

struct FileProblem {
  const char *bedGraph = nullptr, *penalty_str = nullptr, *db = nullptr;
  int status = 0;
  bool is_Inf = false;
  double penalty = 0.0;
  int cov = -1;      /* index into the parsed-coverage table */
  int dp_index = -1; /* index into the device problem set, -1 = trivial/none */
  int shard = -1;    /* PEAKSEG_HIP_DEVICES: the shard that solved its program, -1 = none */
  bool outputs_opened = false;
  bool loss_failed = false, segments_failed = false;
  /* what the loss file says (kept for PeakSegFPOP_dir_batch / the penalty search) */
  int n_segments = 0, n_peaks = 0, bases = 0;
  double total_loss = 0.0;
  long long db_bytes = 0; /* size of the reference's cost-function database for this problem */
};

/* "<path>_penalty=<penalty string>": what the names of a model's files begin with
 * (drv:212-223, R/PeakSegFPOP_dir.R:64) */
std::string penalty_prefix(const std::string &path, const char *penalty_str) {
  return path + "_penalty=" + penalty_str;
}

std::string out_prefix(const FileProblem &fp) { return penalty_prefix(fp.bedGraph, fp.penalty_str); }

/* create / truncate, as the reference's ofstream::open does at drv:212-223 */
bool truncate_file(const std::string &path) {
  FILE *f = fopen(path.c_str(), "w");
  if (!f) return false;
  return fclose(f) == 0;
}

bool write_whole_file(const std::string &path, const std::string &text) {
  FILE *f = fopen(path.c_str(), "w");
  if (!f) return false;
  bool ok = text.empty() || fwrite(text.data(), 1, text.size(), f) == text.size();
  if (fclose(f) != 0) ok = false;
  return ok;
}

void append_fmt(std::string &s, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  int n = vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (n > 0) s.append(buf, (size_t)(n < (int)sizeof buf ? n : (int)sizeof buf - 1));
}

/* Output files are created before the trivial/DP split (drv:212-223) and each of them is
 * written in one piece later: no descriptor stays open across the kernel (a batch of several
 * hundred problems used to hold two FILE* each, past the usual 1024-descriptor limit). */
void open_outputs(FileProblem &fp) {
  const std::string pre = out_prefix(fp);
  fp.loss_failed = !truncate_file(pre + "_loss.tsv");
  fp.segments_failed = !truncate_file(pre + "_segments.bed");
  fp.outputs_opened = true;
}

void write_outputs(FileProblem &fp, const std::string &segments, const std::string &loss) {
  const std::string pre = out_prefix(fp);
  if (!fp.loss_failed && !write_whole_file(pre + "_loss.tsv", loss)) fp.loss_failed = true;
  if (!fp.segments_failed && !write_whole_file(pre + "_segments.bed", segments))
    fp.segments_failed = true;
}

/* trivial one-segment model (drv:224-243) */
void write_trivial(FileProblem &fp, const Coverage &cv) {
  double best_cost;
  if (cv.cum_weighted_count != 0) {
    best_cost =
        cv.cum_weighted_count * (1 - psd_log(cv.cum_weighted_count) + psd_log(cv.cum_weight));
  } else {
    best_cost = 0;
  }
  std::string seg, loss;
  append_fmt(seg, "%s\t%d\t%d\tbackground\t%g\n", cv.chrom.c_str(), cv.first_chromStart,
             cv.chromEnd.back(), cv.cum_weighted_count / cv.cum_weight);
  append_fmt(loss, "%s\t%d\t%d\t%d\t%d\t%.20g\t%.20g\t%d\t%d\t%d\n", fp.penalty_str, 1, 0,
             (int)cv.cum_weight, cv.n(), best_cost / cv.cum_weight, best_cost, 0, 0, 0);
  write_outputs(fp, seg, loss);
  fp.n_segments = 1;
  fp.n_peaks = 0;
  fp.bases = (int)cv.cum_weight;
  fp.total_loss = best_cost;
  fp.db_bytes = 0;
}

/* the DP branch's two files (drv:419-454) */
int write_dp_outputs(FileProblem &fp, const Coverage &cv, const DpFetched &f) {
  if (f.status) return f.status;
  const psd_result &r = f.r;
  int prev_chromEnd = cv.chromEnd.back();
  const char *chrom = cv.chrom.c_str();
  std::string seg, loss;
  seg.reserve((size_t)r.n_segments * 48);
  for (int row = 0; row < r.n_segments; row++) {
    int start = f.seg_start[(size_t)row] < 0 ? cv.first_chromStart
                                             : cv.chromEnd[(size_t)f.seg_start[(size_t)row]];
    /* rows alternate background/peak starting and ending with background (drv:421-429,442) */
    const char *status_str = (row % 2 == 0) ? "background" : "peak";
    append_fmt(seg, "%s\t%d\t%d\t%s\t%g\n", chrom, start, prev_chromEnd, status_str,
               f.seg_mean[(size_t)row]);
    prev_chromEnd = start;
  }
  int n_peaks = (r.n_segments - 1) / 2;
  double total_intervals = (double)r.total_intervals;
  const double total_loss = r.best_cost * cv.cum_weight - fp.penalty * n_peaks;
  append_fmt(loss, "%.20g\t%d\t%d\t%d\t%d\t%.20g\t%.20g\t%d\t%.20g\t%.20g\n", fp.penalty,
             r.n_segments, n_peaks, (int)cv.cum_weight, cv.n(), r.best_cost, total_loss,
             r.n_equality_constraints, total_intervals / (cv.n() * 2), (double)r.max_intervals);
  write_outputs(fp, seg, loss);
  fp.n_segments = r.n_segments;
  fp.n_peaks = n_peaks;
  fp.bases = (int)cv.cum_weight;
  fp.total_loss = total_loss;
  /* leave a sparse file of the size the reference's DiskVector would have:
   * 2N 16-byte positions + per function {int size, int n, int chromEnd} + 20 B per piece */
  fp.db_bytes = 32ll * cv.n() + 12ll * (2ll * cv.n() - 1) + 20ll * (long long)r.total_intervals;
  if (truncate(fp.db, (off_t)fp.db_bytes) != 0) return ERROR_WRITING_COST_FUNCTIONS;
  return 0;
}

/* write failures are reported at the end, loss first (drv:456-461) */
void settle_status(FileProblem &fp) {
  if (fp.status == 0 && fp.outputs_opened) {
    if (fp.loss_failed) {
      fp.status = ERROR_WRITING_LOSS_OUTPUT;
    } else if (fp.segments_failed) {
      fp.status = ERROR_WRITING_SEGMENTS_OUTPUT;
    }
  }
}

/* the DP branch touches the cost-function database first (drv:247-252) */
bool touch_db(FileProblem &fp) {
  FILE *db = fopen(fp.db, "w+b");
  if (!db) {
    fp.status = ERROR_WRITING_COST_FUNCTIONS;
    return false;
  }
  fclose(db);
  return true;
}

std::string real_path(const std::string &path) {
  char buf[PATH_MAX];
  if (realpath(path.c_str(), buf)) return buf;
  return path;
}

/* ---- solve_files: many problems in one call ---------------------------------------------- */

/* A (bedGraph, penalty string) pair listed twice names the same two output files -- the
 * reference builds the names from the path string as given (drv:212-223) -- so the second copy
 * is not processed at all (its writer thread would race the first one's on the same paths);
 * it receives the first one's status and figures at the end.  Two DIFFERENT strings that reach
 * the same file (a symlinked coverage.bedGraph, as in PeakSegPipeline problem directories)
 * name different output files: each entry gets its own, but the file is parsed once and the
 * dynamic program of a (file, penalty) pair runs once (build_programs).
 * -> for each entry the first entry with its pair, or -1 */
std::vector<int> find_duplicates(int n, const FileProblem *fps) {
  std::vector<int> dup_of((size_t)n, -1);
  std::map<std::pair<std::string, std::string>, int> seen;
  for (int i = 0; i < n; i++) {
    auto key = std::make_pair(std::string(fps[i].bedGraph), std::string(fps[i].penalty_str));
    auto it = seen.find(key);
    if (it == seen.end()) {
      seen[key] = i;
    } else {
      dup_of[(size_t)i] = it->second;
    }
  }
  return dup_of;
}

/* penalties, then inputs (validation order of drv:145-209); one parse per file, whatever its
 * names */
void parse_inputs(int n, FileProblem *fps, const std::vector<int> &dup_of,
                  std::vector<Coverage> &covs) {
  std::map<std::string, int> cov_of_path, cov_status;
  for (int i = 0; i < n; i++) {
    FileProblem &fp = fps[i];
    if (dup_of[(size_t)i] >= 0) continue;
    fp.status = parse_penalty(fp.penalty_str, fp.is_Inf, fp.penalty);
    if (fp.status) continue;
    const std::string path = real_path(fp.bedGraph);
    auto it = cov_of_path.find(path);
    if (it == cov_of_path.end()) {
      Coverage cv;
      cov_status[path] = read_bedGraph(fp.bedGraph, cv);
      covs.push_back(std::move(cv));
      it = cov_of_path.emplace(path, (int)covs.size() - 1).first;
    }
    fp.cov = it->second;
    fp.status = cov_status[path];
  }
}

/* One problem whose penalty and input are valid: the output files are created before the
 * trivial/DP split (drv:212-223); the db is only touched in the DP branch (drv:247-252).
 * -> true when a dynamic program is to run for it */
bool open_outputs_and_split(FileProblem &fp, const Coverage &cv) {
  open_outputs(fp);
  if (fp.is_Inf || cv.min_log_mean == cv.max_log_mean) {
    write_trivial(fp, cv);
    return false;
  }
  return touch_db(fp);
}

/* -> the entries that need a dynamic program */
std::vector<int> open_all_and_split(int n, FileProblem *fps, const std::vector<int> &dup_of,
                                    const std::vector<Coverage> &covs) {
  std::vector<int> dp;
  for (int i = 0; i < n; i++) {
    FileProblem &fp = fps[i];
    if (fp.status || dup_of[(size_t)i] >= 0) continue;
    if (open_outputs_and_split(fp, covs[(size_t)fp.cov])) dp.push_back(i);
  }
  return dp;
}

/* the device programs of the entries dp: one contig per parsed file, one problem per (file,
 * penalty string) -- the same file under another name shares its problem; sets dp_index */
DevicePrograms build_programs(FileProblem *fps, const std::vector<int> &dp,
                              const std::vector<Coverage> &covs) {
  DevicePrograms progs;
  std::vector<int> contig_of_cov(covs.size(), -1);
  std::map<std::pair<int, std::string>, int> dp_of; /* (file, penalty string) -> device problem */
  for (int i : dp) {
    FileProblem &fp = fps[i];
    if (contig_of_cov[(size_t)fp.cov] < 0) {
      contig_of_cov[(size_t)fp.cov] = (int)progs.contig_n.size();
      const Coverage &cv = covs[(size_t)fp.cov];
      progs.contig_n.push_back(cv.n());
      progs.cnt_ptr.push_back(cv.count.data());
      progs.wt_ptr.push_back(cv.weight.data());
    }
    auto found = dp_of.emplace(std::make_pair(fp.cov, std::string(fp.penalty_str)),
                               (int)progs.prob_contig.size());
    fp.dp_index = found.first->second;
    if (!found.second) continue;
    progs.prob_contig.push_back(contig_of_cov[(size_t)fp.cov]);
    progs.prob_pen.push_back(fp.penalty);
  }
  return progs;
}

/* all dynamic programs in one device problem set (PEAKSEG_HIP_DEVICES, in a batch entry point:
 * in one set per shard); results into fetched[program], sets the entries' shard */
void solve_programs(FileProblem *fps, const std::vector<int> &dp, const DevicePrograms &progs,
                    bool fan_out, std::vector<DpFetched> &fetched, Lap &lap) {
  std::vector<int> devices;
  const int knob = fan_out && g_shard_device < 0 ? env_devices(devices) : 0;
  if (!devices.empty()) {
    const std::vector<int> shard_of = solve_shards(devices, progs, fetched);
    for (int i : dp) fps[i].shard = shard_of[(size_t)fps[i].dp_index];
    lap("upload + kernel + download, shards");
    return;
  }
  int device = 0;
  const int st = knob ? knob : env_device(device);
  if (st) {
    for (DpFetched &f : fetched) f.status = st;
    return;
  }
  /* a shard thread's nested call (the search batch): its set holds the device's mutex */
  std::unique_lock<std::mutex> hold;
  if (g_shard_device >= 0) hold = std::unique_lock<std::mutex>(device_mutex(device));
  ShardClock unshared;
  solve_on_device(device, progs, fetched.data(), g_shard_clock ? *g_shard_clock : unshared, &lap);
}

/* the two files of every dynamic program (drv:419-454), formatted by up to 16 threads */
void write_all_dp_outputs(FileProblem *fps, const std::vector<int> &dp,
                          const std::vector<Coverage> &covs, const std::vector<DpFetched> &fetched) {
  std::atomic<size_t> next_k{0};
  auto writer = [&]() {
    for (size_t k = next_k++; k < dp.size(); k = next_k++) {
      FileProblem &fp = fps[dp[k]];
      fp.status = write_dp_outputs(fp, covs[(size_t)fp.cov], fetched[(size_t)fp.dp_index]);
    }
  };
  unsigned n_threads = std::thread::hardware_concurrency();
  if (n_threads > 16) n_threads = 16;
  if (n_threads > dp.size()) n_threads = (unsigned)dp.size();
  if (n_threads <= 1) {
    writer();
  } else {
    std::vector<std::thread> pool;
    for (unsigned w = 0; w < n_threads; w++) pool.emplace_back(writer);
    for (auto &th : pool) th.join();
  }
}

/* write failures are reported at the end (drv:456-461); a duplicate entry receives the first
 * copy's status and figures.  -> the first non-zero status */
int settle_all(int n, FileProblem *fps, const std::vector<int> &dup_of) {
  for (int i = 0; i < n; i++)
    if (dup_of[(size_t)i] < 0) settle_status(fps[i]);
  int first = 0;
  for (int i = 0; i < n; i++) {
    FileProblem &fp = fps[i];
    if (dup_of[(size_t)i] >= 0) {
      const FileProblem &o = fps[dup_of[(size_t)i]];
      fp.status = o.status;
      fp.n_segments = o.n_segments;
      fp.n_peaks = o.n_peaks;
      fp.bases = o.bases;
      fp.total_loss = o.total_loss;
      fp.db_bytes = o.db_bytes;
      fp.shard = o.shard;
      /* its own database name, if it has one, is left as the first copy's is */
      if (fp.status == 0 && o.dp_index >= 0 && strcmp(fp.db, o.db) != 0 && touch_db(fp) &&
          truncate(fp.db, (off_t)fp.db_bytes) != 0)
        fp.status = ERROR_WRITING_COST_FUNCTIONS;
    }
    if (fp.status && !first) first = fp.status;
  }
  return first;
}

int solve_files(int n, FileProblem *fps, bool fan_out) {
  Lap lap;
  std::vector<Coverage> covs;
  const std::vector<int> dup_of = find_duplicates(n, fps);
  parse_inputs(n, fps, dup_of, covs);
  lap("parse bedGraph");
  const std::vector<int> dp = open_all_and_split(n, fps, dup_of, covs);
  if (!dp.empty()) {
    const DevicePrograms progs = build_programs(fps, dp, covs);
    std::vector<DpFetched> fetched(progs.prob_contig.size());
    solve_programs(fps, dp, progs, fan_out, fetched, lap);
    write_all_dp_outputs(fps, dp, covs, fetched);
    lap("write segments/loss files");
  }
  return settle_all(n, fps, dup_of);
}

}  // namespace

extern "C" int PeakSegFPOP_disk(char *bedGraph_file_name, char *penalty_str, char *db_file_name) {
  FileProblem fp;
  fp.bedGraph = bedGraph_file_name;
  fp.penalty_str = penalty_str;
  fp.db = db_file_name;
  g_fanout.clear(1);
  return solve_files(1, &fp, false);
}

extern "C" int PeakSegFPOP_disk_batch(int n_problems, char **bedGraph_files, char **penalty_strs,
                                      char **db_files, int *status_out) {
  g_fanout.clear(n_problems);
  if (n_problems <= 0) return 0;
  std::vector<FileProblem> fps((size_t)n_problems);
  for (int i = 0; i < n_problems; i++) {
    fps[(size_t)i].bedGraph = bedGraph_files[i];
    fps[(size_t)i].penalty_str = penalty_strs[i];
    fps[(size_t)i].db = db_files[i];
  }
  int first = solve_files(n_problems, fps.data(), true);
  for (int i = 0; i < n_problems; i++) g_fanout.entry_shard[(size_t)i] = fps[(size_t)i].shard;
  if (status_out)
    for (int i = 0; i < n_problems; i++) status_out[i] = fps[(size_t)i].status;
  return first;
}
