/* peakseg_dir.h -- PeakSegFPOP_dir's protocol for one model of a problem directory, next to the
 * file boundary of peakseg_files.h (/root/reference/R/PeakSegFPOP_dir.R:64-117,
 * R/PeakSegFPOP_file.R:30-87):
 *
 *   dir_cache_ok and its parsers     the result-file cache (R/PeakSegFPOP_dir.R:70-93)
 *   DirModel, finish_model           the names of a (problem dir, penalty) model, and what follows
 *                                    its solve: megabytes, the db removed, _timing.tsv, the loss row
 *   ResidentDir                      a directory whose contig stays parsed and uploaded from one
 *                                    penalty to the next (the sequential search)
 *   PeakSegFPOP_dir_batch            many models in one solve_files call
 */
namespace {

/* ---- PeakSegFPOP_dir's result-file cache (R/PeakSegFPOP_dir.R:70-93) -------------------- */

bool read_small_file(const std::string &path, std::string &out) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return false;
  char chunk[4096];
  size_t got;
  out.clear();
  while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) {
    out.append(chunk, got);
    if (out.size() > (1u << 20)) break; /* one-row files */
  }
  fclose(f);
  return true;
}

std::vector<std::string> split_fields(const std::string &line) {
  std::vector<std::string> out;
  size_t i = 0;
  while (i < line.size()) {
    while (i < line.size() && (line[i] == '\t' || line[i] == ' ' || line[i] == '\r')) i++;
    size_t j = i;
    while (j < line.size() && line[j] != '\t' && line[j] != ' ' && line[j] != '\r') j++;
    if (j > i) out.push_back(line.substr(i, j - i));
    i = j;
  }
  return out;
}

std::vector<std::string> nonempty_lines(const std::string &text) {
  std::vector<std::string> out;
  size_t i = 0;
  while (i < text.size()) {
    size_t j = text.find('\n', i);
    if (j == std::string::npos) j = text.size();
    std::string line = text.substr(i, j - i);
    if (!split_fields(line).empty()) out.push_back(line);
    i = j + 1;
  }
  return out;
}

/* first and last line of a (possibly large) text file without reading all of it */
bool first_last_line(const std::string &path, std::string &first, std::string &last) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return false;
  char buf[8192];
  bool ok = fgets(buf, sizeof buf, f) != nullptr;
  if (ok) {
    first = buf;
    while (!first.empty() && (first.back() == '\n' || first.back() == '\r')) first.pop_back();
    ok = fseek(f, 0, SEEK_END) == 0;
  }
  if (ok) {
    long size = ftell(f);
    long back = size < (long)sizeof buf - 1 ? size : (long)sizeof buf - 1;
    ok = fseek(f, size - back, SEEK_SET) == 0;
    if (ok) {
      size_t got = fread(buf, 1, (size_t)back, f);
      std::string tail(buf, got);
      std::vector<std::string> lines = nonempty_lines(tail);
      ok = !lines.empty();
      if (ok) last = lines.back();
    }
  }
  fclose(f);
  return ok && !split_fields(first).empty();
}

bool parse_int_field(const std::string &s, long long &v) {
  char *end = nullptr;
  errno = 0;
  v = strtoll(s.c_str(), &end, 10);
  return end != s.c_str() && *end == 0 && errno == 0;
}

bool parse_double_field(const std::string &s, double &v) {
  char *end = nullptr;
  v = strtod(s.c_str(), &end);
  return end != s.c_str() && *end == 0;
}

struct LossRow { /* the columns of _loss.tsv the callers use (R/col.name.list.R:12-15) */
  double penalty = 0.0, total_loss = 0.0;
  long long segments = 0, peaks = 0, bases = 0;
};

/* TRUE when the three result files of (problem dir, penalty) exist and are consistent, as
 * PeakSegFPOP_dir decides before it reuses them; any failure means recompute. */
bool dir_cache_ok(const std::string &bedGraph, const std::string &pre, LossRow &row) {
  std::string text, first_seg, last_seg, first_cov, last_cov;
  if (!read_small_file(pre + "_timing.tsv", text)) return false;
  std::vector<std::string> tl = nonempty_lines(text);
  if (tl.size() != 1 || split_fields(tl[0]).size() != 3) return false;
  if (!first_last_line(pre + "_segments.bed", first_seg, last_seg)) return false;
  if (!first_last_line(bedGraph, first_cov, last_cov)) return false;
  if (!read_small_file(pre + "_loss.tsv", text)) return false;
  std::vector<std::string> ll = nonempty_lines(text);
  if (ll.size() != 1) return false;
  std::vector<std::string> lf = split_fields(ll[0]);
  std::vector<std::string> fs = split_fields(first_seg), ls = split_fields(last_seg);
  std::vector<std::string> fc = split_fields(first_cov), lc = split_fields(last_cov);
  if (lf.size() != 10 || fs.size() != 5 || ls.size() != 5 || fc.size() != 4 || lc.size() != 4)
    return false;
  long long fs_end, ls_start, fc_start, lc_end;
  if (!parse_int_field(fs[2], fs_end) || !parse_int_field(ls[1], ls_start) ||
      !parse_int_field(fc[1], fc_start) || !parse_int_field(lc[2], lc_end))
    return false;
  if (!parse_double_field(lf[0], row.penalty) || !parse_int_field(lf[1], row.segments) ||
      !parse_int_field(lf[2], row.peaks) || !parse_int_field(lf[3], row.bases) ||
      !parse_double_field(lf[6], row.total_loss))
    return false;
  return fs_end - ls_start == row.bases && fc_start == ls_start && lc_end == fs_end;
}

/* _timing.tsv: penalty, megabytes, seconds the way write.table() prints them
 * (R/PeakSegFPOP_dir.R:98-106) */
bool write_timing(const std::string &pre, const char *penalty_str, double megabytes,
                  double seconds) {
  std::string t = r_paste_double(strtod(penalty_str, nullptr)) + "\t" +
                  r_paste_double(megabytes) + "\t" + r_paste_double(seconds) + "\n";
  return write_whole_file(pre + "_timing.tsv", t);
}

bool file_exists(const std::string &path) {
  struct stat st;
  return stat(path.c_str(), &st) == 0;
}

/* ---- one model of one problem directory ------------------------------------------------- */

/* The names PeakSegFPOP_dir and PeakSegFPOP_file give a (problem dir, penalty string) model: the
 * result files begin with `pre`, the solver is given the normalised path and the default db name. */
std::string dir_bedGraph(const std::string &dir) { return dir + "/coverage.bedGraph"; }

struct DirModel {
  const char *penalty_str;
  std::string bedGraph, pre, norm, db;

  DirModel(const std::string &dir, const char *pen)
      : penalty_str(pen), bedGraph(dir_bedGraph(dir)),
        pre(penalty_prefix(bedGraph, pen)), norm(real_path(bedGraph)),
        db(penalty_prefix(norm, pen) + ".db") {}

  /* the problem PeakSegFPOP_file hands to the solver; the db is removed before the call */
  FileProblem start() const {
    unlink(db.c_str());
    FileProblem fp;
    fp.bedGraph = norm.c_str();
    fp.penalty_str = penalty_str;
    fp.db = db.c_str();
    return fp;
  }
};

/* After the solve (R/PeakSegFPOP_file.R:75-86, R/PeakSegFPOP_dir.R:98-106): the db's megabytes,
 * the db removed, _timing.tsv written, and the loss row the callers would read back from the
 * 20-digit text of _loss.tsv (same double).  -> the model's status */
int finish_model(const DirModel &m, FileProblem &fp, double seconds, LossRow *row) {
  const double megabytes = file_exists(m.db) ? (double)fp.db_bytes / 1024.0 / 1024.0 : 0.0;
  unlink(m.db.c_str());
  if (fp.status == 0 && !write_timing(m.pre, m.penalty_str, megabytes, seconds))
    fp.status = ERROR_WRITING_LOSS_OUTPUT;
  if (fp.status == 0 && row) {
    row->penalty = fp.penalty;
    row->segments = fp.n_segments;
    row->peaks = fp.n_peaks;
    row->bases = fp.bases;
    row->total_loss = fp.total_loss;
  }
  return fp.status;
}

/* ---- a problem directory kept resident for a sequence of penalties ---------------------- */

struct ResidentDir {
  std::string dir;
  bool parsed = false;
  int parse_status = 0;
  Coverage cv;
  psd_problem_set *set = nullptr;
  double kernel_s = 0.0;
  int solves = 0;

  ~ResidentDir() {
    if (set) peakseg_hip_problem_set_destroy(set);
  }

  /* the dynamic program of fp on the resident contig, uploaded on the first call only */
  void solve(const FileProblem &fp, DpFetched &f) {
    if (!set) {
      const int n = cv.n();
      const int *cnt = cv.count.data(), *wt = cv.weight.data();
      const int contig = 0;
      int device = 0;
      f.status = env_device(device);
      if (f.status == 0)
        f.status = peakseg_hip_problem_set_create(device, 1, &n, &cnt, &wt, 1, &contig, &fp.penalty,
                                                  0, &set);
    } else if (peakseg_hip_problem_set_set_penalty(set, 0, fp.penalty) != 0) {
      f.status = ERROR_DEVICE_SOLVER;
    }
    if (f.status == 0) {
      float ms = 0.f;
      f.status = peakseg_hip_problem_set_solve(set, &ms, nullptr);
      kernel_s += ms / 1e3;
      solves++;
    }
    if (f.status == 0) fetch_dp(0, set, f);
  }

  /* PeakSegFPOP_dir(problem.dir, penalty.str) (R/PeakSegFPOP_dir.R:64-117 over
   * R/PeakSegFPOP_file.R:57-86): reuse consistent result files, else solve, then write
   * _timing.tsv.  The contig is parsed on the first model that is not cached. */
  int model(const char *pen_str, LossRow &row, bool &cached) {
    const DirModel m(dir, pen_str);
    cached = dir_cache_ok(m.bedGraph, m.pre, row);
    if (cached) return 0;
    const double t0 = wall_now();
    FileProblem fp = m.start();
    fp.status = parse_penalty(pen_str, fp.is_Inf, fp.penalty);
    if (fp.status) return fp.status;
    if (!parsed) {
      parse_status = read_bedGraph(m.norm.c_str(), cv);
      parsed = true;
    }
    if (parse_status) return parse_status;
    if (open_outputs_and_split(fp, cv)) {
      DpFetched f;
      solve(fp, f);
      fp.status = write_dp_outputs(fp, cv, f);
    }
    settle_status(fp);
    return finish_model(m, fp, wall_now() - t0, &row);
  }
};

}  // namespace

extern "C" int PeakSegFPOP_dir_batch(int n_problems, char **problem_dirs, char **penalty_strs,
                                     int *status_out, int *cached_out) {
  g_fanout.clear(n_problems);
  if (n_problems <= 0) return 0;
  const double t0 = wall_now();
  std::vector<DirModel> models;
  models.reserve((size_t)n_problems);
  for (int i = 0; i < n_problems; i++) models.emplace_back(problem_dirs[i], penalty_strs[i]);
  std::vector<FileProblem> fps;
  std::vector<int> todo;
  for (int i = 0; i < n_problems; i++) {
    LossRow row;
    const bool hit = dir_cache_ok(models[(size_t)i].bedGraph, models[(size_t)i].pre, row);
    if (cached_out) cached_out[i] = hit ? 1 : 0;
    if (status_out) status_out[i] = 0;
    if (hit) continue;
    fps.push_back(models[(size_t)i].start());
    todo.push_back(i);
  }
  if (!todo.empty()) solve_files((int)fps.size(), fps.data(), true);
  for (size_t k = 0; k < todo.size(); k++) g_fanout.entry_shard[(size_t)todo[k]] = fps[k].shard;
  /* seconds: the reference times each call on its own; here the problems of a batch run
   * concurrently, so each one is charged the batch's wall time in proportion to its data --
   * among the problems of its own shard under PEAKSEG_HIP_DEVICES, whose shards run side by
   * side (shard -1: no fan-out, or the problems no shard solved) */
  const double wall = wall_now() - t0;
  std::map<int, double> bins_of_shard;
  for (auto &fp : fps) bins_of_shard[fp.shard] += fp.status == 0 ? (double)fp.bases : 0.0;
  int first = 0;
  for (size_t k = 0; k < todo.size(); k++) {
    FileProblem &fp = fps[k];
    const double bins_total = bins_of_shard[fp.shard];
    const double seconds = bins_total > 0 ? wall * (double)fp.bases / bins_total : wall;
    const int st = finish_model(models[(size_t)todo[k]], fp, seconds, nullptr);
    if (status_out) status_out[todo[k]] = st;
    if (st && !first) first = st;
  }
  return first;
}
