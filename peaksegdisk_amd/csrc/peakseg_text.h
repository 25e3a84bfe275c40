/* peakseg_text.h -- what the host driver says and reads as text: last error and warning, the
 * PEAKSEG_HIP_TIMING switch and its clock, printing through R's or the shards' channel, HIP_TRY,
 * the reference's bedGraph and penalty parsing, R's paste() of a double. */
namespace {

/* PEAKSEG_HIP_TIMING=1: where a call spends its time, on stderr */
bool timing_on() { return getenv("PEAKSEG_HIP_TIMING") != nullptr; }

double wall_now() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

thread_local std::string g_last_error;
void (*g_print)(const char *) = nullptr;

void set_error(const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
}

/* Things a caller may want to know about a call that SUCCEEDED (a wait that ran into its bound,
 * a fallback taken): kept apart from the error text, which describes failures only. */
thread_local std::string g_last_warning;
void set_warning(const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_warning = buf;
  if (timing_on()) fprintf(stderr, "peakseg_hip warning: %s\n", buf);
}

void print_text(const char *text) {
  if (g_print) {
    g_print(text);
  } else {
    fputs(text, stdout);
  }
}

/* Text of the shard threads of a fanned-out call (PEAKSEG_HIP_DEVICES).  g_print is R's Rprintf,
 * which only R's own thread may call: a shard thread appends to its buffer, and the calling
 * thread prints the complete lines (drain) while it waits and again after the join. */
struct ShardText {
  std::mutex m;
  std::condition_variable cv; /* a line arrived, or a shard ended */
  std::vector<std::string> buf;
  int running = 0;

  void append(int shard, const char *text) {
    std::lock_guard<std::mutex> lk(m);
    buf[(size_t)shard] += text;
    if (strchr(text, '\n')) cv.notify_one();
  }
  void shard_done() {
    std::lock_guard<std::mutex> lk(m);
    running--;
    cv.notify_one();
  }
  /* on the calling thread: print complete lines until every shard has ended, then the rest */
  void drain() {
    std::unique_lock<std::mutex> lk(m);
    for (;;) {
      const bool last = running == 0;
      std::string out;
      for (auto &b : buf) {
        const size_t end = last ? b.size() : b.rfind('\n') + 1; /* npos + 1 == 0 */
        out.append(b, 0, end);
        b.erase(0, end);
      }
      if (!out.empty()) {
        lk.unlock();
        print_text(out.c_str());
        lk.lock();
      }
      if (last) return;
      cv.wait_for(lk, std::chrono::milliseconds(200));
    }
  }
};
thread_local ShardText *g_shard_text = nullptr;
thread_local int g_shard_index = -1;

void emit_text(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (g_shard_text) {
    g_shard_text->append(g_shard_index, buf);
  } else {
    print_text(buf);
  }
}

#define HIP_TRY(expr)                                                               \
  do {                                                                              \
    hipError_t e_ = (expr);                                                         \
    if (e_ != hipSuccess) {                                                         \
      set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return e_ == hipErrorOutOfMemory ? ERROR_DEVICE_MEMORY : ERROR_DEVICE_SOLVER; \
    }                                                                               \
  } while (0)

/* ---- bedGraph input (drv:160-209) ---------------------------------------------------- */

struct Coverage {
  std::vector<int> chromEnd, count, weight;
  std::string chrom; /* the last line's first column (drv:166,178) */
  int first_chromStart = -1;
  double cum_weight = 0.0, cum_weighted_count = 0.0;
  double min_log_mean = INFINITY, max_log_mean = -INFINITY;
  int n() const { return (int)count.size(); }
};

/* One bedGraph line the way the reference's sscanf("%s %d %d %d%s") sees it
 * (drv:175-178).  Returns the item count sscanf would return (-1 for an empty line). */
static int scan_line_sscanf(const char *line, char *chrom, int *chromStart, int *chromEnd,
                            int *coverage, char *extra) {
  /* the reference reads "%s" into char[100] buffers (drv:166-167); bounded here */
  return sscanf(line, "%99s %d %d %d%99s\n", chrom, chromStart, chromEnd, coverage, extra);
}

static inline bool is_ws(unsigned char c) {
  return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r';
}

/* Fast path for the lines real files consist of: token, three decimal integers of at most
 * nine digits (optional '-' / '+'), nothing else.  Returns false for anything it is not sure
 * about; the caller then lets sscanf decide, so behaviour is the reference's by
 * construction (tests/test_cabi_cpu.py fuzzes fast vs sscanf-only). */
static bool scan_line_fast(const char *p, const char *end, char *chrom, int *v) {
  while (p < end && is_ws((unsigned char)*p)) p++;
  const char *tok = p;
  while (p < end && !is_ws((unsigned char)*p)) p++;
  size_t len = (size_t)(p - tok);
  if (len == 0 || len > 99) return false;
  memcpy(chrom, tok, len);
  chrom[len] = 0;
  for (int k = 0; k < 3; k++) {
    const char *q = p;
    while (p < end && is_ws((unsigned char)*p)) p++;
    if (p == q) return false; /* the integer must be separated from the previous field */
    bool neg = false;
    if (p < end && (*p == '-' || *p == '+')) {
      neg = *p == '-';
      p++;
    }
    const char *d = p;
    int x = 0;
    while (p < end && *p >= '0' && *p <= '9') {
      x = x * 10 + (*p - '0');
      p++;
    }
    if (p == d || p - d > 9) return false;
    v[k] = neg ? -x : x;
  }
  while (p < end && is_ws((unsigned char)*p)) p++;
  return p == end; /* a fifth field: sscanf reports it */
}

/* Pass 1 of the reference (drv:173-205): same per-line conversions, same checks in the same
 * order; the whole file is read once and shared by every penalty of a batch.
 * use_fast = false forces the sscanf-only path (tests). */
int read_bedGraph_impl(const char *path, Coverage &cv, bool use_fast) {
  FILE *f = fopen(path, "rb");
  if (!f) return ERROR_UNABLE_TO_OPEN_BEDGRAPH;
  std::string buf;
  {
    char chunk[1 << 16];
    size_t got;
    while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) buf.append(chunk, got);
    fclose(f);
  }
  int chromStart = 0, chromEnd = 0, coverage = 0, items, line_i = 0;
  char chrom[100];
  char extra[100] = "";
  int prev_chromEnd = -1;
  int status = 0;
  std::string tmp;
  const char *p = buf.data(), *file_end = buf.data() + buf.size();
  while (p < file_end) { /* std::getline: up to '\n', the last line may lack it */
    const char *nl = (const char *)memchr(p, '\n', (size_t)(file_end - p));
    const char *line_end = nl ? nl : file_end;
    line_i++;
    int v[3];
    if (use_fast && scan_line_fast(p, line_end, chrom, v)) {
      chromStart = v[0];
      chromEnd = v[1];
      coverage = v[2];
      items = 4;
    } else {
      tmp.assign(p, (size_t)(line_end - p));
      /* an embedded NUL ends the line for sscanf, as line.c_str() does in the reference */
      items = scan_line_sscanf(tmp.c_str(), chrom, &chromStart, &chromEnd, &coverage, extra);
    }
    p = nl ? nl + 1 : file_end;
    if (items < 4) {
      emit_text("problem: %d items on line %d\n", items, line_i);
      status = ERROR_NOT_ENOUGH_COLUMNS;
      break;
    }
    if (0 < strlen(extra)) {
      status = ERROR_NON_INTEGER_DATA;
      break;
    }
    double weight = chromEnd - chromStart;
    cv.cum_weight += weight;
    cv.cum_weighted_count += weight * coverage;
    if (line_i == 1) {
      cv.first_chromStart = chromStart;
    } else if (chromStart != prev_chromEnd) {
      status = ERROR_INCONSISTENT_CHROMSTART_CHROMEND;
      break;
    }
    prev_chromEnd = chromEnd;
    double log_data = psd_log((double)coverage);
    if (log_data < cv.min_log_mean) cv.min_log_mean = log_data;
    if (cv.max_log_mean < log_data) cv.max_log_mean = log_data;
    cv.chromEnd.push_back(chromEnd);
    cv.count.push_back(coverage);
    cv.weight.push_back(chromEnd - chromStart);
  }
  if (status) return status;
  if (line_i == 0) return ERROR_NO_DATA;
  cv.chrom = chrom;
  return 0;
}

int read_bedGraph(const char *path, Coverage &cv) { return read_bedGraph_impl(path, cv, true); }

/* penalty string handling of drv:145-159 */
int parse_penalty(const char *s, bool &is_Inf, double &penalty) {
  is_Inf = strcmp(s, "Inf") == 0;
  char *end;
  errno = 0;
  penalty = strtod(s, &end);
  if (end == s) return ERROR_PENALTY_NOT_NUMERIC;
  if (is_Inf) return 0;
  if (!std::isfinite(penalty)) return ERROR_PENALTY_NOT_FINITE;
  if (penalty < 0) return ERROR_PENALTY_NEGATIVE;
  return 0;
}

/* R's paste()/as.character() of a double: 15 significant digits, trailing zeros dropped, the
 * narrower of fixed and scientific notation (R's formatReal with digits = 15).  The penalties
 * of sequentialSearch_dir reach the solver and the file names through this
 * (R/sequentialSearch_dir.R:43, R/PeakSegFPOP_dir.R:64), and write.table() formats
 * _timing.tsv the same way (R/PeakSegFPOP_dir.R:102-106). */
std::string r_paste_double(double x) {
  if (x != x) return "NaN";
  if (std::isinf(x)) return x > 0 ? "Inf" : "-Inf";
  if (x == 0) return "0";
  char buf[64];
  snprintf(buf, sizeof buf, "%.14e", x);
  const double target = strtod(buf, nullptr);
  int nsig = 15;
  for (int d = 1; d <= 15; d++) { /* fewest digits that reproduce the 15-digit value */
    snprintf(buf, sizeof buf, "%.*e", d - 1, x);
    if (strtod(buf, nullptr) == target) {
      nsig = d;
      break;
    }
  }
  snprintf(buf, sizeof buf, "%.*e", nsig - 1, x);
  const char *e = strchr(buf, 'e');
  const int kpower = e ? atoi(e + 1) : 0;
  const int neg = x < 0 ? 1 : 0;
  int left, rgt;
  if (kpower >= 0) {
    left = kpower + 1;
    rgt = nsig - kpower - 1;
    if (rgt < 0) rgt = 0;
  } else {
    left = 1;
    rgt = nsig - kpower - 1;
  }
  const int w_fixed = neg + left + (rgt > 0 ? rgt + 1 : 0);
  const int w_sci = neg + (nsig > 1 ? nsig + 1 : 1) + (abs(kpower) >= 100 ? 5 : 4);
  char out[400];
  if (w_fixed <= w_sci) {
    snprintf(out, sizeof out, "%.*f", rgt, x);
  } else {
    snprintf(out, sizeof out, "%.*e", nsig - 1, x);
  }
  return out;
}

}  // namespace

/* Tests: R's paste() of a double as this library formats penalties and timing files. */
extern "C" int peakseg_hip_paste_double(double x, char *buf, size_t buf_len) {
  std::string s = r_paste_double(x);
  if (!buf || buf_len == 0) return (int)s.size();
  snprintf(buf, buf_len, "%s", s.c_str());
  return (int)s.size();
}
