/* peakseg_fit.h -- the host side of the penalty-model fits (kernel: penalty_fit.h): the checks of
 * the arguments, one device buffer for everything, the launch between two events on a stream of
 * the call's own, the download.  The call is not tied to a problem set and keeps nothing on the
 * device. */

namespace {

thread_local float g_fit_ms = 0.f;

/* what a call holds on the device, released on every path */
struct FitDevice {
  void *buffer = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~FitDevice() {
    if (buffer) (void)hipFree(buffer);
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

/* 0, or ERROR_FIT_ARGUMENTS with the argument and the row in the error text; n_train: per fold f < F
 * the rows whose fold is not f */
int fit_check(int n, int p, const double *x_std, const double *lo, const double *hi, const int *fold,
              int n_folds, int n_reg, const double *reg, double gram_lambda_max, double threshold,
              int max_iterations, std::vector<long long> &n_train) {
  namespace pf = psd::fit;
  if (n < 2 || n >= pf::MAX_ROWS) {
    set_error("penalty_fit: n = %d rows (2 to 2^20 - 1)", n);
    return ERROR_FIT_ARGUMENTS;
  }
  if (p < 0 || p > pf::MAX_FEATURES) {
    set_error("penalty_fit: p = %d features (0 to %d)", p, pf::MAX_FEATURES);
    return ERROR_FIT_ARGUMENTS;
  }
  if (n_folds < 1 || n_folds > pf::MAX_FOLDS) {
    set_error("penalty_fit: n_folds = %d (1 to %d)", n_folds, pf::MAX_FOLDS);
    return ERROR_FIT_ARGUMENTS;
  }
  if (n_reg < 1 || n_reg > pf::MAX_REG) {
    set_error("penalty_fit: n_reg = %d regularizations (1 to %d)", n_reg, pf::MAX_REG);
    return ERROR_FIT_ARGUMENTS;
  }
  if (n_folds == 1 && n_reg != 1) {
    set_error("penalty_fit: n_reg = %d with n_folds = 1: without validation there is one "
              "regularization", n_reg);
    return ERROR_FIT_ARGUMENTS;
  }
  if ((p > 0 && !x_std) || !lo || !hi || !fold || !reg) {
    set_error("penalty_fit: a NULL array (x_std, lo, hi, fold, reg)");
    return ERROR_FIT_ARGUMENTS;
  }
  if (!(gram_lambda_max > 0) || !std::isfinite(gram_lambda_max)) {
    set_error("penalty_fit: gram_lambda_max = %g must be positive and finite", gram_lambda_max);
    return ERROR_FIT_ARGUMENTS;
  }
  if (!(threshold > 0) || !std::isfinite(threshold)) {
    set_error("penalty_fit: threshold = %g must be positive and finite", threshold);
    return ERROR_FIT_ARGUMENTS;
  }
  if (max_iterations <= 0) {
    set_error("penalty_fit: max_iterations = %d must be positive", max_iterations);
    return ERROR_FIT_ARGUMENTS;
  }
  for (int k = 0; k < n_reg; k++) {
    if (!(reg[k] >= 0) || !std::isfinite(reg[k])) {
      set_error("penalty_fit: reg[%d] = %g must be finite and not negative", k, reg[k]);
      return ERROR_FIT_ARGUMENTS;
    }
    if (k > 0 && !(reg[k] > reg[k - 1])) {
      set_error("penalty_fit: reg[%d] = %g does not exceed reg[%d] = %g: the regularizations must "
                "increase", k, reg[k], k - 1, reg[k - 1]);
      return ERROR_FIT_ARGUMENTS;
    }
  }
  std::vector<long long> in_fold((size_t)n_folds, 0);
  for (int i = 0; i < n; i++) {
    if (std::isnan(lo[i]) || std::isnan(hi[i])) {
      set_error("penalty_fit: row %d: a limit (lo, hi) is NaN", i);
      return ERROR_FIT_ARGUMENTS;
    }
    if (lo[i] > hi[i]) {
      set_error("penalty_fit: row %d: lo = %g exceeds hi = %g", i, lo[i], hi[i]);
      return ERROR_FIT_ARGUMENTS;
    }
    if (std::isinf(lo[i]) && std::isinf(hi[i])) {
      set_error("penalty_fit: row %d: both limits (lo, hi) are infinite: the row says nothing", i);
      return ERROR_FIT_ARGUMENTS;
    }
    if (fold[i] < 0 || fold[i] >= n_folds) {
      set_error("penalty_fit: row %d: fold = %d is outside 0 .. %d", i, fold[i], n_folds - 1);
      return ERROR_FIT_ARGUMENTS;
    }
    in_fold[(size_t)fold[i]]++;
  }
  for (int j = 0; j < p; j++)
    for (int i = 0; i < n; i++)
      if (!std::isfinite(x_std[(size_t)j * (size_t)n + (size_t)i])) {
        set_error("penalty_fit: row %d: x_std of feature %d is not finite", i, j);
        return ERROR_FIT_ARGUMENTS;
      }
  n_train.assign((size_t)n_folds, 0);
  for (int f = 0; f < n_folds; f++) {
    n_train[(size_t)f] = n - in_fold[(size_t)f];
    if (n_folds > 1 && n_train[(size_t)f] == 0) {
      set_error("penalty_fit: fold %d holds every row: it leaves no row to train on", f);
      return ERROR_FIT_ARGUMENTS;
    }
  }
  return 0;
}

/* 0 or a status; the arguments have been checked */
int fit_run(int device, int n, int p, const double *x_std, const double *lo, const double *hi,
            const int *fold, int n_folds, int n_reg, const double *reg, double gram_lambda_max,
            double threshold, int max_iterations, const std::vector<long long> &n_train,
            double *weights_out, int *iterations_out, double *criterion_out, int *converged_out,
            long long *incorrect_out, double *hinge_out) {
  namespace pf = psd::fit;
  const int n_sets = n_folds == 1 ? 1 : n_folds + 1;
  const size_t problems = (size_t)n_sets * (size_t)n_reg, cells = (size_t)n * (size_t)p;
  std::vector<double> inv_rows((size_t)n_sets), step((size_t)n_sets);
  for (int s = 0; s < n_sets; s++) {
    const double rows = (double)(s == n_sets - 1 ? (long long)n : n_train[(size_t)s]);
    inv_rows[(size_t)s] = 1.0 / rows;
    step[(size_t)s] = rows / (4.0 * gram_lambda_max);
  }
  /* one buffer: the doubles, the 64-bit counts, then the ints */
  size_t at = 0;
  auto take = [&at](size_t count, size_t width) {
    const size_t here = at;
    at += (count * width + 7) / 8 * 8;
    return here;
  };
  const size_t o_x = take(cells, 8), o_lo = take((size_t)n, 8), o_hi = take((size_t)n, 8),
               o_reg = take((size_t)n_reg, 8), o_inv = take((size_t)n_sets, 8),
               o_step = take((size_t)n_sets, 8);
  const size_t o_out = at; /* what the launch writes, zeroed in front of it */
  const size_t o_weights = take(problems * (size_t)(p + 1), 8), o_criterion = take(problems, 8),
               o_hinge = take(problems, 8), o_incorrect = take(problems, 8);
  const size_t o_iterations = take(problems, 4), o_converged = take(problems, 4);
  const size_t o_end = at;
  const size_t o_fold = take((size_t)n, 4);

  FitDevice d;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&d.stream));
  for (auto &e : d.ev) HIP_TRY(hipEventCreate(&e));
  HIP_TRY(hipMalloc(&d.buffer, at));
  char *base = (char *)d.buffer;
  if (cells) HIP_TRY(hipMemcpyAsync(base + o_x, x_std, cells * 8, hipMemcpyHostToDevice, d.stream));
  HIP_TRY(hipMemcpyAsync(base + o_lo, lo, (size_t)n * 8, hipMemcpyHostToDevice, d.stream));
  HIP_TRY(hipMemcpyAsync(base + o_hi, hi, (size_t)n * 8, hipMemcpyHostToDevice, d.stream));
  HIP_TRY(hipMemcpyAsync(base + o_fold, fold, (size_t)n * 4, hipMemcpyHostToDevice, d.stream));
  HIP_TRY(hipMemcpyAsync(base + o_reg, reg, (size_t)n_reg * 8, hipMemcpyHostToDevice, d.stream));
  HIP_TRY(hipMemcpyAsync(base + o_inv, inv_rows.data(), (size_t)n_sets * 8, hipMemcpyHostToDevice, d.stream));
  HIP_TRY(hipMemcpyAsync(base + o_step, step.data(), (size_t)n_sets * 8, hipMemcpyHostToDevice, d.stream));
  HIP_TRY(hipStreamSynchronize(d.stream)); /* (inv_rows and step leave this frame's vectors) */

  pf::Args a;
  a.n = n;
  a.p = p;
  a.n_folds = n_folds;
  a.n_reg = n_reg;
  a.n_sets = n_sets;
  a.max_iterations = max_iterations;
  a.threshold = threshold;
  a.x = (const gdouble *)(base + o_x);
  a.lo = (const gdouble *)(base + o_lo);
  a.hi = (const gdouble *)(base + o_hi);
  a.fold = (const gint *)(base + o_fold);
  a.reg = (const gdouble *)(base + o_reg);
  a.inv_rows = (const gdouble *)(base + o_inv);
  a.step = (const gdouble *)(base + o_step);
  a.weights = (gdouble *)(base + o_weights);
  a.criterion = (gdouble *)(base + o_criterion);
  a.hinge = (gdouble *)(base + o_hinge);
  a.incorrect = (gull *)(base + o_incorrect);
  a.iterations = (gint *)(base + o_iterations);
  a.converged = (gint *)(base + o_converged);

  HIP_TRY(hipEventRecord(d.ev[0], d.stream));
  HIP_TRY(hipMemsetAsync(base + o_out, 0, o_end - o_out, d.stream));
  hipLaunchKernelGGL(pf::fit_kernel, dim3((unsigned)problems), dim3(pf::THREADS), 0, d.stream, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(d.ev[1], d.stream));
  HIP_TRY(hipStreamSynchronize(d.stream));
  HIP_TRY(hipEventElapsedTime(&g_fit_ms, d.ev[0], d.ev[1]));

  if (weights_out)
    HIP_TRY(hipMemcpy(weights_out, base + o_weights, problems * (size_t)(p + 1) * 8, hipMemcpyDeviceToHost));
  if (criterion_out) HIP_TRY(hipMemcpy(criterion_out, base + o_criterion, problems * 8, hipMemcpyDeviceToHost));
  if (hinge_out) HIP_TRY(hipMemcpy(hinge_out, base + o_hinge, problems * 8, hipMemcpyDeviceToHost));
  if (incorrect_out) HIP_TRY(hipMemcpy(incorrect_out, base + o_incorrect, problems * 8, hipMemcpyDeviceToHost));
  if (iterations_out) HIP_TRY(hipMemcpy(iterations_out, base + o_iterations, problems * 4, hipMemcpyDeviceToHost));
  if (converged_out) HIP_TRY(hipMemcpy(converged_out, base + o_converged, problems * 4, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

extern "C" int peakseg_hip_penalty_fit(int device, int n, int p, const double *x_std, const double *lo,
                                       const double *hi, const int *fold, int n_folds, int n_reg,
                                       const double *reg, double gram_lambda_max, double threshold,
                                       int max_iterations, double *weights_out, int *iterations_out,
                                       double *criterion_out, int *converged_out,
                                       long long *incorrect_out, double *hinge_out) {
  g_fit_ms = 0.f;
  std::vector<long long> n_train;
  int st = fit_check(n, p, x_std, lo, hi, fold, n_folds, n_reg, reg, gram_lambda_max, threshold,
                     max_iterations, n_train);
  if (st) return st;
  if (peakseg_hip_device_count() <= device || device < 0) {
    set_error("no HIP device %d visible (this library has no CPU fallback)", device);
    return ERROR_NO_HIP_DEVICE;
  }
  return fit_run(device, n, p, x_std, lo, hi, fold, n_folds, n_reg, reg, gram_lambda_max, threshold,
                 max_iterations, n_train, weights_out, iterations_out, criterion_out, converged_out,
                 incorrect_out, hinge_out);
}

extern "C" int peakseg_hip_penalty_fit_last_ms(float *ms) {
  if (ms) *ms = g_fit_ms;
  return 0;
}

extern "C" int peakseg_hip_penalty_fit_max_features(void) { return psd::fit::MAX_FEATURES; }
