/* penalty_fit.h -- the fits of a penalty-learning regression: interval regression with the squared
 * hinge (margin 1), an L1 penalty on the weights and an unpenalised intercept, over a
 * regularisation path and the folds of a cross-validation, all in one launch.
 *
 * Row i < n has the standardised features x_i (p of them) and the target [lo_i, hi_i] in
 * log(penalty), either limit may be infinite.  With phi(z) = (z - 1)^2 for z < 1, else 0, problem
 * (f, k) minimises over (w, b)
 *     (1/|S|) sum over i in S of  phi(f_i - lo_i) + phi(hi_i - f_i)   +   reg[k] |w|_1,
 *     f_i = b + w . x_i,
 * where S holds the rows whose fold is not f (f < F), or all rows (the last set of problems).  The
 * solver is the accelerated proximal gradient method (FISTA) from w = 0, b = 0 with the constant
 * step |S| / (4 Lambda) -- Lambda bounds the largest eigenvalue of the Gram matrix of [X 1] over
 * all rows, which dominates that of every subset, and phi'' <= 2 --, soft thresholding on w, and a
 * restart of the momentum when (y - x+) . (x+ - x) > 0.  Every CHECK iterations, and after the
 * last, one more gradient is taken at the iterate itself (not at the extrapolated point), and the
 * problem ends when c = max(|g_b|, max_j c_j) <= threshold, with
 *     c_j = |g_j + reg sign(w_j)|  where w_j != 0,      max(0, |g_j| - reg)  where w_j = 0:
 * the distance of the subgradient from zero, coordinate by coordinate.  The weights that leave are
 * the ones c was evaluated at.
 *
 * A workgroup of THREADS threads per problem; no workgroup waits for another.  A gradient at a
 * point (LDS) goes over the rows in chunks of CHUNK rows:
 *   residuals   thread t owns the rows t, t + THREADS, ... of the chunk, four at a time: f_i from
 *               b and the features in index order (the weights are broadcast reads of LDS, the
 *               features consecutive rows of a column: X is stored feature-major), then
 *               r_i = phi'(f_i - lo_i) - phi'(hi_i - f_i) for a training row, 0 for the others,
 *               into LDS;
 *   columns     wave v owns the features v, v + WAVES, ... (the intercept is feature p, a column of
 *               ones): its lanes go over the chunk's rows, four sums per lane, then a butterfly of
 *               shuffles, and lane 0 adds the chunk's sum to the feature's word in LDS.
 * Then wave 0 takes the step: lane j has weight j, every lane the intercept.  Every sum has an
 * order that (n, p) alone fix, there are no floating-point atomics, and nothing depends on where
 * a workgroup runs: a call's tables are the same bit for bit whenever it is made.
 *
 * After its last iteration a problem counts, over its validation rows (fold f; the all-rows
 * problems: over every row), the rows whose prediction lies outside their interval and sums
 * phi(f_i - lo_i) + phi(hi_i - f_i) over them.
 *
 * Algorithmic traffic: a gradient reads the 8 n p bytes of X twice (L2: 1.8 MB at 6144 x 36, and
 * every workgroup of the launch reads the same matrix) and lo, hi and fold once (20 n bytes).
 *
 * Written against psd_platform.h only: the SIMT emulator of tests/emu runs this source. */
#ifndef PSD_PENALTY_FIT_H
#define PSD_PENALTY_FIT_H

#include <math.h>

#include "psd_platform.h"

/* the loops over a thread's four rows: their bodies are independent.  The library is built with
 * -fno-unroll-loops, and this pragma is what unrolls them all the same: only then are the arrays of
 * Four indexed by constants and kept in registers -- without it they go to scratch memory */
#if defined(__clang__)
#define PSD_FIT_UNROLL _Pragma("unroll")
#else
#define PSD_FIT_UNROLL _Pragma("GCC unroll 4")
#endif

namespace psd {
namespace fit {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;
constexpr int MAX_FEATURES = 64;      /* a lane of wave 0 per weight */
constexpr int SLOTS = MAX_FEATURES + 1; /* the weights, then the intercept */
constexpr int ROWS_PER_THREAD = 24;
constexpr int CHUNK = THREADS * ROWS_PER_THREAD; /* 6144 rows: 48 KB of residuals in LDS */
constexpr int CHECK = 8;              /* iterations between two evaluations of the criterion */
constexpr int MAX_ROWS = 1 << 20;
constexpr int MAX_FOLDS = 16;
constexpr int MAX_REG = 256;

/* what ends a problem */
enum { GO_ON = 0, CONVERGED = 1, OUT_OF_ITERATIONS = 2 };

struct Args {
  int n, p, n_folds, n_reg; /* n_folds: F; the grid is n_sets * n_reg, the last set trains on all rows */
  int n_sets;               /* F + 1, or 1 when F = 1 (no validation: the all-rows problems alone) */
  int max_iterations;
  double threshold;
  /* in HBM (the address space is in the types: no FLAT instructions) */
  const gdouble *x;         /* feature-major: x[j * n + i] */
  const gdouble *lo, *hi;
  const gint *fold;
  const gdouble *reg;       /* n_reg */
  const gdouble *inv_rows;  /* per set: 1 / |S| */
  const gdouble *step;      /* per set: |S| / (4 Lambda) */
  gdouble *weights;         /* per problem p + 1: the weights, then the intercept */
  gint *iterations;
  gdouble *criterion;
  gint *converged;
  gull *incorrect;
  gdouble *hinge;
};

PSD_D double phi(double z) {
  const double d = z - 1.0;
  return z < 1.0 ? d * d : 0.0;
}
PSD_D double dphi(double z) { return z < 1.0 ? 2.0 * (z - 1.0) : 0.0; }

/* the sum (the largest) over the wave, in every lane: a + b and b + a are the same bits */
PSD_D double wave_sum(double v, int lane) {
  for (int off = 1; off < WAVE; off <<= 1) v += shfl_d(v, lane ^ off);
  return v;
}
PSD_D double wave_max(double v, int lane) {
  for (int off = 1; off < WAVE; off <<= 1) {
    const double o = shfl_d(v, lane ^ off);
    v = o > v ? o : v;
  }
  return v;
}
PSD_D long long wave_sum_i64(long long v, int lane) {
  for (int off = 1; off < WAVE; off <<= 1) {
    const unsigned lo = (unsigned)shfl_i((int)(unsigned)(unsigned long long)v, lane ^ off);
    const unsigned hi = (unsigned)shfl_i((int)(unsigned)((unsigned long long)v >> 32), lane ^ off);
    v += (long long)(((unsigned long long)hi << 32) | lo);
  }
  return v;
}

/* Four rows of a thread: loc[a] = base + a THREADS inside the chunk of `rows` rows at row0.  A row
 * past the chunk's end reads the thread's first row (base < rows) and is not used. */
struct Four {
  int loc[4];
  bool ok[4];
  long long at[4];
  double f[4];
};

/* f_i = b + sum over j in index order of w_j x_ij, at the point l_pt (weights, then intercept) */
PSD_D void predict_four(const Args &a, const double *l_pt, int base, long long row0, int rows, Four &q) {
PSD_FIT_UNROLL
  for (int k = 0; k < 4; k++) {
    q.loc[k] = base + k * THREADS;
    q.ok[k] = q.loc[k] < rows;
    q.at[k] = row0 + (q.ok[k] ? q.loc[k] : base);
    q.f[k] = l_pt[a.p];
  }
  for (int j = 0; j < a.p; j++) {
    const double w = l_pt[j];
    const gdouble *col = a.x + (long long)j * a.n;
PSD_FIT_UNROLL
    for (int k = 0; k < 4; k++) q.f[k] += w * col[q.at[k]];
  }
}

/* does row i train problem set `set`? */
PSD_D bool trains(const Args &a, int set, long long i) {
  return set == a.n_sets - 1 || a.fold[i] != set;
}

/* the residuals of the chunk's rows at l_pt into l_r (every thread its own rows) */
PSD_D void chunk_residuals(const Args &a, int set, const double *l_pt, long long row0, int rows,
                           double *l_r) {
  for (int base = (int)threadIdx.x; base < rows; base += 4 * THREADS) {
    Four q;
    predict_four(a, l_pt, base, row0, rows, q);
PSD_FIT_UNROLL
    for (int k = 0; k < 4; k++)
      if (q.ok[k]) {
        const long long i = q.at[k];
        const double r = dphi(q.f[k] - a.lo[i]) - dphi(a.hi[i] - q.f[k]);
        l_r[q.loc[k]] = trains(a, set, i) ? r : 0.0;
      }
  }
}

/* sum over the chunk's rows of r_i x_ij for the features of this wave, added to l_g[j]; the first
 * chunk starts the sums */
PSD_D void chunk_columns(const Args &a, long long row0, int rows, const double *l_r, double *l_g,
                         bool first) {
  const int lane = lane_id(), wave = uniform_i(wave_id());
  for (int j = wave; j <= a.p; j += WAVES) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (j < a.p) {
      const gdouble *col = a.x + (long long)j * a.n + row0;
      for (int base = lane; base < rows; base += 4 * WAVE) {
PSD_FIT_UNROLL
        for (int k = 0; k < 4; k++) {
          const int loc = base + k * WAVE;
          const bool ok = loc < rows;
          const double r = ok ? l_r[loc] : 0.0;
          s[k] += r * col[ok ? loc : base];
        }
      }
    } else { /* the intercept: a column of ones */
      for (int base = lane; base < rows; base += 4 * WAVE) {
PSD_FIT_UNROLL
        for (int k = 0; k < 4; k++) {
          const int loc = base + k * WAVE;
          s[k] += loc < rows ? l_r[loc] : 0.0;
        }
      }
    }
    const double sum = wave_sum((s[0] + s[1]) + (s[2] + s[3]), lane);
    if (lane == 0) l_g[j] = first ? sum : l_g[j] + sum;
  }
}

/* l_g[0 .. p] = the sums of r_i x_ij (the gradient of the smooth part times |S|) at l_pt.  Ends
 * behind a __syncthreads(): every thread may read l_g. */
PSD_D void gradient_sums(const Args &a, int set, const double *l_pt, double *l_r, double *l_g) {
  for (long long row0 = 0; row0 < a.n; row0 += CHUNK) {
    const int rows = a.n - row0 < CHUNK ? (int)(a.n - row0) : CHUNK;
    chunk_residuals(a, set, l_pt, row0, rows, l_r);
    __syncthreads();
    chunk_columns(a, row0, rows, l_r, l_g, row0 == 0);
    __syncthreads();
  }
}

__global__ __launch_bounds__(THREADS) void fit_kernel(Args a) {
  PSD_LDS double l_r[CHUNK];
  PSD_LDS double l_x[SLOTS]; /* the iterate */
  PSD_LDS double l_y[SLOTS]; /* the extrapolated point */
  PSD_LDS double l_g[SLOTS];
  PSD_LDS double l_wave[WAVES];
  PSD_LDS long long l_wave_count[WAVES];
  PSD_LDS double l_criterion;
  PSD_LDS int l_end;
  const int tid = (int)threadIdx.x, lane = lane_id(), wave = uniform_i(wave_id());
  const int problem = (int)blockIdx.x, set = problem / a.n_reg, p = a.p;
  const double reg = a.reg[problem % a.n_reg];
  const double inv_rows = a.inv_rows[set], step = a.step[set];
  if (tid < SLOTS) l_x[tid] = l_y[tid] = l_g[tid] = 0.0;
  __syncthreads();
  double t = 1.0; /* (wave 0's) */
  int it = 0, end = GO_ON;
  for (;;) {
    if (it % CHECK == 0 || it >= a.max_iterations) {
      gradient_sums(a, set, l_x, l_r, l_g);
      if (wave == 0) {
        double c = 0.0;
        if (lane < p) {
          const double g = l_g[lane] * inv_rows, w = l_x[lane];
          if (w != 0.0) {
            c = fabs(w > 0.0 ? g + reg : g - reg);
          } else {
            c = fabs(g) > reg ? fabs(g) - reg : 0.0;
          }
        }
        c = wave_max(c, lane);
        const double gb = fabs(l_g[p] * inv_rows);
        c = gb > c ? gb : c;
        if (lane == 0) {
          l_criterion = c;
          l_end = c <= a.threshold ? CONVERGED : (it >= a.max_iterations ? OUT_OF_ITERATIONS : GO_ON);
        }
      }
      __syncthreads();
      end = l_end; /* (the next write to l_end lies behind the barriers of a gradient) */
      if (end != GO_ON) break;
    }
    gradient_sums(a, set, l_y, l_r, l_g);
    if (wave == 0) {
      /* x+ = prox(y - step g); every lane takes the intercept's step, lane j < p weight j's */
      const double yb = l_y[p], xb = l_x[p];
      const double nb = yb - step * (l_g[p] * inv_rows);
      double y = 0.0, x = 0.0, nx = 0.0;
      if (lane < p) {
        y = l_y[lane];
        x = l_x[lane];
        const double u = y - step * (l_g[lane] * inv_rows), shrink = step * reg;
        nx = u > shrink ? u - shrink : (u < -shrink ? u + shrink : 0.0);
      }
      const double turn = wave_sum((y - nx) * (nx - x), lane) + (yb - nb) * (nb - xb);
      double keep = 0.0; /* the momentum */
      if (turn > 0.0) {
        t = 1.0;
      } else {
        const double nt = 0.5 * (1.0 + sqrt(1.0 + 4.0 * t * t));
        keep = (t - 1.0) / nt;
        t = nt;
      }
      if (lane < p) {
        l_x[lane] = nx;
        l_y[lane] = nx + keep * (nx - x);
      }
      if (lane == 0) {
        l_x[p] = nb;
        l_y[p] = nb + keep * (nb - xb);
      }
    }
    __syncthreads();
    it++;
  }
  /* what the problem leaves: the iterate the criterion was evaluated at */
  gdouble *out = a.weights + (long long)problem * (p + 1);
  if (tid <= p) out[tid] = l_x[tid];
  if (tid == 0) {
    a.iterations[problem] = it;
    a.criterion[problem] = l_criterion;
    a.converged[problem] = end == CONVERGED ? 1 : 0;
  }
  /* its validation rows: thread t the rows t, t + THREADS, ... in row order */
  long long wrong = 0;
  double loss = 0.0;
  const bool all_rows = set == a.n_sets - 1;
  for (int base = tid; base < a.n; base += 4 * THREADS) {
    Four q;
    predict_four(a, l_x, base, 0, a.n, q);
PSD_FIT_UNROLL
    for (int k = 0; k < 4; k++)
      if (q.ok[k] && (all_rows || a.fold[q.at[k]] == set)) {
        const double lo = a.lo[q.at[k]], hi = a.hi[q.at[k]];
        wrong += (q.f[k] < lo || q.f[k] > hi) ? 1 : 0;
        loss += phi(q.f[k] - lo) + phi(hi - q.f[k]);
      }
  }
  wrong = wave_sum_i64(wrong, lane);
  loss = wave_sum(loss, lane);
  if (lane == 0) {
    l_wave[wave] = loss;
    l_wave_count[wave] = wrong;
  }
  __syncthreads();
  if (tid == 0) { /* the waves in their order */
    for (int k = 1; k < WAVES; k++) {
      loss += l_wave[k];
      wrong += l_wave_count[k];
    }
    a.hinge[problem] = loss;
    a.incorrect[problem] = (unsigned long long)wrong;
  }
}

}  // namespace fit
}  // namespace psd
#endif
