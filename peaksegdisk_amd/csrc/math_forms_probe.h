/* math_forms_probe.h -- tests only: every form of include/peakseg_detmath_core.h on the device,
 * element by element, for both sets of constants.
 *
 * The forward kernels reach the fused forms (psd_exp2, psd_log2, psd_exp2_log) and the branch-free
 * Newton forms (psd_exp_nb, psd_log_nb, psd_log_wild_nb) only inside whole solves, whose arguments
 * never leave the hot path.  This kernel hands each form caller-chosen arguments, so that a test can
 * put them on the edges of the tables, of the rounding of the exp's index and of the range, and can
 * lay rare arguments out lane by lane: a wave in which ONE lane is rare takes the wave-uniform slow
 * branch (PSD_ANY_LANE) with all its lanes, and the others must keep their hot-path value.
 *
 * Included once, outside the PSD_VARIANT namespaces: no forward kernel's code depends on it.
 * Written against psd_platform.h only: the SIMT emulator of tests/emu runs this source. */
#ifndef PSD_MATH_FORMS_PROBE_H
#define PSD_MATH_FORMS_PROBE_H

#include "psd_platform.h"

namespace psd {
namespace forms_probe {

constexpr int THREADS = 256;
constexpr int N_FORMS = 8; /* exp, log, exp2, log2, exp2_log, exp_nb, log_nb, log_wild_nb */
constexpr int N_SETS = 2;  /* 0: plain constants, 1: constants in vector registers (_vk) */

#define PSD_FORMS_PLAIN(name) name
#if defined(__HIP_DEVICE_COMPILE__)
#define PSD_FORMS_VK(name) name##_vk
#else
/* Where __HIP_DEVICE_COMPILE__ is not defined (the host pass of the compiler, and the emulator,
 * which compiles the host branch of the math headers) there is no _vk set: set 1 is the plain set. */
#define PSD_FORMS_VK(name) name
#endif

/* form f on one element; the outputs a form does not have, and *rare for the forms that keep no
 * record, stay as they are */
#define PSD_FORMS_EVAL(fn, M)                                                                       \
  PSD_D void fn(int f, double x0, double x1, double z, double *y0, double *y1, double *lz,          \
                int *rare) {                                                                        \
    switch (f) {                                                                                    \
      case 0: *y0 = M(psd_exp)(x0); break;                                                          \
      case 1: *y0 = M(psd_log)(x0); break;                                                          \
      case 2: M(psd_exp2)(x0, x1, y0, y1); break;                                                   \
      case 3: M(psd_log2)(x0, x1, y0, y1); break;                                                   \
      case 4: M(psd_exp2_log)(x0, x1, z, y0, y1, lz); break;                                        \
      case 5: *y0 = M(psd_exp_nb)(x0, rare); break;                                                 \
      case 6: *y0 = M(psd_log_nb)(x0, rare); break;                                                 \
      default: *y0 = M(psd_log_wild_nb)(x0, rare); break;                                           \
    }                                                                                               \
  }
PSD_FORMS_EVAL(eval_plain, PSD_FORMS_PLAIN)
PSD_FORMS_EVAL(eval_vk, PSD_FORMS_VK)
#undef PSD_FORMS_EVAL
#undef PSD_FORMS_PLAIN
#undef PSD_FORMS_VK

/* form and set are the same for every thread of the launch; every array has n elements */
__global__ __launch_bounds__(THREADS) void math_forms_probe_kernel(
    int form, int set, int n, const double *x0, const double *x1, const double *z, double *y0,
    double *y1, double *lz, int *rare) {
  psd_tables_init();
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n) {
    double r0 = 0.0, r1 = 0.0, rz = 0.0;
    int rec = 0;
    if (set == 0)
      eval_plain(form, x0[i], x1[i], z[i], &r0, &r1, &rz, &rec);
    else
      eval_vk(form, x0[i], x1[i], z[i], &r0, &r1, &rz, &rec);
    y0[i] = r0;
    y1[i] = r1;
    lz[i] = rz;
    rare[i] = rec;
  }
}

}  // namespace forms_probe
}  // namespace psd
#endif
