// Array evaluators for the device-math tests (tests/libm_ref.py loads this as a shared object):
//   eval_libm      the host libm, one call per non-inlinable wrapper (GCC can then neither fold a call nor merge
//                  a sin and a cos of one argument into sincos), for the fn codes of clrrt_selftest_math;
//   eval_restated  the same switch as k_selftest_math (clrrt_kernels.hip), compiled for the host from
//                  clrrt_glibc.hpp / clrrt_glibcf.hpp.
// Float functions take (float)a, (float)b and return the float widened to double, as the hook does.
#define _GNU_SOURCE 1
#include <math.h>
#include <cmath>
#include <cstdint>
#include <limits>

#include "../../cl-rrt_amd/csrc/clrrt_glibc.hpp"
#include "../../cl-rrt_amd/csrc/clrrt_glibcf.hpp"

#define NI __attribute__((noinline)) static
NI double l_sin(double x) { return ::sin(x); }
NI double l_cos(double x) { return ::cos(x); }
NI double l_tan(double x) { return ::tan(x); }
NI double l_sqrt(double x) { return ::sqrt(x); }
NI double l_fmod(double x, double y) { return ::fmod(x, y); }
NI double l_atan2(double y, double x) { return ::atan2(y, x); }
NI double l_exp(double x) { return ::exp(x); }
NI double l_round(double x) { return ::round(x); }
NI void l_sincos(double x, double* s, double* c) { ::sincos(x, s, c); }
NI float l_cosf(float x) { return ::cosf(x); }
NI float l_sinf(float x) { return ::sinf(x); }
NI float l_atan2f(float y, float x) { return ::atan2f(y, x); }
NI float l_acosf(float x) { return ::acosf(x); }
NI float l_asinf(float x) { return ::asinf(x); }
NI float l_atanf(float x) { return ::atanf(x); }
NI float l_sqrtf(float x) { return ::sqrtf(x); }
NI double l_div(double x, double y) { return x / y; }
NI float l_fdiv(float x, float y) { return x / y; }

static const double kUnknown = std::numeric_limits<double>::quiet_NaN();

extern "C" void eval_libm(int fn, int n, const double* a, const double* b, double* out) {
  for (int i = 0; i < n; i++) {
    const double x = a[i], y = b[i];
    const float xf = (float)x, yf = (float)y;
    double r, s, c;
    switch (fn) {
      case 0: case 22: case 26: r = l_sin(x); break;
      case 1: case 23: case 27: r = l_cos(x); break;
      case 2: r = l_tan(x); break;
      case 3: r = l_sqrt(x); break;
      case 4: r = l_fmod(x, y); break;
      case 5: r = l_atan2(x, y); break;
      case 6: r = l_exp(x); break;
      case 7: r = l_div(x, y); break;
      case 8: r = (double)l_cosf(xf); break;
      case 9: r = (double)l_sinf(xf); break;
      case 10: r = (double)l_atan2f(xf, yf); break;
      case 11: r = (double)l_acosf(xf); break;
      case 12: r = (double)l_asinf(xf); break;
      case 13: r = (double)l_sqrtf(xf); break;
      case 14: r = (double)l_fdiv(xf, yf); break;
      case 15: r = l_round(x); break;
      case 16: case 20: case 24: l_sincos(x, &s, &c); r = s; break;
      case 17: case 21: case 25: l_sincos(x, &s, &c); r = c; break;
      case 28: r = l_tan(y); break;
      case 29: r = (double)l_atanf(xf); break;
      default: r = kUnknown; break;
    }
    out[i] = r;
  }
}

extern "C" void eval_restated(int fn, int n, const double* a, const double* b, double* out) {
  namespace glibc = clrrt::glibc;
  namespace glibcf = clrrt::glibcf;
  for (int i = 0; i < n; i++) {
    const double x = a[i], y = b[i];
    const float xf = (float)x, yf = (float)y;
    double r;
    switch (fn) {
      case 0: r = glibc::sin(x); break;
      case 1: r = glibc::cos(x); break;
      case 2: r = glibc::tan(x); break;
      case 3: r = ::sqrt(x); break;
      case 4: r = ::fmod(x, y); break;
      case 5: r = glibc::atan2(x, y); break;
      case 6: r = glibc::exp(x); break;
      case 7: r = x / y; break;
      case 8: { float sf, cf; glibc::sincosf(xf, sf, cf); r = (double)cf; } break;
      case 9: r = (double)glibc::sinf(xf); break;
      case 10: r = (double)glibcf::atan2f(xf, yf); break;
      case 11: r = (double)glibcf::acosf(xf); break;
      case 12: r = (double)glibcf::asinf(xf); break;
      case 13: r = (double)::sqrtf(xf); break;
      case 14: r = (double)(xf / yf); break;
      case 15: r = ::round(x); break;
      case 16: { double sx, cx; glibc::sincos(x, sx, cx); r = sx; } break;
      case 17: { double sx, cx; glibc::sincos(x, sx, cx); r = cx; } break;
      case 24: case 25: case 26: case 27: case 28: {
        double v[5];
        if (!glibc::step_trig(x, y, v[0], v[1], v[2], v[3], v[4])) {
          glibc::sincos_sel(x, v[0], v[1]);
          glibc::sin_cos_fma_sel(x, v[2], v[3]);
          v[4] = glibc::tan(y);
        }
        r = v[fn - 24];
      } break;
      case 20: { double sx, cx; glibc::sincos_sel(x, sx, cx); r = sx; } break;
      case 21: { double sx, cx; glibc::sincos_sel(x, sx, cx); r = cx; } break;
      case 22: { double sx, cx; glibc::sin_cos_fma_sel(x, sx, cx); r = sx; } break;
      case 23: { double sx, cx; glibc::sin_cos_fma_sel(x, sx, cx); r = cx; } break;
      case 29: r = (double)glibcf::atanf(xf); break;
      default: r = kUnknown; break;
    }
    out[i] = r;
  }
}
