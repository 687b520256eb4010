// heat3d-mi355x — FTCS row kernels (see cpu_rows.hpp).  This file is compiled
// twice: as is (namespace rows_generic) and from cpu_rows_fma.cpp with
// H3D_ROWS_NS=rows_fma and -mfma -mavx2.
#include <cmath>

#include "cpu_rows.hpp"
#include "kernels.hpp"

#ifndef H3D_ROWS_NS
#define H3D_ROWS_NS rows_generic
#define H3D_ROWS_DISPATCH 1
#endif

namespace heat3d {
namespace cpu {
namespace H3D_ROWS_NS {

template <typename Real, bool SRC>
static inline double row(const Real* __restrict in, Real* __restrict out, const Real* __restrict src, int64_t n,
                         int64_t sx, int64_t sy, Real Dx, Real Dy, Real Dz) {
  double lres = 0.0;
  bool nan = false;
  for (int64_t k = 0; k < n; ++k) {
    const Real T = in[k];
    Real nv;
    if constexpr (SRC)
      nv = ftcs_update_src<Real>(T, in[k - sx], in[k + sx], in[k - sy], in[k + sy], in[k - 1], in[k + 1], Dx, Dy,
                                 Dz, src[k]);
    else
      nv = ftcs_update<Real>(T, in[k - sx], in[k + sx], in[k - sy], in[k + sy], in[k - 1], in[k + 1], Dx, Dy, Dz);
    out[k] = nv;
    const double d = resid_abs(nv, T);  // in the field's precision (kernels.hpp)
    nan |= d != d;
    lres = d > lres ? d : lres;
  }
  return nan ? std::nan("") : lres;
}

template <typename Real, bool SRC>
static inline double row_var(const Real* __restrict in, Real* __restrict out, const Real* __restrict h,
                             const Real* __restrict src, int64_t n, int64_t sx, int64_t sy, Real Dx, Real Dy,
                             Real Dz) {
  double lres = 0.0;
  bool nan = false;
  for (int64_t k = 0; k < n; ++k) {
    const Real T = in[k];
    Real nv = ftcs_update_var<Real>(T, in[k - sx], in[k + sx], in[k - sy], in[k + sy], in[k - 1], in[k + 1], h[k],
                                    h[k - sx], h[k + sx], h[k - sy], h[k + sy], h[k - 1], h[k + 1], Dx, Dy, Dz);
    if constexpr (SRC) nv = add_source<Real>(nv, src[k]);
    out[k] = nv;
    const double d = resid_abs(nv, T);
    nan |= d != d;
    lres = d > lres ? d : lres;
  }
  return nan ? std::nan("") : lres;
}

template <typename Real>
static inline double row_wall(const Real* __restrict in, Real* __restrict out, int64_t n, int64_t oxm, int64_t oxp,
                              int64_t oym, int64_t oyp, int64_t kzm, int64_t kzp, Real Dx, Real Dy, Real Dz) {
  double lres = 0.0;
  bool nan = false;
  for (int64_t k = 0; k < n; ++k) {
    const Real T = in[k];
    const Real zm = k == kzm ? T : in[k - 1], zp = k == kzp ? T : in[k + 1];
    const Real nv = ftcs_update<Real>(T, in[k + oxm], in[k + oxp], in[k + oym], in[k + oyp], zm, zp, Dx, Dy, Dz);
    out[k] = nv;
    const double d = resid_abs(nv, T);
    nan |= d != d;
    lres = d > lres ? d : lres;
  }
  return nan ? std::nan("") : lres;
}

double ftcs_row_wall_f64(const double* in, double* out, int64_t n, int64_t oxm, int64_t oxp, int64_t oym, int64_t oyp,
                         int64_t kzm, int64_t kzp, double Dx, double Dy, double Dz) {
  return row_wall<double>(in, out, n, oxm, oxp, oym, oyp, kzm, kzp, Dx, Dy, Dz);
}
double ftcs_row_wall_f32(const float* in, float* out, int64_t n, int64_t oxm, int64_t oxp, int64_t oym, int64_t oyp,
                         int64_t kzm, int64_t kzp, float Dx, float Dy, float Dz) {
  return row_wall<float>(in, out, n, oxm, oxp, oym, oyp, kzm, kzp, Dx, Dy, Dz);
}

// convective walls: as row_wall, with the ghost convective_ghost(T, beta, tinf)
// in place of T (beta: x-, x+, y-, y+, z-, z+; 0 on an insulated face)
template <typename Real>
static inline double row_conv(const Real* __restrict in, Real* __restrict out, int64_t n, int64_t oxm, int64_t oxp,
                              int64_t oym, int64_t oyp, int64_t kzm, int64_t kzp, const Real* beta, Real tinf, Real Dx,
                              Real Dy, Real Dz) {
  double lres = 0.0;
  bool nan = false;
  const Real bxm = beta[0], bxp = beta[1], bym = beta[2], byp = beta[3], bzm = beta[4], bzp = beta[5];
  for (int64_t k = 0; k < n; ++k) {
    const Real T = in[k];
    const Real d = tinf - T;
    const Real xm = oxm ? in[k + oxm] : h3d_fma(bxm, d, T), xp = oxp ? in[k + oxp] : h3d_fma(bxp, d, T);
    const Real ym = oym ? in[k + oym] : h3d_fma(bym, d, T), yp = oyp ? in[k + oyp] : h3d_fma(byp, d, T);
    const Real zm = k == kzm ? h3d_fma(bzm, d, T) : in[k - 1], zp = k == kzp ? h3d_fma(bzp, d, T) : in[k + 1];
    const Real nv = ftcs_update<Real>(T, xm, xp, ym, yp, zm, zp, Dx, Dy, Dz);
    out[k] = nv;
    const double r = resid_abs(nv, T);
    nan |= r != r;
    lres = r > lres ? r : lres;
  }
  return nan ? std::nan("") : lres;
}

double ftcs_row_conv_f64(const double* in, double* out, int64_t n, int64_t oxm, int64_t oxp, int64_t oym, int64_t oyp,
                         int64_t kzm, int64_t kzp, const double* beta, double tinf, double Dx, double Dy, double Dz) {
  return row_conv<double>(in, out, n, oxm, oxp, oym, oyp, kzm, kzp, beta, tinf, Dx, Dy, Dz);
}
double ftcs_row_conv_f32(const float* in, float* out, int64_t n, int64_t oxm, int64_t oxp, int64_t oym, int64_t oyp,
                         int64_t kzm, int64_t kzp, const float* beta, float tinf, float Dx, float Dy, float Dz) {
  return row_conv<float>(in, out, n, oxm, oxp, oym, oyp, kzm, kzp, beta, tinf, Dx, Dy, Dz);
}

// walls with a heat source: row_wall / row_conv with ftcs_update_src, the ghost
// substitution first and the source added to the finished update (the order of
// a single step on refreshed wall planes)
template <typename Real>
static inline double row_wall_src(const Real* __restrict in, Real* __restrict out, const Real* __restrict src,
                                  int64_t n, int64_t oxm, int64_t oxp, int64_t oym, int64_t oyp, int64_t kzm,
                                  int64_t kzp, Real Dx, Real Dy, Real Dz) {
  double lres = 0.0;
  bool nan = false;
  for (int64_t k = 0; k < n; ++k) {
    const Real T = in[k];
    const Real zm = k == kzm ? T : in[k - 1], zp = k == kzp ? T : in[k + 1];
    const Real nv =
        ftcs_update_src<Real>(T, in[k + oxm], in[k + oxp], in[k + oym], in[k + oyp], zm, zp, Dx, Dy, Dz, src[k]);
    out[k] = nv;
    const double d = resid_abs(nv, T);
    nan |= d != d;
    lres = d > lres ? d : lres;
  }
  return nan ? std::nan("") : lres;
}

double ftcs_row_wall_src_f64(const double* in, double* out, const double* src, int64_t n, int64_t oxm, int64_t oxp,
                             int64_t oym, int64_t oyp, int64_t kzm, int64_t kzp, double Dx, double Dy, double Dz) {
  return row_wall_src<double>(in, out, src, n, oxm, oxp, oym, oyp, kzm, kzp, Dx, Dy, Dz);
}
double ftcs_row_wall_src_f32(const float* in, float* out, const float* src, int64_t n, int64_t oxm, int64_t oxp,
                             int64_t oym, int64_t oyp, int64_t kzm, int64_t kzp, float Dx, float Dy, float Dz) {
  return row_wall_src<float>(in, out, src, n, oxm, oxp, oym, oyp, kzm, kzp, Dx, Dy, Dz);
}

template <typename Real>
static inline double row_conv_src(const Real* __restrict in, Real* __restrict out, const Real* __restrict src,
                                  int64_t n, int64_t oxm, int64_t oxp, int64_t oym, int64_t oyp, int64_t kzm,
                                  int64_t kzp, const Real* beta, Real tinf, Real Dx, Real Dy, Real Dz) {
  double lres = 0.0;
  bool nan = false;
  const Real bxm = beta[0], bxp = beta[1], bym = beta[2], byp = beta[3], bzm = beta[4], bzp = beta[5];
  for (int64_t k = 0; k < n; ++k) {
    const Real T = in[k];
    const Real d = tinf - T;
    const Real xm = oxm ? in[k + oxm] : h3d_fma(bxm, d, T), xp = oxp ? in[k + oxp] : h3d_fma(bxp, d, T);
    const Real ym = oym ? in[k + oym] : h3d_fma(bym, d, T), yp = oyp ? in[k + oyp] : h3d_fma(byp, d, T);
    const Real zm = k == kzm ? h3d_fma(bzm, d, T) : in[k - 1], zp = k == kzp ? h3d_fma(bzp, d, T) : in[k + 1];
    const Real nv = ftcs_update_src<Real>(T, xm, xp, ym, yp, zm, zp, Dx, Dy, Dz, src[k]);
    out[k] = nv;
    const double r = resid_abs(nv, T);
    nan |= r != r;
    lres = r > lres ? r : lres;
  }
  return nan ? std::nan("") : lres;
}

double ftcs_row_conv_src_f64(const double* in, double* out, const double* src, int64_t n, int64_t oxm, int64_t oxp,
                             int64_t oym, int64_t oyp, int64_t kzm, int64_t kzp, const double* beta, double tinf,
                             double Dx, double Dy, double Dz) {
  return row_conv_src<double>(in, out, src, n, oxm, oxp, oym, oyp, kzm, kzp, beta, tinf, Dx, Dy, Dz);
}
double ftcs_row_conv_src_f32(const float* in, float* out, const float* src, int64_t n, int64_t oxm, int64_t oxp,
                             int64_t oym, int64_t oyp, int64_t kzm, int64_t kzp, const float* beta, float tinf,
                             float Dx, float Dy, float Dz) {
  return row_conv_src<float>(in, out, src, n, oxm, oxp, oym, oyp, kzm, kzp, beta, tinf, Dx, Dy, Dz);
}

double ftcs_row_f64(const double* in, double* out, int64_t n, int64_t sx, int64_t sy, double Dx, double Dy,
                    double Dz) {
  return row<double, false>(in, out, nullptr, n, sx, sy, Dx, Dy, Dz);
}
double ftcs_row_f32(const float* in, float* out, int64_t n, int64_t sx, int64_t sy, float Dx, float Dy, float Dz) {
  return row<float, false>(in, out, nullptr, n, sx, sy, Dx, Dy, Dz);
}
double ftcs_row_src_f64(const double* in, double* out, const double* src, int64_t n, int64_t sx, int64_t sy,
                        double Dx, double Dy, double Dz) {
  return row<double, true>(in, out, src, n, sx, sy, Dx, Dy, Dz);
}
double ftcs_row_src_f32(const float* in, float* out, const float* src, int64_t n, int64_t sx, int64_t sy, float Dx,
                        float Dy, float Dz) {
  return row<float, true>(in, out, src, n, sx, sy, Dx, Dy, Dz);
}

double ftcs_row_var_f64(const double* in, double* out, const double* cond, const double* src, int64_t n, int64_t sx,
                        int64_t sy, double Dx, double Dy, double Dz) {
  return src ? row_var<double, true>(in, out, cond, src, n, sx, sy, Dx, Dy, Dz)
             : row_var<double, false>(in, out, cond, nullptr, n, sx, sy, Dx, Dy, Dz);
}
double ftcs_row_var_f32(const float* in, float* out, const float* cond, const float* src, int64_t n, int64_t sx,
                        int64_t sy, float Dx, float Dy, float Dz) {
  return src ? row_var<float, true>(in, out, cond, src, n, sx, sy, Dx, Dy, Dz)
             : row_var<float, false>(in, out, cond, nullptr, n, sx, sy, Dx, Dy, Dz);
}

}  // namespace H3D_ROWS_NS

#ifdef H3D_ROWS_DISPATCH
const RowKernels& cpu_row_kernels() {
  static const RowKernels k = [] {
    __builtin_cpu_init();
    if (__builtin_cpu_supports("fma") && __builtin_cpu_supports("avx2"))
      return RowKernels{rows_fma::ftcs_row_f64, rows_fma::ftcs_row_f32, "x86-64+fma+avx2", rows_fma::ftcs_row_src_f64,
                        rows_fma::ftcs_row_src_f32, rows_fma::ftcs_row_var_f64, rows_fma::ftcs_row_var_f32,
                        rows_fma::ftcs_row_wall_f64, rows_fma::ftcs_row_wall_f32, rows_fma::ftcs_row_conv_f64,
                        rows_fma::ftcs_row_conv_f32, rows_fma::ftcs_row_wall_src_f64, rows_fma::ftcs_row_wall_src_f32,
                        rows_fma::ftcs_row_conv_src_f64, rows_fma::ftcs_row_conv_src_f32};
    return RowKernels{rows_generic::ftcs_row_f64, rows_generic::ftcs_row_f32, "x86-64 (libm fma)",
                      rows_generic::ftcs_row_src_f64, rows_generic::ftcs_row_src_f32, rows_generic::ftcs_row_var_f64,
                      rows_generic::ftcs_row_var_f32, rows_generic::ftcs_row_wall_f64, rows_generic::ftcs_row_wall_f32,
                      rows_generic::ftcs_row_conv_f64, rows_generic::ftcs_row_conv_f32,
                      rows_generic::ftcs_row_wall_src_f64, rows_generic::ftcs_row_wall_src_f32,
                      rows_generic::ftcs_row_conv_src_f64, rows_generic::ftcs_row_conv_src_f32};
  }();
  return k;
}
#endif

}  // namespace cpu
}  // namespace heat3d
