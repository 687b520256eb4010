// heat3d-mi355x — FTCS row kernels (see cpu_rows.hpp).  This file is compiled
// twice: as is (namespace rows_generic) and from cpu_rows_fma.cpp with
// H3D_ROWS_NS=rows_fma and -mfma -mavx2.
#include <cmath>

#include "cpu_rows.hpp"
#include "kernels.hpp"

#ifndef H3D_ROWS_NS
#define H3D_ROWS_NS rows_generic
#define H3D_ROWS_ISA "x86-64 (libm fma)"
#define H3D_ROWS_DISPATCH 1
#endif

namespace heat3d {
namespace cpu {
namespace H3D_ROWS_NS {

// The uniform update in the form (SRC, WALL).  Without walls the neighbours
// are at -sx, +sx, -sy, +sy and no element is compared with a wall coordinate.
// Behind insulated walls the ghost is the centre value itself, behind
// convective ones convective_ghost(T, beta, tinf) = fma(beta, tinf - T, T),
// which differs from T for a non-finite T even at beta = 0: two forms.  With a
// source, ftcs_update_src: the ghost substitution first and the source added to
// the finished update (the order of a single step on refreshed wall planes).
// (in, out and src are parameters of their own: __restrict on them is what
// lets the compiler carry in[k], in[k + 1] from one element to the next)
template <typename Real, bool SRC, WallKind WALL>
static inline double row_loop(const Real* __restrict in, Real* __restrict out,
                              [[maybe_unused]] const Real* __restrict src, const RowArgs<Real>& a) {
  const int64_t n = a.n;
  const Real Dx = a.Dx, Dy = a.Dy, Dz = a.Dz;
  [[maybe_unused]] const int64_t sx = a.sx, sy = a.sy;
  [[maybe_unused]] const int64_t oxm = a.oxm, oxp = a.oxp, oym = a.oym, oyp = a.oyp, kzm = a.kzm, kzp = a.kzp;
  [[maybe_unused]] Real bxm = 0, bxp = 0, bym = 0, byp = 0, bzm = 0, bzp = 0, tinf = 0;
  if constexpr (WALL == WallKind::Convective) {
    bxm = a.beta[0], bxp = a.beta[1], bym = a.beta[2], byp = a.beta[3], bzm = a.beta[4], bzp = a.beta[5];
    tinf = a.tinf;
  }
  double lres = 0.0;
  bool nan = false;
  for (int64_t k = 0; k < n; ++k) {
    const Real T = in[k];
    Real xm, xp, ym, yp, zm, zp;
    if constexpr (WALL == WallKind::None) {
      xm = in[k - sx], xp = in[k + sx], ym = in[k - sy], yp = in[k + sy], zm = in[k - 1], zp = in[k + 1];
    } else if constexpr (WALL == WallKind::Insulated) {
      xm = in[k + oxm], xp = in[k + oxp], ym = in[k + oym], yp = in[k + oyp];
      zm = k == kzm ? T : in[k - 1], zp = k == kzp ? T : in[k + 1];
    } else {
      const Real d = tinf - T;
      xm = oxm ? in[k + oxm] : h3d_fma(bxm, d, T), xp = oxp ? in[k + oxp] : h3d_fma(bxp, d, T);
      ym = oym ? in[k + oym] : h3d_fma(bym, d, T), yp = oyp ? in[k + oyp] : h3d_fma(byp, d, T);
      zm = k == kzm ? h3d_fma(bzm, d, T) : in[k - 1], zp = k == kzp ? h3d_fma(bzp, d, T) : in[k + 1];
    }
    Real nv;
    if constexpr (SRC) nv = ftcs_update_src<Real>(T, xm, xp, ym, yp, zm, zp, Dx, Dy, Dz, src[k]);
    else nv = ftcs_update<Real>(T, xm, xp, ym, yp, zm, zp, Dx, Dy, Dz);
    out[k] = nv;
    const double r = resid_abs(nv, T);  // in the field's precision (kernels.hpp)
    nan |= r != r;
    lres = r > lres ? r : lres;
  }
  return nan ? std::nan("") : lres;
}

template <typename Real, bool SRC, WallKind WALL>
static double row(const RowArgs<Real>& a) {
  return row_loop<Real, SRC, WALL>(a.in, a.out, a.src, a);
}

// The update with a conductivity in the form (SRC, WALL).  Behind a wall only
// the neighbour's temperature is replaced, exactly as in the uniform row above
// (the centre value behind an insulated face, convective_ghost behind a
// convective one); the face weights stay Ch[c] + Ch[neighbour], Ch read at the
// wall vertex.  Then ftcs_update_var, then the source: the order and the
// arithmetic of a single step on refreshed wall planes, so the flux through an
// insulated face is w * (c - c) = +0.
template <typename Real, bool SRC, WallKind WALL>
static inline double row_var_loop(const Real* __restrict in, Real* __restrict out, const Real* __restrict h,
                                  [[maybe_unused]] const Real* __restrict src, const RowArgs<Real>& a) {
  const int64_t n = a.n;
  const Real Dx = a.Dx, Dy = a.Dy, Dz = a.Dz;
  const int64_t sx = a.sx, sy = a.sy;
  [[maybe_unused]] const int64_t oxm = a.oxm, oxp = a.oxp, oym = a.oym, oyp = a.oyp, kzm = a.kzm, kzp = a.kzp;
  [[maybe_unused]] Real bxm = 0, bxp = 0, bym = 0, byp = 0, bzm = 0, bzp = 0, tinf = 0;
  if constexpr (WALL == WallKind::Convective) {
    bxm = a.beta[0], bxp = a.beta[1], bym = a.beta[2], byp = a.beta[3], bzm = a.beta[4], bzp = a.beta[5];
    tinf = a.tinf;
  }
  double lres = 0.0;
  bool nan = false;
  for (int64_t k = 0; k < n; ++k) {
    const Real T = in[k];
    Real xm, xp, ym, yp, zm, zp;
    if constexpr (WALL == WallKind::None) {
      xm = in[k - sx], xp = in[k + sx], ym = in[k - sy], yp = in[k + sy], zm = in[k - 1], zp = in[k + 1];
    } else if constexpr (WALL == WallKind::Insulated) {
      xm = in[k + oxm], xp = in[k + oxp], ym = in[k + oym], yp = in[k + oyp];
      zm = k == kzm ? T : in[k - 1], zp = k == kzp ? T : in[k + 1];
    } else {
      const Real d = tinf - T;
      xm = oxm ? in[k + oxm] : h3d_fma(bxm, d, T), xp = oxp ? in[k + oxp] : h3d_fma(bxp, d, T);
      ym = oym ? in[k + oym] : h3d_fma(bym, d, T), yp = oyp ? in[k + oyp] : h3d_fma(byp, d, T);
      zm = k == kzm ? h3d_fma(bzm, d, T) : in[k - 1], zp = k == kzp ? h3d_fma(bzp, d, T) : in[k + 1];
    }
    Real nv = ftcs_update_var<Real>(T, xm, xp, ym, yp, zm, zp, h[k], h[k - sx], h[k + sx], h[k - sy], h[k + sy],
                                    h[k - 1], h[k + 1], Dx, Dy, Dz);
    if constexpr (SRC) nv = add_source<Real>(nv, src[k]);
    out[k] = nv;
    const double d = resid_abs(nv, T);
    nan |= d != d;
    lres = d > lres ? d : lres;
  }
  return nan ? std::nan("") : lres;
}

template <typename Real, bool SRC, WallKind WALL>
static double row_var(const RowArgs<Real>& a) {
  return row_var_loop<Real, SRC, WALL>(a.in, a.out, a.cond, a.src, a);
}

// The update with a heat capacity (StencilParams::cap) in the form (COND, SRC,
// WALL): the same ghost substitution, then the increment of the step started
// from zero (steady_increment / steady_increment_var), the source added to it,
// and cap_update: T' = fma(s, u, T) with s read at the updated point only.
template <typename Real, bool COND, bool SRC, WallKind WALL>
static inline double row_cap_loop(const Real* __restrict in, Real* __restrict out,
                                  [[maybe_unused]] const Real* __restrict h,
                                  [[maybe_unused]] const Real* __restrict src, const Real* __restrict cap,
                                  const RowArgs<Real>& a) {
  const int64_t n = a.n;
  const Real Dx = a.Dx, Dy = a.Dy, Dz = a.Dz;
  const int64_t sx = a.sx, sy = a.sy;
  [[maybe_unused]] const int64_t oxm = a.oxm, oxp = a.oxp, oym = a.oym, oyp = a.oyp, kzm = a.kzm, kzp = a.kzp;
  [[maybe_unused]] Real bxm = 0, bxp = 0, bym = 0, byp = 0, bzm = 0, bzp = 0, tinf = 0;
  if constexpr (WALL == WallKind::Convective) {
    bxm = a.beta[0], bxp = a.beta[1], bym = a.beta[2], byp = a.beta[3], bzm = a.beta[4], bzp = a.beta[5];
    tinf = a.tinf;
  }
  double lres = 0.0;
  bool nan = false;
  for (int64_t k = 0; k < n; ++k) {
    const Real T = in[k];
    Real xm, xp, ym, yp, zm, zp;
    if constexpr (WALL == WallKind::None) {
      xm = in[k - sx], xp = in[k + sx], ym = in[k - sy], yp = in[k + sy], zm = in[k - 1], zp = in[k + 1];
    } else if constexpr (WALL == WallKind::Insulated) {
      xm = in[k + oxm], xp = in[k + oxp], ym = in[k + oym], yp = in[k + oyp];
      zm = k == kzm ? T : in[k - 1], zp = k == kzp ? T : in[k + 1];
    } else {
      const Real d = tinf - T;
      xm = oxm ? in[k + oxm] : h3d_fma(bxm, d, T), xp = oxp ? in[k + oxp] : h3d_fma(bxp, d, T);
      ym = oym ? in[k + oym] : h3d_fma(bym, d, T), yp = oyp ? in[k + oyp] : h3d_fma(byp, d, T);
      zm = k == kzm ? h3d_fma(bzm, d, T) : in[k - 1], zp = k == kzp ? h3d_fma(bzp, d, T) : in[k + 1];
    }
    Real u;
    if constexpr (COND)
      u = steady_increment_var<Real>(T, xm, xp, ym, yp, zm, zp, h[k], h[k - sx], h[k + sx], h[k - sy], h[k + sy],
                                     h[k - 1], h[k + 1], Dx, Dy, Dz);
    else u = steady_increment<Real>(T, xm, xp, ym, yp, zm, zp, Dx, Dy, Dz);
    if constexpr (SRC) u = add_source<Real>(u, src[k]);
    const Real nv = cap_update<Real>(cap[k], u, T);
    out[k] = nv;
    const double d = resid_abs(nv, T);
    nan |= d != d;
    lres = d > lres ? d : lres;
  }
  return nan ? std::nan("") : lres;
}

template <typename Real, bool COND, bool SRC, WallKind WALL>
static double row_cap(const RowArgs<Real>& a) {
  return row_cap_loop<Real, COND, SRC, WALL>(a.in, a.out, a.cond, a.src, a.cap, a);
}

template <typename Real>
static constexpr RowTable<Real> make_table() {
  constexpr WallKind N = WallKind::None, I = WallKind::Insulated, C = WallKind::Convective;
  return {{{row<Real, false, N>, row<Real, false, I>, row<Real, false, C>},
           {row<Real, true, N>, row<Real, true, I>, row<Real, true, C>}},
          {{row_var<Real, false, N>, row_var<Real, false, I>, row_var<Real, false, C>},
           {row_var<Real, true, N>, row_var<Real, true, I>, row_var<Real, true, C>}},
          {{{row_cap<Real, false, false, N>, row_cap<Real, false, false, I>, row_cap<Real, false, false, C>},
            {row_cap<Real, false, true, N>, row_cap<Real, false, true, I>, row_cap<Real, false, true, C>}},
           {{row_cap<Real, true, false, N>, row_cap<Real, true, false, I>, row_cap<Real, true, false, C>},
            {row_cap<Real, true, true, N>, row_cap<Real, true, true, I>, row_cap<Real, true, true, C>}}}};
}

// (constant-initialised: nothing of this build runs before it is chosen)
const RowKernels table = {make_table<double>(), make_table<float>(), H3D_ROWS_ISA};

}  // namespace H3D_ROWS_NS

#ifdef H3D_ROWS_DISPATCH
const RowKernels& cpu_row_kernels() {
  static const bool fma = [] {
    __builtin_cpu_init();
    return __builtin_cpu_supports("fma") && __builtin_cpu_supports("avx2");
  }();
  return fma ? rows_fma::table : rows_generic::table;
}
#endif

}  // namespace cpu
}  // namespace heat3d
