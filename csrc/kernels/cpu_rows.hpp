// heat3d-mi355x — CPU inner row of the FTCS update, built twice.
//
// The update's fused multiply-adds (kernels.hpp ftcs_update) must be real,
// correctly rounded FMAs on the host too.  Compiled for baseline x86-64 they
// become libm fma() calls (exact, but ~15x slower and never vectorised), so
// the row loop lives in cpu_rows.cpp, which CMake builds once for baseline
// x86-64 and once with -mfma -mavx2 (cpu_rows_fma.cpp); cpu_row_kernels()
// picks the FMA build when the running CPU has FMA + AVX2.  Both builds give
// bitwise identical results.
#pragma once

#include <cstdint>

namespace heat3d {
namespace cpu {

// out[k] = ftcs_update(in[k], ...) for k in [0, n); returns max |out - in|
// (NaN-propagating, as a double).
template <typename Real>
using FtcsRowFn = double (*)(const Real* in, Real* out, int64_t n, int64_t sx, int64_t sy, Real Dx, Real Dy,
                             Real Dz);

// the same with a heat source: out[k] = ftcs_update_src(in[k], ..., src[k])
template <typename Real>
using FtcsRowSrcFn = double (*)(const Real* in, Real* out, const Real* src, int64_t n, int64_t sx, int64_t sy,
                                Real Dx, Real Dy, Real Dz);

// with a conductivity field: out[k] = ftcs_update_var(in[k], ..., cond[k], ...),
// plus src[k] where src != nullptr (ftcs_update_var_src)
template <typename Real>
using FtcsRowVarFn = double (*)(const Real* in, Real* out, const Real* cond, const Real* src, int64_t n, int64_t sx,
                                int64_t sy, Real Dx, Real Dy, Real Dz);

// insulated walls (StencilParams::wall): om / op are the offsets of the x and
// y neighbours (0 where the neighbour across a wall is replaced by the centre
// value), kzm / kzp the row indices whose z- / z+ neighbour is (-1: none)
template <typename Real>
using FtcsRowWallFn = double (*)(const Real* in, Real* out, int64_t n, int64_t oxm, int64_t oxp, int64_t oym,
                                 int64_t oyp, int64_t kzm, int64_t kzp, Real Dx, Real Dy, Real Dz);

// convective walls (StencilParams::wall_beta): as FtcsRowWallFn, with the
// coefficients of the six faces (x-, x+, y-, y+, z-, z+; 0 on an insulated one)
// and the ambient temperature
template <typename Real>
using FtcsRowConvFn = double (*)(const Real* in, Real* out, int64_t n, int64_t oxm, int64_t oxp, int64_t oym,
                                 int64_t oyp, int64_t kzm, int64_t kzp, const Real* beta, Real tinf, Real Dx, Real Dy,
                                 Real Dz);

// walls with a heat source: FtcsRowWallFn / FtcsRowConvFn with src[k] added to
// the finished update (ftcs_update_src; the ghost substitution comes first)
template <typename Real>
using FtcsRowWallSrcFn = double (*)(const Real* in, Real* out, const Real* src, int64_t n, int64_t oxm, int64_t oxp,
                                    int64_t oym, int64_t oyp, int64_t kzm, int64_t kzp, Real Dx, Real Dy, Real Dz);
template <typename Real>
using FtcsRowConvSrcFn = double (*)(const Real* in, Real* out, const Real* src, int64_t n, int64_t oxm, int64_t oxp,
                                    int64_t oym, int64_t oyp, int64_t kzm, int64_t kzp, const Real* beta, Real tinf,
                                    Real Dx, Real Dy, Real Dz);

struct RowKernels {
  FtcsRowFn<double> f64;
  FtcsRowFn<float> f32;
  const char* isa;
  FtcsRowSrcFn<double> src_f64;
  FtcsRowSrcFn<float> src_f32;
  FtcsRowVarFn<double> var_f64;
  FtcsRowVarFn<float> var_f32;
  FtcsRowWallFn<double> wall_f64;
  FtcsRowWallFn<float> wall_f32;
  FtcsRowConvFn<double> conv_f64;
  FtcsRowConvFn<float> conv_f32;
  FtcsRowWallSrcFn<double> wall_src_f64;
  FtcsRowWallSrcFn<float> wall_src_f32;
  FtcsRowConvSrcFn<double> conv_src_f64;
  FtcsRowConvSrcFn<float> conv_src_f32;
};

const RowKernels& cpu_row_kernels();

namespace rows_generic {
double ftcs_row_f64(const double*, double*, int64_t, int64_t, int64_t, double, double, double);
double ftcs_row_f32(const float*, float*, int64_t, int64_t, int64_t, float, float, float);
double ftcs_row_src_f64(const double*, double*, const double*, int64_t, int64_t, int64_t, double, double, double);
double ftcs_row_src_f32(const float*, float*, const float*, int64_t, int64_t, int64_t, float, float, float);
double ftcs_row_var_f64(const double*, double*, const double*, const double*, int64_t, int64_t, int64_t, double,
                        double, double);
double ftcs_row_var_f32(const float*, float*, const float*, const float*, int64_t, int64_t, int64_t, float, float,
                        float);
double ftcs_row_wall_f64(const double*, double*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, double,
                         double, double);
double ftcs_row_wall_f32(const float*, float*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, float,
                         float, float);
double ftcs_row_conv_f64(const double*, double*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                         const double*, double, double, double, double);
double ftcs_row_conv_f32(const float*, float*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                         const float*, float, float, float, float);
double ftcs_row_wall_src_f64(const double*, double*, const double*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                             int64_t, double, double, double);
double ftcs_row_wall_src_f32(const float*, float*, const float*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                             int64_t, float, float, float);
double ftcs_row_conv_src_f64(const double*, double*, const double*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                             int64_t, const double*, double, double, double, double);
double ftcs_row_conv_src_f32(const float*, float*, const float*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                             int64_t, const float*, float, float, float, float);
}  // namespace rows_generic
namespace rows_fma {
double ftcs_row_f64(const double*, double*, int64_t, int64_t, int64_t, double, double, double);
double ftcs_row_f32(const float*, float*, int64_t, int64_t, int64_t, float, float, float);
double ftcs_row_src_f64(const double*, double*, const double*, int64_t, int64_t, int64_t, double, double, double);
double ftcs_row_src_f32(const float*, float*, const float*, int64_t, int64_t, int64_t, float, float, float);
double ftcs_row_var_f64(const double*, double*, const double*, const double*, int64_t, int64_t, int64_t, double,
                        double, double);
double ftcs_row_var_f32(const float*, float*, const float*, const float*, int64_t, int64_t, int64_t, float, float,
                        float);
double ftcs_row_wall_f64(const double*, double*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, double,
                         double, double);
double ftcs_row_wall_f32(const float*, float*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, float,
                         float, float);
double ftcs_row_conv_f64(const double*, double*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                         const double*, double, double, double, double);
double ftcs_row_conv_f32(const float*, float*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                         const float*, float, float, float, float);
double ftcs_row_wall_src_f64(const double*, double*, const double*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                             int64_t, double, double, double);
double ftcs_row_wall_src_f32(const float*, float*, const float*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                             int64_t, float, float, float);
double ftcs_row_conv_src_f64(const double*, double*, const double*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                             int64_t, const double*, double, double, double, double);
double ftcs_row_conv_src_f32(const float*, float*, const float*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                             int64_t, const float*, float, float, float, float);
}  // namespace rows_fma

}  // namespace cpu
}  // namespace heat3d
