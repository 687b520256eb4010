// heat3d-mi355x — CPU inner row of the FTCS update, built twice.
//
// The update's fused multiply-adds (kernels.hpp ftcs_update) must be real,
// correctly rounded FMAs on the host too.  Compiled for baseline x86-64 they
// become libm fma() calls (exact, but ~15x slower and never vectorised), so
// the row loop lives in cpu_rows.cpp, which CMake builds once for baseline
// x86-64 and once with -mfma -mavx2 (cpu_rows_fma.cpp); cpu_row_kernels()
// picks the FMA build when the running CPU has FMA + AVX2.  Both builds give
// bitwise identical results.
//
// One row template covers the forms of the uniform update (kernels.hpp
// SweepForm: with or without a heat source, behind no, insulated or convective
// walls), a second one the same forms of the update with a conductivity field,
// a third one the forms with a heat capacity (with or without a conductivity).
// Every row has the same signature, and each build exports one table of them.
#pragma once

#include <cstdint>

#include "kernels.hpp"

namespace heat3d {
namespace cpu {

// One row: out[k] = the update of in[k] for k in [0, n).  A form reads the
// fields that concern it and ignores the others.
template <typename Real>
struct RowArgs {
  const Real* in;
  Real* out;
  int64_t n;
  Real Dx, Dy, Dz;
  const Real* src;   // heat source: src[k] is added to the finished update (ftcs_update_src)
  const Real* cond;  // conductivity form (ftcs_update_var; with src != nullptr ftcs_update_var_src)
  const Real* cap;   // heat-capacity forms only: s = dtype(1 / rc), cap[k] scales the increment (cap_update)
  int64_t sx, sy;    // strides of the x and y neighbours (the forms without walls)
  // walls (StencilParams::wall): the offsets of the x and y neighbours, 0 where
  // the neighbour's temperature across a wall is replaced by the ghost value
  // (the conductivity forms still read Ch at the wall vertex: sx, sy), and the row
  // indices whose z- / z+ neighbour is (-1 or beyond n: none).  The ghost is
  // the centre value behind insulated walls, convective_ghost(T, beta, tinf)
  // behind convective ones (the ghost substitution comes first, then the source)
  int64_t oxm, oxp, oym, oyp, kzm, kzp;
  // convective walls (StencilParams::wall_beta): the coefficients of the six
  // faces (x-, x+, y-, y+, z-, z+; 0 on an insulated one), the ambient temperature
  const Real* beta;
  Real tinf;
};

// returns max |out - in| over the row (NaN-propagating, as a double)
template <typename Real>
using RowFn = double (*)(const RowArgs<Real>&);

template <typename Real>
struct RowTable {
  RowFn<Real> row[2][3];  // [SweepForm::src][SweepForm::wall]
  RowFn<Real> var[2][3];  // the conductivity forms, by the same indices
  // the heat-capacity forms (StencilParams::cap): [conductivity][src][wall]
  RowFn<Real> cap[2][2][3];
  // the row of a call: its form, and whether it has a conductivity
  RowFn<Real> of(SweepForm f, bool cond) const { return (cond ? var : row)[f.src][(int)f.wall]; }
  // ... of a call with a heat capacity
  RowFn<Real> of_cap(SweepForm f, bool cond) const { return cap[cond][f.src][(int)f.wall]; }
};

struct RowKernels {
  RowTable<double> f64;
  RowTable<float> f32;
  const char* isa;
  template <typename Real>
  const RowTable<Real>& of() const {
    if constexpr (sizeof(Real) == 8) return f64;
    else return f32;
  }
};

// the table of the build this CPU runs
const RowKernels& cpu_row_kernels();

namespace rows_generic {
extern const RowKernels table;
}
namespace rows_fma {
extern const RowKernels table;
}

}  // namespace cpu
}  // namespace heat3d
