// heat3d-mi355x — the dispatch of the lean sweep's wall forms (insulated or
// convective walls, each with or without a heat source), written once.  Every
// form has a unit of its own (stencil_tbl_wall.hip, _conv, _wall_src,
// _conv_src) that instantiates exactly the variants of its list
// (stencil_tbl_*_variants.inc) and hands the same list, as types, to
// dispatch_tbl_form: the shapes a unit can launch are the shapes it lists and
// no others.  What differs between the forms is data: the list, and the
// default shapes that run in another shape (TblRedirect).
#pragma once

#include <array>
#include <type_traits>

#include "stencil_tbl_impl.hpp"

namespace heat3d {
namespace hip {

// one line of a variant list: H3D_Vx(Real, R, WY, K, Q, NTS, SW)
template <typename T, int R, int WY, int K, int Q, int NTS, bool SW>
struct TblShape {};
template <typename... Shapes>
struct TblShapes {};
// (closes the comma-separated expansion of a list; matches no dtype)
using TblShapesEnd = TblShape<void, 0, 0, 0, 0, 0, false>;

// A shape that spills in a form (the register reports are in
// profiles/wall_source_sweeps.md) runs in a shape of fewer waves that does not:
// the spec resolving to R x WY at depth K with store field O is launched, and
// listed, as toR x toWY.  Every shape computes the same bits.
struct TblRedirect {
  bool f64;
  int K, R, WY, O, toR, toWY;
};

// The dispatch of form (SRC, WALL): stencil_tbl.hip has <*, 0> (dispatch_tbl,
// dispatch_tbl_src), each wall form's unit its own.  kernels.hpp lean_dispatch
// is the table of the six.
template <bool SRC, int WALL>
bool lean_form_dispatch(DType t, const StencilParams* p, const KernelSpec& k, hipStream_t s, LeanShape* shape);
template <> bool lean_form_dispatch<false, 0>(DType, const StencilParams*, const KernelSpec&, hipStream_t, LeanShape*);
template <> bool lean_form_dispatch<true, 0>(DType, const StencilParams*, const KernelSpec&, hipStream_t, LeanShape*);
template <> bool lean_form_dispatch<false, 1>(DType, const StencilParams*, const KernelSpec&, hipStream_t, LeanShape*);
template <> bool lean_form_dispatch<true, 1>(DType, const StencilParams*, const KernelSpec&, hipStream_t, LeanShape*);
template <> bool lean_form_dispatch<false, 2>(DType, const StencilParams*, const KernelSpec&, hipStream_t, LeanShape*);
template <> bool lean_form_dispatch<true, 2>(DType, const StencilParams*, const KernelSpec&, hipStream_t, LeanShape*);

// what a spec asks for, in the fields of a list line
struct TblWant {
  int R, WY, K, Q, O;
  bool SW;
};

template <typename Real, bool SRC, int WALL, typename T, int R, int WY, int K, int Q, int NTS, bool SW>
bool launch_if_listed(TblShape<T, R, WY, K, Q, NTS, SW>, const TblWant& w, const StencilParams* p, const KernelSpec& k,
                      hipStream_t s) {
  if constexpr (std::is_same_v<T, Real>) {  // (launch_tbl is named for the list's own lines only)
    if (w.R == R && w.WY == WY && w.K == K && w.Q == Q && w.O == NTS && w.SW == SW) {
      if (p) launch_tbl<Real, R, WY, K, Q, NTS, SW, SRC, 0, WALL>(*p, k, s);
      return true;
    }
  }
  return false;
}

// With walls the default form is the one-value-per-lane lean kernel for fp32
// too (the pair kernel has no wall form): an unset V resolves to 1.
// p == nullptr: only report whether the form of k exists (and its shape).
template <typename Real, bool SRC, int WALL, typename... Shapes, std::size_t N>
bool dispatch_tbl_form_t(TblShapes<Shapes...>, const std::array<TblRedirect, N>& redirects, const StencilParams* p,
                         const KernelSpec& k, hipStream_t s, LeanShape* shape) {
  constexpr bool f64 = sizeof(Real) == 8;
  KernelSpec k1 = k;
  if (k1.V == 0) k1.V = 1;
  const KernelSpec r = k1.resolved(f64 ? DType::F64 : DType::F32);
  TblWant w{r.R, r.WY, k.K, r.NT, r.O > 0 ? r.O : 0, false};
  for (const TblRedirect& d : redirects)
    if (d.f64 == f64 && d.K == w.K && d.R == w.R && d.WY == w.WY && d.O == w.O) {
      w.R = d.toR, w.WY = d.toWY;
      break;
    }
  LeanShape thin;
  if (p && lean_thin_slab(k.K, k.V == 0 && k.R == 0 && k.WY == 0 && k.NT == 0, p->box.extent(0), p->box.extent(1), &thin))
    w = TblWant{thin.R, thin.WY, k.K, 3, f64 ? 2 : 0, true};
  else if (r.V != 1 || r.WZ != 1 || r.EW != 0)
    return false;  // (no pair form, no edge role)
  const bool ok = (launch_if_listed<Real, SRC, WALL>(Shapes{}, w, p, k, s) || ...);
  if (ok && shape) *shape = LeanShape{w.R, w.WY, w.SW};
  return ok;
}

template <bool SRC, int WALL, typename List, std::size_t N>
bool dispatch_tbl_form(DType t, List list, const std::array<TblRedirect, N>& redirects, const StencilParams* p,
                       const KernelSpec& k, hipStream_t s, LeanShape* shape) {
  return t == DType::F64 ? dispatch_tbl_form_t<double, SRC, WALL>(list, redirects, p, k, s, shape)
                         : dispatch_tbl_form_t<float, SRC, WALL>(list, redirects, p, k, s, shape);
}

}  // namespace hip
}  // namespace heat3d
