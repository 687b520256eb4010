// heat3d-mi355x — the dispatch of the lean sweep's six forms (with or without a
// heat source; no, insulated or convective walls), written once.  Every form
// has a list (stencil_tbl_*_variants.inc) whose lines are instantiated exactly
// (the forms without walls by the stencil_tbl_part*.hip units, each wall form
// by a unit of its own: stencil_tbl_wall.hip, _conv, _wall_src, _conv_src) and
// handed, as types, to dispatch_tbl_form: the dispatch is the list, so what a
// form can launch is what it lists and nothing else.  What differs between the
// forms is data: the list, and the default shapes that run in another shape
// (TblRedirect).  The one thing beside the lists is the packed-pair kernel
// (stencil_tbp.hip), which only the form without source and walls has.
#pragma once

#include <array>
#include <type_traits>

#include "stencil_tbl_impl.hpp"

namespace heat3d {
namespace hip {

// one line of a variant list: H3D_Vx(Real, R, WY, K, Q, NTS, SW), and the edge
// role EW of an H3D_VE line (spec field 9; 0 on every other line)
template <typename T, int R, int WY, int K, int Q, int NTS, bool SW, int EW = 0>
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

// The dispatch of form (SRC, WALL): stencil_tbl.hip has <*, 0>, each wall
// form's unit its own.  kernels.hpp lean_dispatch is the table of the six.
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
  int EW = 0;
};

template <typename Real, bool SRC, int WALL, typename T, int R, int WY, int K, int Q, int NTS, bool SW, int EW>
bool launch_if_listed(TblShape<T, R, WY, K, Q, NTS, SW, EW>, const TblWant& w, const StencilParams* p, const KernelSpec& k,
                      hipStream_t s) {
  if constexpr (std::is_same_v<T, Real>) {  // (launch_tbl is named for the list's own lines only)
    if (w.R == R && w.WY == WY && w.K == K && w.Q == Q && w.O == NTS && w.SW == SW && w.EW == EW) {
      if (p) launch_tbl<Real, R, WY, K, Q, NTS, SW, SRC, EW, WALL>(*p, k, s);
      return true;
    }
  }
  return false;
}

// With a source or walls the default form is the one-value-per-lane lean
// kernel for fp32 too (the pair kernel has no such form): an unset V resolves
// to 1.  Without either, a spec resolving to V = 2 (two columns per lane: packed
// fp32 / 16-byte fp64 pairs) goes to the pair kernel, which reports no shape.
// The edge role is a field of a list line; no source or wall list has one.
// p == nullptr: only report whether the form of k exists (and its shape).
template <typename Real, bool SRC, int WALL, typename... Shapes, std::size_t N>
bool dispatch_tbl_form_t(TblShapes<Shapes...>, const std::array<TblRedirect, N>& redirects, const StencilParams* p,
                         const KernelSpec& k, hipStream_t s, LeanShape* shape) {
  constexpr bool f64 = sizeof(Real) == 8;
  constexpr DType t = f64 ? DType::F64 : DType::F32;
  constexpr bool pairs = !SRC && WALL == 0;
  KernelSpec k1 = k;
  if (!pairs && k1.V == 0) k1.V = 1;
  const KernelSpec r = k1.resolved(t);
  TblWant w{r.R, r.WY, k.K, r.NT, r.O > 0 ? r.O : 0, false, r.EW};
  for (const TblRedirect& d : redirects)
    if (d.f64 == f64 && d.K == w.K && d.R == w.R && d.WY == w.WY && d.O == w.O) {
      w.R = d.toR, w.WY = d.toWY;
      break;
    }
  LeanShape thin;
  if (p && lean_thin_slab(k.K, k.V == 0 && k.R == 0 && k.WY == 0 && k.NT == 0, p->box.extent(0), p->box.extent(1), &thin)) {
    w = TblWant{thin.R, thin.WY, k.K, 3, f64 ? 2 : 0, true};
  } else if (pairs && r.V == 2) {
    if (r.EW != 0) return false;  // (no edge role there)
    if (!p) return lean_pair_supported(t, k);
    stencil_lean_pair(t, *p, k, s);
    return true;
  } else if (r.V != 1 || r.WZ != 1) {
    return false;  // one value per lane, one wave across z
  }
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
