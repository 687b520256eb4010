// heat3d-mi355x — the convective-wall forms of the lean K-step sweep with a heat
// source ("tl" with StencilParams::wall, wall_beta and src): instantiation of the variants
// listed in stencil_tbl_conv_src_variants.inc and their dispatch.  The kernel is
// the sixth textual inclusion of stencil_tbl_kernel.inc (stencil_tbl_impl.hpp,
// H3D_TBL_SRC 1 with H3D_TBL_WALL 2): a unit of its own, so every other lean
// kernel keeps its code object.
#include "stencil_tbl_impl.hpp"

namespace heat3d {
namespace hip {

#define H3D_VCS(T, R, WY, K, Q, N, S) \
  template void launch_tbl<T, R, WY, K, Q, N, S, true, 0, 2>(const StencilParams&, const KernelSpec&, hipStream_t);
#include "stencil_tbl_conv_src_variants.inc"
#undef H3D_VCS

// As for the wall forms an unset V resolves to 1 for either dtype.
// p == nullptr: only report whether the form of k exists.
template <typename Real>
static bool dispatch_tbl_conv_src(const StencilParams* p, const KernelSpec& k, hipStream_t s) {
  constexpr bool f64 = sizeof(Real) == 8;
  KernelSpec k1 = k;
  if (k1.V == 0) k1.V = 1;
  const KernelSpec r = k1.resolved(f64 ? DType::F64 : DType::F32);
  const int K = k.K, Q = r.NT;
  const int O = r.O > 0 ? r.O : 0;
  int R = r.R, WY = r.WY;
  // The default shapes that spill in this form run in a shape of fewer waves
  // that does not (register report in profiles/wall_source_sweeps.md); the
  // list and the H3D_TBLCS lines below name the shape that runs.  Every shape
  // computes the same bits.
  if constexpr (f64) {
    if (K == 3 && R == 3 && WY == 16 && O == 2) R = 4, WY = 12;  // 48-row tiles still
    if (K == 4 && R == 3 && WY == 12 && O == 2) R = 5, WY = 8;  // 40-row tiles for 36
    if (K == 2 && R == 5 && WY == 16 && (O & ~kResidualLastOnly) == 2) R = 6, WY = 12;  // 72-row tiles for 80
  } else {
    if (K == 4 && R == 4 && WY == 16 && O == 0) R = 4, WY = 12;  // 48-row tiles for 64
  }
  if (p) {
    // the thin x slabs' y-marching tiles, chosen as dispatch_tbl chooses them
    const Box& bx = p->box;
    const bool dflt = k.V == 0 && k.R == 0 && k.WY == 0 && k.NT == 0;
    if (K == 3 && dflt && bx.extent(0) == 4 && bx.extent(1) >= 16 * bx.extent(0)) {
      launch_tbl<Real, 2, 5, 3, 3, f64 ? 2 : 0, true, true, 0, 2>(*p, k, s);
      return true;
    }
    if (K == 3 && dflt && bx.extent(0) > 0 && bx.extent(0) <= 2 * K && bx.extent(1) >= 16 * bx.extent(0)) {
      launch_tbl<Real, 3, 3, 3, 3, f64 ? 2 : 0, true, true, 0, 2>(*p, k, s);
      return true;
    }
    if (K == 4 && dflt && bx.extent(0) > 0 && bx.extent(0) <= K && bx.extent(1) >= 16 * bx.extent(0)) {
      launch_tbl<Real, 3, 4, 4, 3, f64 ? 2 : 0, true, true, 0, 2>(*p, k, s);
      return true;
    }
  }
  if (r.V != 1 || r.WZ != 1 || Q != 3 || r.EW != 0) return false;  // (no pair form, no edge role)
#define H3D_TBLCS(RR, YY, KK, AA)                                             \
  if (R == RR && WY == YY && K == KK && O == (AA)) {                          \
    if (p) launch_tbl<Real, RR, YY, KK, 3, (AA), false, true, 0, 2>(*p, k, s); \
    return true;                                                              \
  }
  if constexpr (f64) {
    H3D_TBLCS(4, 12, 3, 2) H3D_TBLCS(3, 16, 3, 2 | kResidualLastOnly)
    H3D_TBLCS(5, 8, 4, 2) H3D_TBLCS(3, 12, 4, 2 | kResidualLastOnly)
    H3D_TBLCS(6, 12, 2, 2) H3D_TBLCS(6, 12, 2, 2 | kResidualLastOnly)
  } else {
    H3D_TBLCS(3, 16, 3, 0) H3D_TBLCS(4, 12, 4, 0) H3D_TBLCS(3, 16, 2, 0)
  }
#undef H3D_TBLCS
  return false;
}

bool lean_conv_src_dispatch(DType t, const StencilParams* p, const KernelSpec& k, void* stream) {
  return t == DType::F64 ? dispatch_tbl_conv_src<double>(p, k, S(stream))
                         : dispatch_tbl_conv_src<float>(p, k, S(stream));
}

}  // namespace hip
}  // namespace heat3d
