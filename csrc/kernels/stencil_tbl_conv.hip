// heat3d-mi355x — the convective-wall forms of the lean K-step sweep ("tl" with
// StencilParams::wall and wall_beta): instantiation of the variants listed in
// stencil_tbl_conv_variants.inc and their dispatch.  The kernel is the fourth
// textual inclusion of stencil_tbl_kernel.inc (stencil_tbl_impl.hpp,
// H3D_TBL_WALL 2): a unit of its own, so every other lean kernel, the
// insulated-wall forms included, keeps its code object.
#include "stencil_tbl_impl.hpp"

namespace heat3d {
namespace hip {

#define H3D_VC(T, R, WY, K, Q, N, S) \
  template void launch_tbl<T, R, WY, K, Q, N, S, false, 0, 2>(const StencilParams&, const KernelSpec&, hipStream_t);
#include "stencil_tbl_conv_variants.inc"
#undef H3D_VC

// As for insulated walls the default form is the one-value-per-lane lean
// kernel for fp32 too (the pair kernel has no wall form): an unset V resolves
// to 1.  p == nullptr: only report whether the convective form of k exists.
template <typename Real>
static bool dispatch_tbl_conv(const StencilParams* p, const KernelSpec& k, hipStream_t s) {
  constexpr bool f64 = sizeof(Real) == 8;
  KernelSpec k1 = k;
  if (k1.V == 0) k1.V = 1;
  const KernelSpec r = k1.resolved(f64 ? DType::F64 : DType::F32);
  const int K = k.K, R = r.R, WY = r.WY, Q = r.NT;
  if (p) {
    // the thin x slabs' y-marching tiles, chosen as dispatch_tbl chooses them
    const Box& bx = p->box;
    const bool dflt = k.V == 0 && k.R == 0 && k.WY == 0 && k.NT == 0;
    if (K == 3 && dflt && bx.extent(0) == 4 && bx.extent(1) >= 16 * bx.extent(0)) {
      launch_tbl<Real, 2, 5, 3, 3, f64 ? 2 : 0, true, false, 0, 2>(*p, k, s);
      return true;
    }
    if (K == 3 && dflt && bx.extent(0) > 0 && bx.extent(0) <= 2 * K && bx.extent(1) >= 16 * bx.extent(0)) {
      launch_tbl<Real, 3, 3, 3, 3, f64 ? 2 : 0, true, false, 0, 2>(*p, k, s);
      return true;
    }
    if (K == 4 && dflt && bx.extent(0) > 0 && bx.extent(0) <= K && bx.extent(1) >= 16 * bx.extent(0)) {
      launch_tbl<Real, 3, 4, 4, 3, f64 ? 2 : 0, true, false, 0, 2>(*p, k, s);
      return true;
    }
  }
  if (r.V != 1 || r.WZ != 1 || Q != 3 || r.EW != 0) return false;  // (no pair form, no edge role)
  const int O = r.O > 0 ? r.O : 0;
#define H3D_TBLC(RR, YY, KK, AA)                                               \
  if (R == RR && WY == YY && K == KK && O == (AA)) {                           \
    if (p) launch_tbl<Real, RR, YY, KK, 3, (AA), false, false, 0, 2>(*p, k, s); \
    return true;                                                               \
  }
  if constexpr (f64) {
    H3D_TBLC(3, 16, 3, 2) H3D_TBLC(3, 16, 3, 2 | kResidualLastOnly)
    H3D_TBLC(3, 12, 4, 2) H3D_TBLC(3, 12, 4, 2 | kResidualLastOnly)
    H3D_TBLC(5, 16, 2, 2) H3D_TBLC(5, 16, 2, 2 | kResidualLastOnly)
  } else {
    H3D_TBLC(3, 16, 3, 0) H3D_TBLC(4, 16, 4, 0) H3D_TBLC(3, 16, 2, 0)
  }
#undef H3D_TBLC
  return false;
}

bool lean_conv_dispatch(DType t, const StencilParams* p, const KernelSpec& k, void* stream) {
  return t == DType::F64 ? dispatch_tbl_conv<double>(p, k, S(stream)) : dispatch_tbl_conv<float>(p, k, S(stream));
}

}  // namespace hip
}  // namespace heat3d
