// heat3d-mi355x — the convective-wall forms of the lean K-step sweep ("tl" with
// StencilParams::wall and wall_beta): instantiation of the variants listed in
// stencil_tbl_conv_variants.inc, and the same list handed to the shared dispatch
// of the wall forms (stencil_tbl_form.hpp).  The kernel is the fourth textual
// inclusion of stencil_tbl_kernel.inc (stencil_tbl_impl.hpp, H3D_TBL_WALL 2): a
// unit of its own, so every other lean kernel, the insulated-wall forms
// included, keeps its code object.
#include "stencil_tbl_form.hpp"

namespace heat3d {
namespace hip {

#define H3D_VC(T, R, WY, K, Q, N, S) \
  template void launch_tbl<T, R, WY, K, Q, N, S, false, 0, 2>(const StencilParams&, const KernelSpec&, hipStream_t);
#include "stencil_tbl_conv_variants.inc"
#undef H3D_VC

#define H3D_VC(T, R, WY, K, Q, N, S) TblShape<T, R, WY, K, Q, N, S>,
using Listed = TblShapes<
#include "stencil_tbl_conv_variants.inc"
    TblShapesEnd>;
#undef H3D_VC
// every default spec runs its own shape
static constexpr std::array<TblRedirect, 0> kRedirects{};

template <>
bool lean_form_dispatch<false, 2>(DType t, const StencilParams* p, const KernelSpec& k, hipStream_t s, LeanShape* shape) {
  return dispatch_tbl_form<false, 2>(t, Listed{}, kRedirects, p, k, s, shape);
}

}  // namespace hip
}  // namespace heat3d
