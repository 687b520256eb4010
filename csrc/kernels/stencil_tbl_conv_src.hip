// heat3d-mi355x — the convective-wall forms of the lean K-step sweep with a heat
// source ("tl" with StencilParams::wall, wall_beta and src): instantiation of the
// variants listed in stencil_tbl_conv_src_variants.inc, and the same list handed
// to the shared dispatch of the wall forms (stencil_tbl_form.hpp).  The kernel is
// the sixth textual inclusion of stencil_tbl_kernel.inc (stencil_tbl_impl.hpp,
// H3D_TBL_SRC 1 with H3D_TBL_WALL 2): a unit of its own, so every other lean
// kernel keeps its code object.
#include "stencil_tbl_form.hpp"

namespace heat3d {
namespace hip {

#define H3D_VCS(T, R, WY, K, Q, N, S) \
  template void launch_tbl<T, R, WY, K, Q, N, S, true, 0, 2>(const StencilParams&, const KernelSpec&, hipStream_t);
#include "stencil_tbl_conv_src_variants.inc"
#undef H3D_VCS

#define H3D_VCS(T, R, WY, K, Q, N, S) TblShape<T, R, WY, K, Q, N, S>,
using Listed = TblShapes<
#include "stencil_tbl_conv_src_variants.inc"
    TblShapesEnd>;
#undef H3D_VCS
// the default shapes that spill in this form, and the listed shape each runs in
static constexpr std::array<TblRedirect, 5> kRedirects{{
    {true, 3, 3, 16, 2, 4, 12},                      // fp64 K = 3: 48-row tiles still
    {true, 4, 3, 12, 2, 5, 8},                       // fp64 K = 4: 40-row tiles for 36
    {true, 2, 5, 16, 2, 6, 12},                      // fp64 K = 2: 72-row tiles for 80,
    {true, 2, 5, 16, 2 | kResidualLastOnly, 6, 12},  // ... with the last residual only too
    {false, 4, 4, 16, 0, 4, 12},                     // fp32 K = 4: 48-row tiles for 64
}};

template <>
bool lean_form_dispatch<true, 2>(DType t, const StencilParams* p, const KernelSpec& k, hipStream_t s, LeanShape* shape) {
  return dispatch_tbl_form<true, 2>(t, Listed{}, kRedirects, p, k, s, shape);
}

}  // namespace hip
}  // namespace heat3d
