// heat3d-mi355x — instantiation unit 2 of the lean sweep kernel variants
// (stencil_tbl_variants.inc entries with PART = 2); see stencil_tbl.hip.
#include "stencil_tbl_impl.hpp"

namespace heat3d {
namespace hip {

#define H3D_SEL0(...)
#define H3D_SEL1(...)
#define H3D_SEL2(...)
#define H3D_SEL3(...)
#undef H3D_SEL2
#define H3D_SEL2(...) __VA_ARGS__
#define H3D_V(T, R, WY, K, Q, N, S, P) \
  H3D_SEL##P(template void launch_tbl<T, R, WY, K, Q, N, S>(const StencilParams&, const KernelSpec&, hipStream_t);)
#define H3D_VE(T, R, WY, K, Q, N, S, EW, P) \
  H3D_SEL##P(template void launch_tbl<T, R, WY, K, Q, N, S, false, EW>(const StencilParams&, const KernelSpec&, hipStream_t);)
#include "stencil_tbl_variants.inc"
#undef H3D_V
#undef H3D_VE
// ... and of the heat-source forms (stencil_tbl_src_variants.inc)
#define H3D_VS(T, R, WY, K, Q, N, S, P) \
  H3D_SEL##P(template void launch_tbl<T, R, WY, K, Q, N, S, true>(const StencilParams&, const KernelSpec&, hipStream_t);)
#include "stencil_tbl_src_variants.inc"
#undef H3D_VS

}  // namespace hip
}  // namespace heat3d
