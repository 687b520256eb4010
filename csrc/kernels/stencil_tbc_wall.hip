// heat3d-mi355x — the insulated-wall forms of the tc sweep (K-step sweeps with a
// conductivity field and a heat capacity, stencil_tbc.hip): the kernel
// stencil_tbc_wall of stencil_tbv_impl.hpp, instantiated here, in a unit of its
// own.  Every shape computes the same bits; each form runs in the shape of the
// tv form where that needs no scratch, else in one of fewer waves or rows that
// does not (register report and the shapes tried: profiles/capacity_sweeps.md).
// A form that has no scratch-free shape of at least 8 waves would have no line:
// it would not be built, and the solver would run a shallower depth instead.
#include "stencil_tbv_impl.hpp"

namespace heat3d {
namespace hip {

template <typename Real>
static bool dispatch(bool src, const StencilParams* p, const KernelSpec& k, hipStream_t s, LeanShape* shape) {
#define H3D_FORM(SRCB, KK, RR, YY) H3D_TBC_SHAPE(1, SRCB, KK, RR, YY)
  if constexpr (sizeof(Real) == 8) {
    H3D_FORM(false, 2, 2, 16)
    H3D_FORM(true, 2, 2, 12)   // 2 x 16 needs 16 B of scratch
    H3D_FORM(false, 3, 3, 8)   // 2 x 12 needs 24 B of scratch: the same 24-row tile on 8 waves
    H3D_FORM(true, 3, 3, 8)    // 2 x 12 needs 88 B of scratch
  } else {
    H3D_FORM(false, 2, 4, 16)  // 5 x 16 needs 36 B of scratch
    H3D_FORM(true, 2, 4, 16)   // 5 x 16 needs 112 B of scratch
    H3D_FORM(false, 3, 3, 12)  // 4 x 12 needs 12 B of scratch
    H3D_FORM(true, 3, 3, 12)   // 4 x 12 needs 76 B of scratch
  }
#undef H3D_FORM
  return false;
}

bool tbc_wall_dispatch(DType t, bool src, const StencilParams* p, const KernelSpec& k, hipStream_t s, LeanShape* shape) {
  return t == DType::F64 ? dispatch<double>(src, p, k, s, shape) : dispatch<float>(src, p, k, s, shape);
}

}  // namespace hip
}  // namespace heat3d
