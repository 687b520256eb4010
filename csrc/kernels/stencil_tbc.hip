// heat3d-mi355x — K-step temporally blocked sweeps with a spatially varying
// conductivity and a spatially varying heat capacity ("tc"):
// rc T_t = div(kappa grad T) + q, K time steps per HBM sweep.
//
// The tc kernel is the tv kernel (stencil_tbv.hip: same contract, geometry,
// rings, masks, residuals, x plan) with one more static field, s = dtype(1 / rc).
// The kernel text is shared (stencil_tbv_kernel.inc with H3D_TBV_CAP 1, included
// by stencil_tbv_impl.hpp); the tv kernels keep their code.  One stage at an
// updated point computes, in this order: the wall ghost substitution of the wall
// forms; the six face weights, each the one rounded add Ch[p] + Ch[q]; the
// increment u = fma(Dz, fz, fma(Dy, fy, Dx * fx)) (steady_increment_var: the
// chain starts from zero); u = add_source(u, S) with a source; and
// T' = cap_update(s, u, T) = fma(s, u, T).  Those are the functions of
// kernels.hpp that cpu::stencil_multi and the single steps of stencil_cap.hip
// call, so fields and all K residual slots are bitwise those of K single steps
// with p.cond and p.cap.
//
// s has no neighbours: stage s at step x reads it on plane x - s, on the wave's
// own R rows and the lane's own column.  It is loaded where it is used, as the
// source rows are (a buffer load on the same plane resource with the same
// clamped plane and row offsets): K planes of s in a register ring do not fit
// (register report and the shapes tried: profiles/capacity_sweeps.md).  A
// clamped value only ever feeds a masked-out result.
//
// This unit holds the forms without walls and the dispatch of every form; the
// wall forms are instantiated in stencil_tbc_wall.hip and stencil_tbc_conv.hip.
// Each form runs in the tv form's shape where that needs no scratch with the
// capacity loads added, else in one of fewer waves or rows that does not.
//
// Out of scope, as for tv: the fused convergence check, schedule tuning,
// last-residual-only variants, the edge role, thin-slab forms.  A capacity
// without a conductivity has no sweep: the uniform step's increment is
// steady_increment, whose bits a tc kernel on a constant Ch would not give.
#include "stencil_tbv_impl.hpp"

namespace heat3d {
namespace hip {

template <typename Real>
static bool dispatch(bool src, const StencilParams* p, const KernelSpec& k, hipStream_t s, LeanShape* shape) {
#define H3D_FORM(SRCB, KK, RR, YY) H3D_TBC_SHAPE(0, SRCB, KK, RR, YY)
  if constexpr (sizeof(Real) == 8) {
    H3D_FORM(false, 2, 2, 16)
    H3D_FORM(true, 2, 2, 16)
    H3D_FORM(false, 3, 2, 12)
    H3D_FORM(true, 3, 3, 8)    // 2 x 12 needs 52 B of scratch: the same 24-row tile on 8 waves
  } else {
    H3D_FORM(false, 2, 5, 16)
    H3D_FORM(true, 2, 4, 16)   // 5 x 16 needs 44 B of scratch
    H3D_FORM(false, 3, 4, 12)
    H3D_FORM(true, 3, 3, 12)   // 4 x 12 needs 8 B of scratch
  }
#undef H3D_FORM
  return false;
}

bool tbc_plain_dispatch(DType t, bool src, const StencilParams* p, const KernelSpec& k, hipStream_t s, LeanShape* shape) {
  return t == DType::F64 ? dispatch<double>(src, p, k, s, shape) : dispatch<float>(src, p, k, s, shape);
}

// The tc dispatch of any form (source flag and wall kind, StencilParams::form).
// Launches *p, or (p == nullptr) only reports whether the form of depth k.K is
// built; *shape, if given, receives its tile.
static bool dispatch_tbc(DType t, SweepForm form, const StencilParams* p, const KernelSpec& k, hipStream_t s,
                         LeanShape* shape = nullptr) {
  if (k.V || k.R || k.WZ || k.WY || k.NT || k.O > 0 || k.EW) return false;  // no shape fields
  switch (form.wall) {
    case WallKind::Insulated: return tbc_wall_dispatch(t, form.src, p, k, s, shape);
    case WallKind::Convective: return tbc_conv_dispatch(t, form.src, p, k, s, shape);
    default: break;
  }
  return tbc_plain_dispatch(t, form.src, p, k, s, shape);
}

bool cap_sweep_supported(DType t, const KernelSpec& k, SweepForm form, LeanShape* shape) {
  if (k.kind != KernelSpec::TBC) return false;
  return dispatch_tbc(t, form, nullptr, k, nullptr, shape);
}

int cap_sweep_max_depth(DType t, SweepForm form) {
  KernelSpec k;
  k.kind = KernelSpec::TBC;
  int best = 0;
  // (every depth up to the answer: a partial sweep runs a shallower one)
  for (k.K = 2; k.K <= 6 && cap_sweep_supported(t, k, form); ++k.K) best = k.K;
  return best;
}

static const char* tbc_form_name(SweepForm f) {
  switch (f.wall) {
    case WallKind::Insulated: return f.src ? "insulated walls and a source" : "insulated walls";
    case WallKind::Convective: return f.src ? "convective walls and a source" : "convective walls";
    default: return f.src ? "a source" : "no source";
  }
}

void stencil_cap_sweep(DType t, const StencilParams& p, const KernelSpec& k, void* stream) {
  HEAT3D_CHECK(k.kind == KernelSpec::TBC, "stencil_cap_sweep needs a tc kernel");
  if (!p.cap)
    HEAT3D_THROW("tc kernels need a heat-capacity field (" << k.str() << " without one; use "
                                                           << (p.cond ? "tv2 / tv3" : "tl2..tl6") << ")");
  if (!p.cond)
    HEAT3D_THROW("tc kernels need a conductivity field (" << k.str() << " without one): a heat capacity alone runs as "
                                                                       "single steps (tile | naive)");
  HEAT3D_CHECK(!p.fuse_check && !p.tune, "tc kernels have no fused check and no schedule tuning");
  if (p.box.empty()) return;
  const SweepForm form = p.form();
  if (!dispatch_tbc(t, form, &p, k, S(stream))) {
    if (form.wall != WallKind::None && dispatch_tbc(t, SweepForm{form.src, WallKind::None}, nullptr, k, nullptr))
      HEAT3D_THROW("tc kernel " << k.str() << " (" << dtype_name(t) << ") has no form with " << tbc_form_name(form)
                                << ": that form is not built (a shallower depth or single steps run it)");
    HEAT3D_THROW("unsupported tc kernel variant " << k.str() << " (" << dtype_name(t)
                                                  << "): tc2 and tc3, without shape fields");
  }
}

}  // namespace hip
}  // namespace heat3d
