// heat3d-mi355x — K-step temporally blocked sweeps with a spatially varying
// conductivity ("tv"): T_t = div(kappa grad T) + q, K time steps per HBM sweep.
//
// Same contract as the lean kernel (stencil_tbl_impl.hpp): one sweep turns T^n
// into T^{n+K} on p.box, the intermediate stages are computed on the update
// ranges, stage s records its residual in slot p.slot + s over the counting
// region of cpu::stencil_multi, and every point goes through the update of
// kernels.hpp, here ftcs_update_varw, so fields and residuals are bitwise those
// of K single steps with p.cond.  The geometry is the lean kernel's: 64-lane
// tiles storing up to 64 - 2K columns, WY waves of R rows marching x, a T^n ring
// of three planes, stage rings f[K-1][3][R], one LDS barrier per plane step for
// the y edge rows of every stage's centre plane, zero-fill DPP shifts for z,
// buffer loads with SGPR row offsets clamped to the live rows and planes.
//
// What is new is the static field Ch = dtype(0.5 c).  Stage s at step x works
// on plane x - s and reads Ch on planes x - s - 1 .. x - s + 1, so one register
// ring of the planes x - K .. x + 1, loaded once per plane step (two planes
// ahead, one at K = 4), serves every stage.  A wave keeps R + 2 rows of
// every Ch plane: its own and the two y neighbours of its edge rows, loaded
// directly (Ch is static; the neighbouring wave and tile load the same rows, so
// these are cache hits) instead of a second LDS exchange, for which the LDS of
// a 16-wave tile has no room.  Every face weight is formed where it is used, as
// the one rounded add Ch[p] + Ch[q]: the add commutes, so both cells of a face
// get the same bits, and the operands are exactly those ftcs_update_var adds on
// the CPU.  z neighbours of Ch come by the same zero-fill DPP as T's: lanes 0
// and 63 are outside every stage's cone.  Ch loads are clamped exactly as the T
// loads are; a clamped value only ever feeds a masked-out result.
//
// Behind insulated or convective walls the kernel has wall forms (the kernel
// text is stencil_tbv_kernel.inc, included once per form by
// stencil_tbv_impl.hpp; the wall forms are instantiated in stencil_tbv_wall.hip
// and stencil_tbv_conv.hip and dispatched from here).
//
// Out of scope here (the lean kernel has them): the fused convergence check,
// schedule tuning, last-residual-only variants, packed pairs, the edge role and
// the y-marching thin-slab forms.  Thin boxes are correct, not fast.
#include "stencil_tbv_impl.hpp"

namespace heat3d {
namespace hip {

// One shape per (dtype, K), with and without a heat source (register report:
// profiles/cond_sweeps.md).  p == nullptr: only report whether the form exists.
template <typename Real>
static bool dispatch_tbv_plain(bool q, const StencilParams* p, const KernelSpec& k, hipStream_t s, LeanShape* shape) {
#define H3D_TBV(RR, YY, KK)                                      \
  if (k.K == KK) {                                               \
    if (shape) *shape = LeanShape{RR, YY, false};                \
    if (p && q) launch_tbv<Real, RR, YY, KK, true>(*p, k, s);    \
    else if (p) launch_tbv<Real, RR, YY, KK, false>(*p, k, s);   \
    return true;                                                 \
  }
  if constexpr (sizeof(Real) == 8) {
    // 16 waves of 2 rows (128 VGPRs); K = 3: 12 waves (168).  Three rows per
    // wave spill at either depth, and no fp64 K = 4 shape of >= 8 waves fits
    H3D_TBV(2, 16, 2)
    H3D_TBV(2, 12, 3)
  } else {
    H3D_TBV(5, 16, 2)
    H3D_TBV(4, 12, 3)
  }
#undef H3D_TBV
  return false;
}

// The tv dispatch of any form (source flag and wall kind, StencilParams::form):
// the forms without walls from the list above, the wall forms from the lists of
// their units.  Launches *p, or (p == nullptr) only reports whether the form of
// depth k.K is built; *shape, if given, receives its tile.
static bool dispatch_tbv(DType t, SweepForm form, const StencilParams* p, const KernelSpec& k, hipStream_t s,
                         LeanShape* shape = nullptr) {
  if (k.V || k.R || k.WZ || k.WY || k.NT || k.O > 0 || k.EW) return false;  // no shape fields
  switch (form.wall) {
    case WallKind::Insulated: return tbv_wall_dispatch(t, form.src, p, k, s, shape);
    case WallKind::Convective: return tbv_conv_dispatch(t, form.src, p, k, s, shape);
    default: break;
  }
  return t == DType::F64 ? dispatch_tbv_plain<double>(form.src, p, k, s, shape)
                         : dispatch_tbv_plain<float>(form.src, p, k, s, shape);
}

bool cond_sweep_supported(DType t, const KernelSpec& k, SweepForm form, LeanShape* shape) {
  if (k.kind != KernelSpec::TBV) return false;
  return dispatch_tbv(t, form, nullptr, k, nullptr, shape);
}

bool cond_sweep_supported(DType t, const KernelSpec& k, bool with_source) {
  return cond_sweep_supported(t, k, SweepForm{with_source, WallKind::None});
}

int cond_sweep_max_depth(DType t, SweepForm form) {
  KernelSpec k;
  k.kind = KernelSpec::TBV;
  int best = 0;
  // (every depth up to the answer: a partial sweep runs a shallower one)
  for (k.K = 2; k.K <= 6 && cond_sweep_supported(t, k, form); ++k.K) best = k.K;
  return best;
}

static const char* tbv_form_name(SweepForm f) {
  switch (f.wall) {
    case WallKind::Insulated: return f.src ? "insulated walls and a source" : "insulated walls";
    case WallKind::Convective: return f.src ? "convective walls and a source" : "convective walls";
    default: return f.src ? "a source" : "no source";
  }
}

void stencil_cond_sweep(DType t, const StencilParams& p, const KernelSpec& k, void* stream) {
  HEAT3D_CHECK(k.kind == KernelSpec::TBV, "stencil_cond_sweep needs a tv kernel");
  if (!p.cond) HEAT3D_THROW("tv kernels need a conductivity field (" << k.str() << " without one; use tl2..tl6)");
  if (p.cap)
    HEAT3D_THROW("tv kernel " << k.str() << " has no heat-capacity form: with a capacity field use tc2 / tc3 (the tv "
                                            "sweep with a capacity), or single steps (tile | naive)");
  HEAT3D_CHECK(!p.fuse_check && !p.tune, "tv kernels have no fused check and no schedule tuning");
  if (p.box.empty()) return;
  const SweepForm form = p.form();
  if (!dispatch_tbv(t, form, &p, k, S(stream))) {
    if (form.wall != WallKind::None && dispatch_tbv(t, SweepForm{form.src, WallKind::None}, nullptr, k, nullptr))
      HEAT3D_THROW("tv kernel " << k.str() << " (" << dtype_name(t) << ") has no form with " << tbv_form_name(form)
                                << ": that form is not built (a shallower depth or single steps run it)");
    HEAT3D_THROW("unsupported tv kernel variant " << k.str() << " (" << dtype_name(t)
                                                  << "): tv2 and tv3, without shape fields");
  }
}

}  // namespace hip
}  // namespace heat3d
