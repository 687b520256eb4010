// heat3d-mi355x — K-step temporally blocked FTCS sweeps, lean form ("tl"):
// the dispatch of the forms without walls, z-stride planner and the public
// entry points.  The kernel and its launcher live in stencil_tbl_impl.hpp; the
// variants (listed in stencil_tbl_variants.inc and stencil_tbl_src_variants.inc)
// are instantiated by the stencil_tbl_part*.hip units so that they compile in
// parallel.
#include "stencil_tbl_form.hpp"

#include <array>
#include <map>
#include <mutex>

namespace heat3d {
namespace hip {

// every listed variant is instantiated elsewhere: declared before any use, so
// that this unit instantiates no sweep kernel
#define H3D_V(T, R, WY, K, Q, N, S, P) \
  extern template void launch_tbl<T, R, WY, K, Q, N, S>(const StencilParams&, const KernelSpec&, hipStream_t);
#define H3D_VE(T, R, WY, K, Q, N, S, EW, P) \
  extern template void launch_tbl<T, R, WY, K, Q, N, S, false, EW>(const StencilParams&, const KernelSpec&, hipStream_t);
#include "stencil_tbl_variants.inc"
#undef H3D_V
#undef H3D_VE
#define H3D_VS(T, R, WY, K, Q, N, S, P) \
  extern template void launch_tbl<T, R, WY, K, Q, N, S, true>(const StencilParams&, const KernelSpec&, hipStream_t);
#include "stencil_tbl_src_variants.inc"
#undef H3D_VS

// Tile stride along z.  64 - 2K stored columns per 64-lane tile, or — fp64
// only — the largest multiple of 8 below it, which starts every tile's stored
// strip on a 64-byte boundary: whole 64-B write segments instead of partial
// ones at both seams, worth 2-10% per sweep at equal tile counts (MI355X,
// fp64 K = 3: 768^3 +2%, 1000^3 +3.5%, 1280^3 +10%; tools/gpu_zs2.sh).  The
// narrower stride can add a tile column, so it is taken only where the
// x-plan model, with that gain, predicts a shorter sweep (1024^3: 56 of 58,
// +4.6%; 512^3 would cross a round of workgroups and keeps 58), and only for
// boxes of >= 500 x planes: the slab shares of the 4- and 8-GPU runs (250 and
// 122 interior planes) lost 13% and 8% with it in the phantom-rank proxy
// while the 2-GPU share (510 planes) gained 1.5%.
static int lean_z_stride_plan(int64_t nx, int64_t ny, int64_t nz, int K, int esize, int TY, int slots, int U, int L);
int lean_z_stride(int64_t nx, int64_t ny, int64_t nz, int K, int esize, int TY, int slots, int U, int L) {
  // memoised: every eager launch asks (the N > 1 schedule is eager)
  static std::mutex mu;
  static std::map<std::array<int64_t, 9>, int> memo;
  const std::array<int64_t, 9> key{nx, ny, nz, K, esize, TY, slots, U, L};
  {
    std::lock_guard<std::mutex> lk(mu);
    auto it = memo.find(key);
    if (it != memo.end()) return it->second;
  }
  const int zs = lean_z_stride_plan(nx, ny, nz, K, esize, TY, slots, U, L);
  std::lock_guard<std::mutex> lk(mu);
  memo[key] = zs;
  return zs;
}

static int lean_z_stride_plan(int64_t nx, int64_t ny, int64_t nz, int K, int esize, int TY, int slots, int U, int L) {
  const int wide = 64 - 2 * K;
  const int aligned = esize == 8 ? wide & ~7 : wide;
  if (aligned == wide || aligned <= 0 || nx < 500) return wide;
  const int64_t nyb = std::max<int64_t>(1, (ny + TY - 2 * K - 1) / (TY - 2 * K));
  auto cost = [&](int zs) {
    const int64_t tiles = std::max<int64_t>(1, (nz + zs - 1) / zs) * nyb;
    const XPlan p = L > 0 ? fixed_xplan(nx, tiles, L) : plan_x(nx, tiles, slots, 2 * (K - 1), U, L == -1);
    return tiling_cost(p, nx, tiles, slots, 2 * (K - 1), U);
  };
  constexpr double kAlignedGain = 0.92;
  return cost(aligned) * kAlignedGain < cost(wide) ? aligned : wide;
}

// The two forms without walls: their lists, as types, are their dispatch
// (stencil_tbl_form.hpp).  No default shape of theirs runs as another.
#define H3D_V(T, R, WY, K, Q, N, S, P) TblShape<T, R, WY, K, Q, N, S>,
#define H3D_VE(T, R, WY, K, Q, N, S, EW, P) TblShape<T, R, WY, K, Q, N, S, EW>,
using Listed = TblShapes<
#include "stencil_tbl_variants.inc"
    TblShapesEnd>;
#undef H3D_V
#undef H3D_VE
#define H3D_VS(T, R, WY, K, Q, N, S, P) TblShape<T, R, WY, K, Q, N, S>,
using ListedSrc = TblShapes<
#include "stencil_tbl_src_variants.inc"
    TblShapesEnd>;
#undef H3D_VS
static constexpr std::array<TblRedirect, 0> kRedirects{};

template <>
bool lean_form_dispatch<false, 0>(DType t, const StencilParams* p, const KernelSpec& k, hipStream_t s, LeanShape* shape) {
  return dispatch_tbl_form<false, 0>(t, Listed{}, kRedirects, p, k, s, shape);
}
template <>
bool lean_form_dispatch<true, 0>(DType t, const StencilParams* p, const KernelSpec& k, hipStream_t s, LeanShape* shape) {
  return dispatch_tbl_form<true, 0>(t, ListedSrc{}, kRedirects, p, k, s, shape);
}

bool lean_dispatch(DType t, SweepForm form, const StencilParams* p, const KernelSpec& k, void* stream, LeanShape* shape) {
  using Fn = bool (*)(DType, const StencilParams*, const KernelSpec&, hipStream_t, LeanShape*);
  static constexpr Fn forms[2][3] = {  // [src][wall]
      {lean_form_dispatch<false, 0>, lean_form_dispatch<false, 1>, lean_form_dispatch<false, 2>},
      {lean_form_dispatch<true, 0>, lean_form_dispatch<true, 1>, lean_form_dispatch<true, 2>}};
  return forms[form.src][(int)form.wall](t, p, k, S(stream), shape);
}

bool lean_supported(DType t, const KernelSpec& k, SweepForm form) {
  return (form.wall == WallKind::None || k.kind == KernelSpec::TBL) && lean_dispatch(t, form, nullptr, k, nullptr);
}

void stencil_lean(DType t, const StencilParams& p, const KernelSpec& k, void* stream) {
  refuse_conductivity(p, k);
  if (p.box.empty()) return;
  const SweepForm form = p.form();
  if (lean_dispatch(t, form, &p, k, stream)) return;
  const KernelSpec r = k.resolved(t);
  // a sweep next to an insulated wall never falls back to Dirichlet arithmetic
  // (nor, next to a convective one, to insulated arithmetic)
  if (form.wall != WallKind::None)
    HEAT3D_THROW("tl kernel variant " << r.str() << " (" << dtype_name(t) << ") has no "
                                      << (form.wall == WallKind::Convective ? "convective-wall" : "insulated-wall")
                                      << " form" << (form.src ? " with a heat source" : "")
                                      << "; with insulated or convective walls use the default --kernel2 (tl2, tl3 or tl4 "
                                         "without shape fields)");
  if (form.src)
    HEAT3D_THROW("tl kernel variant " << r.str() << " (" << dtype_name(t)
                                      << ") has no heat-source form; with a source use the default --kernel2 "
                                         "(tl2, tl3 or tl4 without shape fields)");
  HEAT3D_THROW("unsupported tl kernel variant V=" << r.V << " R=" << r.R << " WY=" << r.WY << " K=" << k.K
                                                  << " Q=" << r.NT);
}

void sweep(DType t, const StencilParams& p, const KernelSpec& k, void* stream) {
  HEAT3D_CHECK(k.multi_step(), "sweep needs a K-step kernel (tl2..tl6, tv2..tv3, tc2..tc3)");
  if (k.kind == KernelSpec::TBV) stencil_cond_sweep(t, p, k, stream);
  else if (k.kind == KernelSpec::TBC) stencil_cap_sweep(t, p, k, stream);
  else stencil_lean(t, p, k, stream);
}

// (every K-step launch comes through stencil_lean or stencil_lean_pair)
void refuse_conductivity(const StencilParams& p, const KernelSpec& k) {
  // (never the arithmetic of one capacity where the call has a capacity field)
  if (p.cap)
    HEAT3D_THROW("K-step sweep kernel " << k.str() << " has no heat-capacity form: with a capacity field every "
                                                     "iteration runs as a single step (tile | naive)");
  // nor do the pair kernel (spec field V = 2, asked for by name: with walls an
  // unset V means 1 for either dtype) and the tv kernels have a wall form;
  // stencil_lean goes on to the lean kernel's wall forms after this check
  if (p.has_walls() && (k.kind == KernelSpec::TBV || k.V == 2 || p.cond))
    HEAT3D_THROW("K-step sweep kernel " << k.str() << " has no insulated-wall form");
  if (p.cond)
    HEAT3D_THROW("K-step sweep kernel " << k.str() << " has no conductivity form: with a conductivity field every "
                                                     "iteration runs as a single step (tile | naive)");
}

}  // namespace hip
}  // namespace heat3d
