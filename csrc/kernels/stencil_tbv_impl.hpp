// heat3d-mi355x — the tv sweep kernel (K-step sweeps with a conductivity
// field) in its three wall forms and its launcher, shared by stencil_tbv.hip
// (the forms without walls, and the dispatch of every form),
// stencil_tbv_wall.hip (insulated walls) and stencil_tbv_conv.hip (convective
// walls).  The kernel is described in stencil_tbv.hip, its wall forms in
// stencil_tbv_kernel.inc.
#pragma once

#include "stencil_tbl_impl.hpp"

namespace heat3d {
namespace hip {

namespace {

// Ch ring: 6 slots for every depth (lcm(3, 6, 2) = 6 keeps the unroll that makes
// the ring indices static short; a slot no stage reads costs no register), and
// how many planes ahead of step x the ring is loaded
constexpr int kTbvRing = 6;
constexpr int tbv_ahead(int K) { return K <= 3 ? 2 : 1; }

}  // namespace

// Textual inclusion, as the lean kernel's forms: the kernels without walls keep
// the code and the names they had before the wall forms existed.
#define H3D_TBV_CAP 0
#define H3D_TBV_NAME stencil_tbv
#define H3D_TBV_WALL 0
#include "stencil_tbv_kernel.inc"
#undef H3D_TBV_NAME
#undef H3D_TBV_WALL
#define H3D_TBV_NAME stencil_tbv_wall
#define H3D_TBV_WALL 1
#include "stencil_tbv_kernel.inc"
#undef H3D_TBV_NAME
#undef H3D_TBV_WALL
#define H3D_TBV_NAME stencil_tbv_conv
#define H3D_TBV_WALL 2
#include "stencil_tbv_kernel.inc"
#undef H3D_TBV_NAME
#undef H3D_TBV_WALL
#undef H3D_TBV_CAP
// ... and the tc kernels: the same three forms with a heat capacity
// (H3D_TBV_CAP 1), instantiated in stencil_tbc.hip, stencil_tbc_wall.hip and
// stencil_tbc_conv.hip
#define H3D_TBV_CAP 1
#define H3D_TBV_NAME stencil_tbc
#define H3D_TBV_WALL 0
#include "stencil_tbv_kernel.inc"
#undef H3D_TBV_NAME
#undef H3D_TBV_WALL
#define H3D_TBV_NAME stencil_tbc_wall
#define H3D_TBV_WALL 1
#include "stencil_tbv_kernel.inc"
#undef H3D_TBV_NAME
#undef H3D_TBV_WALL
#define H3D_TBV_NAME stencil_tbc_conv
#define H3D_TBV_WALL 2
#include "stencil_tbv_kernel.inc"
#undef H3D_TBV_NAME
#undef H3D_TBV_WALL
#undef H3D_TBV_CAP

// the kernel of wall form WALL, CAP: its heat-capacity form (only the form that
// is asked for gets instantiated)
template <typename Real, int R, int WY, int K, bool SRC, int WALL, bool CAP>
constexpr auto tbv_kernel() {
  if constexpr (CAP) {
    if constexpr (WALL == 2) return &stencil_tbc_conv<Real, R, WY, K, SRC>;
    else if constexpr (WALL == 1) return &stencil_tbc_wall<Real, R, WY, K, SRC>;
    else return &stencil_tbc<Real, R, WY, K, SRC>;
  } else {
    if constexpr (WALL == 2) return &stencil_tbv_conv<Real, R, WY, K, SRC>;
    else if constexpr (WALL == 1) return &stencil_tbv_wall<Real, R, WY, K, SRC>;
    else return &stencil_tbv<Real, R, WY, K, SRC>;
  }
}

// WALL: 0 no walls, 1 the insulated-wall form (p.wall), 2 the convective-wall
// form (p.wall_beta, p.ambient as well), as StencilParams::form() names them.
// CAP: the tc kernels (p.cap as well; the callers have checked that it is set).
template <typename Real, int R, int WY, int K, bool SRC, int WALL = 0, bool CAP = false>
static void launch_tbv(const StencilParams& p, const KernelSpec& ks, hipStream_t s) {
  constexpr auto kernel = tbv_kernel<Real, R, WY, K, SRC, WALL, CAP>();
  const void* kfn = reinterpret_cast<const void*>(kernel);
  const SweepForm form = p.form();
  HEAT3D_CHECK(SRC == form.src, "tv: source form mismatch");
  HEAT3D_CHECK(WALL == (int)form.wall, "tv: wall form mismatch");
  HEAT3D_CHECK(CAP == (p.cap != nullptr) && p.cond, "tv: conductivity / capacity form mismatch");
  const Box& b = p.box;
  const Layout& L = p.L;
  constexpr int TY = WY * R;
  HEAT3D_CHECK(L.n[0] + 2 * L.gx < (1LL << 30) && L.n[1] + 2 * L.gy < (1LL << 30) &&
                   L.sy * (int64_t)sizeof(Real) * (R + 2 + 2 * L.gy + TY + 2 * K) < (1LL << 31),
               "tv: extents exceed 32-bit tile coordinates");
  TBLArgs g{};
  g.sx = L.sx;
  g.sy = L.sy;
  g.origin = L.origin;
  for (int a = 0; a < 3; ++a) {
    g.blo[a] = (int)b.lo[a];
    g.bhi[a] = (int)b.hi[a];
  }
  const bool wx = p.ux[1] >= p.ux[0], wy = p.uy[1] >= p.uy[0], wz = p.uz[1] >= p.uz[0];
  g.ulo = (int)(wx ? p.ux[0] : b.lo[0]);
  g.uhi = (int)(wx ? p.ux[1] : b.hi[0]);
  g.uylo = (int)(wy ? p.uy[0] : b.lo[1]);
  g.uyhi = (int)(wy ? p.uy[1] : b.hi[1]);
  g.uzlo = (int)(wz ? p.uz[0] : b.lo[2]);
  g.uzhi = (int)(wz ? p.uz[1] : b.hi[2]);
  g.xlo_live = (int)-L.gx;
  g.xhi_live = (int)(L.n[0] + L.gx - 1);
  g.ylo_live = (int)-L.gy;
  g.yhi_live = (int)(L.n[1] + L.gy - 1);
  // every loaded column of every tile lies inside the row's allocation (as the
  // lean kernel: rows start zoff >= 16 elements before k = 0, the tail pad
  // covers the last tile's overhang); the store box is owned points
  HEAT3D_CHECK(b.lo[2] - K >= -L.zoff, "tv: tile columns before the row start");
  for (int a = 0; a < 3; ++a)
    HEAT3D_CHECK(b.lo[a] >= 0 && b.hi[a] <= L.n[a], "tv: box " << b.str() << " outside the owned extents");
  HEAT3D_CHECK(g.uylo - 1 >= -L.gy && g.uyhi <= L.n[1] + L.gy && g.uylo <= b.lo[1] && g.uyhi >= b.hi[1] &&
                   g.uzlo - 1 >= -L.gz && g.uzhi <= L.n[2] + L.gz && g.uzlo <= b.lo[2] && g.uzhi >= b.hi[2],
               "tv: y/z update range outside the ghosted layout");
  HEAT3D_CHECK(g.ulo - 1 >= g.xlo_live && g.uhi <= g.xhi_live + 1 && g.ulo <= b.lo[0] && g.uhi >= b.hi[0],
               "tv: u range [" << g.ulo << "," << g.uhi << ") outside the ghosted layout");
  constexpr int YS = TY - 2 * K;
  constexpr int U = lcm_l(lcm_l(kTbvRing, 3), 2);  // the kernel's unroll
  static const int slots = device_slots(kfn, 64 * WY);
  const int ZS = ks.ZS > 0 ? ks.ZS : 64 - 2 * K;
  HEAT3D_CHECK(ZS >= 1 && ZS <= 64 - 2 * K, "tv: z stride " << ZS << " outside [1, " << 64 - 2 * K << "]");
  g.c00 = (int)(b.lo[2] - K);
  g.r00 = (int)(b.lo[1] - K);
  g.nyb = (int)std::max<int64_t>(1, (b.extent(1) + YS - 1) / YS);
  g.zs = ZS;
  g.nzb = (int)std::max<int64_t>(1, (b.extent(2) + ZS - 1) / ZS);
  const int64_t tiles = (int64_t)g.nzb * g.nyb;
  const int64_t nxb = b.extent(0);
  HEAT3D_CHECK(!p.state || p.slot + K <= kResidualSlots, "tv: residual slots " << p.slot << "+" << K);
  auto scratch = [](const void* f) {
    hipFuncAttributes a{};
    return hipFuncGetAttributes(&a, f) == hipSuccess ? (int)a.localSizeBytes : 0;
  };
  static const int spill = scratch(kfn);
  HEAT3D_CHECK(spill == 0, "tv variant " << ks.str() << " spills " << spill << " B of registers per lane");
  unsigned long long* r = p.state && p.residual ? &p.state->residual[p.slot] : nullptr;
  const int* done = p.state ? &p.state->done : nullptr;
  const XPlan xp = ks.L > 0 ? fixed_xplan(nxb, tiles, ks.L) : plan_x(nxb, tiles, slots, 2 * (K - 1), U, ks.L == -1);
  HEAT3D_CHECK(xp.seg >= 1 && xp.seg < (1 << 15) && xp.split < (1 << 15) && xp.r < (1 << 30), "tv: x plan out of range");
  g.segsplit = xp.seg | (xp.split << 16);
  g.n1 = xp.n1;
  g.rb = xp.r | (xp.nb2 > 0 ? (1 << 30) : 0);
  const int64_t nblocks = (int64_t)xp.n1 + xp.r + xp.nb2;
  HEAT3D_CHECK(nblocks < (1LL << 31) && nblocks >= 1, "tv: bad block count " << nblocks);
  if (trace_enabled())
    std::fprintf(stderr, "[heat3d trace] tv K=%d box x %lld: zs=%d seg=%d tiles=%dx%d blocks=%lld\n", K, (long long)nxb,
                 ZS, xp.seg, g.nzb, g.nyb, (long long)nblocks);
  const Real* in = static_cast<const Real*>(p.in);
  Real* out = static_cast<Real*>(p.out);
  const Real* ch = static_cast<const Real*>(p.cond);
  const Real* src = static_cast<const Real*>(p.src);
  const Real Dx = (Real)p.D[0], Dy = (Real)p.D[1], Dz = (Real)p.D[2];
  const dim3 grid((unsigned)nblocks), block(64 * WY);
  // (the wall forms' arguments sit between g and Dx; the tc kernels take s after the source)
  auto launch = [&](auto... wall_args) {
    if constexpr (CAP) {
      const Real* cap = static_cast<const Real*>(p.cap);
      hipLaunchKernelGGL(kernel, grid, block, 0, s, in, out, ch, src, cap, g, wall_args..., Dx, Dy, Dz, r, done);
    } else {
      hipLaunchKernelGGL(kernel, grid, block, 0, s, in, out, ch, src, g, wall_args..., Dx, Dy, Dz, r, done);
    }
  };
  if constexpr (WALL == 0) {
    launch();
  } else {
    // the walls in the kernel's frame (as launch_tbl; the tv kernels have no swapped form)
    TBLWalls wl{};
    auto coord = [](int64_t v, int side) {
      const int none = side ? kWallNoneHi : kWallNoneLo;
      return v == kNoWall || v <= kWallNoneLo || v >= kWallNoneHi ? none : (int)v;
    };
    for (int e = 0; e < 2; ++e) {
      wl.x[e] = coord(p.wall[0][e], e);
      wl.y[e] = coord(p.wall[1][e], e);
      wl.z[e] = coord(p.wall[2][e], e);
    }
    if constexpr (WALL == 1) {
      launch(wl);
    } else {
      // ... and the convective coefficients (an insulated face: 0)
      TBLConv<Real> cv{};
      auto beta = [&](int a, int e) {
        return (Real)(p.wall[a][e] != kNoWall && p.wall_beta[a][e] > 0 ? p.wall_beta[a][e] : 0);
      };
      for (int e = 0; e < 2; ++e) {
        cv.x[e] = beta(0, e);
        cv.y[e] = beta(1, e);
        cv.z[e] = beta(2, e);
      }
      cv.tinf = (Real)p.ambient;
      launch(wl, cv);
    }
  }
  HIPK_CHECK(hipGetLastError());
}

// The wall forms' dispatch, one per translation unit (stencil_tbv_wall.hip,
// stencil_tbv_conv.hip): launches *p (its form: form.src and the unit's wall
// kind) with the shape of depth k.K, or (p == nullptr) only reports whether
// that form is built; *shape, if given, receives the tile.
bool tbv_wall_dispatch(DType t, bool src, const StencilParams* p, const KernelSpec& k, hipStream_t s, LeanShape* shape);
bool tbv_conv_dispatch(DType t, bool src, const StencilParams* p, const KernelSpec& k, hipStream_t s, LeanShape* shape);

// One line of a wall unit's shape list: the form (source or not) of depth KK
// runs as RR rows x YY waves.  A form without a line is not built.
#define H3D_TBV_WALL_SHAPE(WALL, SRCB, KK, RR, YY)               \
  if (k.K == KK && src == SRCB) {                                \
    if (shape) *shape = LeanShape{RR, YY, false};                \
    if (p) launch_tbv<Real, RR, YY, KK, SRCB, WALL>(*p, k, s);   \
    return true;                                                 \
  }

// The tc kernels' dispatch, one per translation unit (stencil_tbc.hip: no
// walls, stencil_tbc_wall.hip, stencil_tbc_conv.hip), as the wall forms' above.
bool tbc_plain_dispatch(DType t, bool src, const StencilParams* p, const KernelSpec& k, hipStream_t s, LeanShape* shape);
bool tbc_wall_dispatch(DType t, bool src, const StencilParams* p, const KernelSpec& k, hipStream_t s, LeanShape* shape);
bool tbc_conv_dispatch(DType t, bool src, const StencilParams* p, const KernelSpec& k, hipStream_t s, LeanShape* shape);

// One line of a tc unit's shape list (as H3D_TBV_WALL_SHAPE)
#define H3D_TBC_SHAPE(WALL, SRCB, KK, RR, YY)                          \
  if (k.K == KK && src == SRCB) {                                      \
    if (shape) *shape = LeanShape{RR, YY, false};                      \
    if (p) launch_tbv<Real, RR, YY, KK, SRCB, WALL, true>(*p, k, s);   \
    return true;                                                       \
  }

}  // namespace hip
}  // namespace heat3d
