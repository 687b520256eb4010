// heat3d-mi355x — the lean K-step sweep kernel and its launcher (shared by
// stencil_tbl.hip, which dispatches, and the stencil_tbl_part*.hip units, which
// instantiate the variants listed in stencil_tbl_variants.inc in parallel).
#pragma once

// heat3d-mi355x — K-step temporally blocked FTCS kernel, lean form ("tl").
//
// Same contract as stencil_tbr.hip (one HBM sweep turns T^n into T^{n+K};
// every point goes through the reference update heat3D.cu:128-131 with the
// arithmetic of kernels.hpp ftcs_update, so fields and all K residuals are
// bitwise identical to K single steps), re-planned after the ISA and
// counters of the ring kernel on MI355X: ~40% of its VALU stream per point
// update was overhead (SGPR spill reloads through v_readlane, read-lanes of
// separately loaded halo columns, per-point validity selects), which is what
// kept a 4-step variant from fitting 16 waves x 128 VGPRs.  Here
//
//   * halos are ordinary lanes and rows: a tile loads 64 consecutive columns
//     (one wave wide) and WY*R rows; stage s output is valid on lanes
//     [s+1, 63-s) and tile rows [s+1, TY-s-1); T^{n+K} is stored on
//     lanes [K, 64-K) x rows [K, TY-K).  z neighbours are zero-filling DPP
//     shifts (no "old" operand, no read-lanes, no halo registers); the tile's
//     outer rows take a wave's own edge row from LDS as a stand-in (finite,
//     outside every stored / counted point);
//   * residuals accumulate per lane without masks; the per-lane validity of
//     stage s (cone, update range, box widened by K-1-s) is applied once, at
//     the end;
//   * a wave whose rows are inside the box, the update range and the tile's
//     cone runs a mask-free step ("fast"): 9 fp64 ops for the update, 2 for
//     the residual, 4 DPP moves.  Steps of the pipeline fill / drain, tiles on
//     a Dirichlet face and waves on the tile's edge run the masked step (the
//     same code with uniform x / y conditions and a per-lane z mask); the
//     choice is a uniform branch per step, both forms hold one barrier;
//   * a third form, the edge role (template parameter EW > 0, spec field 9):
//     waves 0 and WY - 1 hold the tile's K halo rows, of which stage s is
//     valid on tile rows [s + 1, TY - s - 1) only, so halo row j needs j of
//     the K stages (6 of a 4 x 4 wave's 16 row-stages at K = 4).  Under the
//     role those waves run a loop of their own whose step evaluates, per row,
//     the stages inside that cone and nothing else, by static indices, so the
//     stage rings outside the cone are never allocated; the registers and
//     issue slots that frees carry E = EW - 1 owned rows per edge wave
//     (TY = WY*R + 2E rows, TY - 2K stored: 52 / 44 at E = 2 against 48 / 40).
//     The step is mask-free where every row of the wave is inside the box and
//     the update range; on Dirichlet faces and in fill / drain it is the
//     masked step restricted to the same cone.  An edge wave publishes the
//     one LDS row its neighbour reads and holds the same barrier.  The three
//     roles branch once per wave, never per step, which keeps each loop's
//     live registers its own.  The edge-role kernels also have a z-masked
//     step (StepForm below: the mask-free step with the stage outputs selected
//     by the lane's z condition) for the y-free waves of a tile that has
//     columns outside the z update range, skip the stages of the masked step
//     that the pipeline fill of a piece has not reached, and leave the padded
//     steps after a piece's last plane unrun;
//   * loads are an SGPR row base plus one lane offset (global_load saddr
//     form), clamped rows / planes fold into the SGPR base.
//
// Tiles advance along z by 64 - 2K columns and along y by WY*R - 2K rows;
// workgroups march along x segments (XPlan, as the ring kernel), dispatched
// XCD-aware.  y rows of each stage's centre plane go through LDS once per
// step (double-buffered by step parity: one barrier per step).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <map>
#include <mutex>
#include <cstdlib>
#include <tuple>
#include <type_traits>

#include "hip_helpers.hpp"

namespace heat3d {
namespace hip {

struct TBLArgs {
  int64_t sx, sy, origin;      // plane / row strides, element index of owned (0,0,0)
  int blo[3], bhi[3];          // store box
  int ulo, uhi, uylo, uyhi;    // update ranges (x, y)
  int uzlo, uzhi;              // update range (z)
  int xlo_live, xhi_live;      // x planes present in memory
  int ylo_live, yhi_live;      // y rows present in memory
  int c00, r00;                // first loaded column / row of tile (0, 0)
  int nzb, nyb;
  int segsplit, n1, rb;        // x plan: seg | split << 16, whole pieces, r | split-tail << 30
  int zs;                      // tile stride along z = stored columns per tile (<= 64 - 2K)
  DeviceState* fst;            // fused convergence check (fused_check_tail): state, nullptr = off
  int fslot, fblocks;          // its first residual slot and the grid's workgroup count
};

// Insulated walls in the kernel's frame (x the marching axis, y the tile rows,
// z the lanes): the coordinate of the wall-adjacent plane / row / column, or
// a sentinel no coordinate reaches (kWallNoneLo below everything on the low
// side, kWallNoneHi above everything on the high side)
struct TBLWalls {
  int x[2], y[2], z[2];
};
constexpr int kWallNoneLo = -(1 << 30), kWallNoneHi = 1 << 30;
// Convective walls: the coefficient of each face in the same frame (0: an
// insulated face, or none) and the ambient temperature, in the field's dtype
template <typename Real>
struct TBLConv {
  Real x[2], y[2], z[2];
  Real tinf;
};

namespace {

constexpr int gcd_l(int a, int b) { return b == 0 ? a : gcd_l(b, a % b); }
constexpr int lcm_l(int a, int b) { return a / gcd_l(a, b) * b; }

__device__ __forceinline__ int sgpr(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Raw buffer resource over one x plane (SGPRs: 48-bit base, no range limit;
// dword 3 = the gfx9 untyped-buffer word).  A row load / store is then
// buffer_{load,store}_dwordx2 v, v_lane_bytes, s[rsrc], s_row_bytes offen:
// no per-lane 64-bit address registers, no address VALU.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t plane_rsrc(const void* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)0xffffffff, 0x00020000);
}
template <typename Real>
__device__ __forceinline__ Real buf_load(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
  if constexpr (sizeof(Real) == 8)
    return __builtin_bit_cast(Real, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
  else
    return __builtin_bit_cast(Real, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
// AUX = cache policy bits of the store (2 = nt: streaming, not kept in L2)
template <typename Real, int AUX = 0>
__device__ __forceinline__ void buf_store(Real v, __amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
  if constexpr (sizeof(Real) == 8)
    __builtin_amdgcn_raw_buffer_store_b64(
        __builtin_bit_cast(unsigned __attribute__((ext_vector_type(2))), v), r, voff, soff, AUX);
  else
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, voff, soff, AUX);
}

// The form of one plane step of the lean kernel (stencil_tbl_kernel.inc step()):
// kStepMasked evaluates every x / y / z condition; kStepFree none (a wave whose
// rows, columns and stage planes are all updated, counted and stored);
// kStepZ (edge-role kernels) the z conditions only: a wave and plane step that
// would be mask-free in a tile that has columns outside the z update range.
enum StepForm : int { kStepMasked = 0, kStepFree = 1, kStepZ = 2 };
template <int F>
using step_form = std::integral_constant<int, F>;

// f(integral_constant<int, I>) for I = B .. E-1, unrolled at compile time
template <int B, int E, typename Fn>
__device__ __forceinline__ void static_for(Fn&& fn) {
  if constexpr (B < E) {
    fn(std::integral_constant<int, B>{});
    static_for<B + 1, E>(fn);
  }
}

}  // namespace

// NTS: store cache policy; SW: swapped axes (x planes are the tile rows, the
// kernel marches y): the row neighbours are the x terms of the update.
//
// SRC: heat source (kernels.hpp ftcs_update_src).  Stage s at step x adds S of
// plane x - s to its update before the residual and the masked select, so
// points outside the update ranges never see S.  The source rows are addressed
// like the field's: a buffer resource per (clamped) plane, the same roff[] /
// lane_b offsets.  Of the two ways to hold S, a K-plane register ring (K R
// values per lane, one load per plane) and re-loading plane x - s at stage s
// (R values per lane in flight, K loads per plane of which K - 1 hit in L2),
// this kernel re-loads: the fp64 K = 3 default shape uses 112 of the 128 VGPRs
// its 16 waves may have; a ring of 9 doubles per lane plus the 3 of the plane
// in flight is 24 VGPRs more, over the budget, where the re-load form stays
// inside it without scratch, as every source variant does for its workgroup
// size (register report in profiles/source_term.md; measured cost at 1022^3
// fp64 K = 3: 7.37 against 3.55 ms per sweep, well above the 1.42x traffic
// model — the in-order memory counter makes a stage's wait for its source
// rows also wait for the T^n prefetch issued before them).  The source forms are
// kernels of their own (stencil_tbl_src, the same definition included with
// H3D_TBL_SRC 1), so the kernels without a source keep their code, names and
// tuned schedules.
#define H3D_TBL_NAME stencil_tbl
#define H3D_TBL_SRC 0
#define H3D_TBL_WALL 0
#include "stencil_tbl_kernel.inc"
#undef H3D_TBL_NAME
#undef H3D_TBL_SRC
#define H3D_TBL_NAME stencil_tbl_src
#define H3D_TBL_SRC 1
#include "stencil_tbl_kernel.inc"
#undef H3D_TBL_NAME
#undef H3D_TBL_SRC
#undef H3D_TBL_WALL
// WALL: insulated (zero-flux) walls (kernels.hpp StencilParams::wall).  At an
// updated point next to an insulated wall the neighbour across it is replaced
// by the centre value before the update, at every stage: a deep mirrored ghost
// would not do, because fma(-2, c, xp) + xm is not symmetric in xm and xp and
// mirrored points would differ in the last bit from single steps.  The
// substitution lives in the masked step only: per stage a uniform compare of
// its plane for the marching axis, two bits per row in an SGPR for the rows, a
// lane mask for z (constant over the piece).  Waves, tiles and plane steps
// that hold a wall-adjacent row, column or plane are kept off the mask-free
// step (wfast, zfast, xf_lo / xf_hi), which is therefore the code of the
// uniform kernel; no register row is added.  A kernel of its own
// (stencil_tbl_wall, instantiated in stencil_tbl_wall.hip), so the kernels
// without walls keep their code, names and tuned schedules.
#define H3D_TBL_NAME stencil_tbl_wall
#define H3D_TBL_SRC 0
#define H3D_TBL_WALL 1
#include "stencil_tbl_kernel.inc"
#undef H3D_TBL_NAME
#undef H3D_TBL_SRC
#undef H3D_TBL_WALL
// WALL 2: convective (Robin) walls (kernels.hpp StencilParams::wall_beta).  The
// wall form's masked step with one more term: the neighbour across a wall is
// the ghost fma(beta, T_inf - c, c) of that face, T_inf - c formed once per
// row; beta = 0 (an insulated face of the same run) gives c.  The six
// coefficients and the ambient arrive by value (TBLConv, uniform: SGPRs).  The
// classification that keeps wall-adjacent waves, tiles and plane steps off the
// mask-free step is the wall form's, unchanged.  A kernel of its own again
// (stencil_tbl_conv, instantiated in stencil_tbl_conv.hip): insulated-only runs
// keep stencil_tbl_wall.
#define H3D_TBL_NAME stencil_tbl_conv
#define H3D_TBL_SRC 0
#define H3D_TBL_WALL 2
#include "stencil_tbl_kernel.inc"
#undef H3D_TBL_NAME
#undef H3D_TBL_SRC
#undef H3D_TBL_WALL
// SRC with WALL 1 / 2: an internally heated body behind insulated or convective
// walls.  The wall form's masked step with the source form's re-loaded source
// rows (the same clamped plane and roff[] offsets): the ghost substitution first,
// then the update, then the source, which is the order of the single-step path
// (wall planes refreshed, then ftcs_update_src).  The mask-free step is the
// source form's.  Kernels of their own once more (stencil_tbl_wall_src and
// stencil_tbl_conv_src, instantiated in stencil_tbl_wall_src.hip and
// stencil_tbl_conv_src.hip), so the six kernels above keep their code; the
// shapes that fit the register budget are in profiles/wall_source_sweeps.md.
#define H3D_TBL_NAME stencil_tbl_wall_src
#define H3D_TBL_SRC 1
#define H3D_TBL_WALL 1
#include "stencil_tbl_kernel.inc"
#undef H3D_TBL_NAME
#undef H3D_TBL_SRC
#undef H3D_TBL_WALL
#define H3D_TBL_NAME stencil_tbl_conv_src
#define H3D_TBL_SRC 1
#define H3D_TBL_WALL 2
#include "stencil_tbl_kernel.inc"
#undef H3D_TBL_NAME
#undef H3D_TBL_SRC
#undef H3D_TBL_WALL

// The kernel of form (SRC, WALL), one of the six inclusions above, and the
// name its timed schedules are stored under.  (if constexpr: only the form that
// is asked for gets instantiated.)
template <typename Real, int R, int WY, int K, int Q, int NTS, bool SW, bool SRC, int EW, int WALL>
constexpr auto tbl_kernel() {
  if constexpr (SRC && WALL == 2) return &stencil_tbl_conv_src<Real, R, WY, K, Q, NTS, SW>;
  else if constexpr (SRC && WALL == 1) return &stencil_tbl_wall_src<Real, R, WY, K, Q, NTS, SW>;
  else if constexpr (SRC) return &stencil_tbl_src<Real, R, WY, K, Q, NTS, SW>;
  else if constexpr (WALL == 2) return &stencil_tbl_conv<Real, R, WY, K, Q, NTS, SW>;
  else if constexpr (WALL == 1) return &stencil_tbl_wall<Real, R, WY, K, Q, NTS, SW>;
  else return &stencil_tbl<Real, R, WY, K, Q, NTS, SW, EW>;
}
template <typename Real, bool SRC, int WALL>
constexpr const char* tbl_tuning_name() {
  constexpr bool f64 = sizeof(Real) == 8;
  if constexpr (SRC && WALL == 2) return f64 ? "tl-fp64-conv-src" : "tl-fp32-conv-src";
  else if constexpr (SRC && WALL == 1) return f64 ? "tl-fp64-wall-src" : "tl-fp32-wall-src";
  else if constexpr (SRC) return f64 ? "tl-fp64-src" : "tl-fp32-src";
  else if constexpr (WALL == 2) return f64 ? "tl-fp64-conv" : "tl-fp32-conv";
  else if constexpr (WALL == 1) return f64 ? "tl-fp64-wall" : "tl-fp32-wall";
  else return f64 ? "tl-fp64" : "tl-fp32";
}

// EW: the edge role of waves 0 and WY - 1 (0 = off, else 1 + their owned rows)
// WALL: 1 the insulated-wall form (p.wall; no edge role), 2 the convective-wall
// form (p.wall_beta, p.ambient as well); either with SRC: their source forms
template <typename Real, int R, int WY, int K, int Q, int NTS = 0, bool SW = false, bool SRC = false, int EW = 0,
          int WALL = 0>
void launch_tbl(const StencilParams& p, const KernelSpec& ks, hipStream_t s) {
  constexpr bool swap_xy = SW;
  constexpr auto kernel = tbl_kernel<Real, R, WY, K, Q, NTS, SW, SRC, EW, WALL>();
  const void* kfn = reinterpret_cast<const void*>(kernel);
  static_assert(EW == 0 || !SRC, "the edge role has no source form");
  static_assert(!WALL || EW == 0, "the wall form has no edge role");
  const SweepForm form = p.form();
  HEAT3D_CHECK(SRC == form.src, "tl: source form mismatch");
  HEAT3D_CHECK(WALL == (int)form.wall, "tl: wall form mismatch");
  Box b = p.box;
  constexpr int TY = WY * R + 2 * (EW > 0 ? EW - 1 : 0);  // as the kernel's
  // swap_xy: march along y with x as the tile rows (thin x slabs: a tile of
  // WY*R x-rows covers the slab and its K-deep halos, workgroups march the
  // long y extent).  The kernel is axis-agnostic through its strides and
  // ranges, so the swap is a relabelling of the arguments.
  const Layout& L = p.L;
  const int64_t Lsx = swap_xy ? L.sy : L.sx, Lsy = swap_xy ? L.sx : L.sy;
  const int64_t Ln0 = swap_xy ? L.n[1] : L.n[0], Ln1 = swap_xy ? L.n[0] : L.n[1];
  const int64_t Lg0 = swap_xy ? L.gy : L.gx, Lg1 = swap_xy ? L.gx : L.gy;
  const int64_t(&pux)[2] = swap_xy ? p.uy : p.ux;
  const int64_t(&puy)[2] = swap_xy ? p.ux : p.uy;
  if (swap_xy) {
    std::swap(b.lo[0], b.lo[1]);
    std::swap(b.hi[0], b.hi[1]);
  }
  HEAT3D_CHECK(Ln0 + 2 * Lg0 < (1LL << 30) && Ln1 + 2 * Lg1 < (1LL << 30) &&
                   Lsy * (int64_t)sizeof(Real) * (R + EW + 2 * Lg1 + TY + 2 * K) < (1LL << 31),
               "tl: extents exceed 32-bit tile coordinates");
  TBLArgs g{};
  g.sx = Lsx;
  g.sy = Lsy;
  g.origin = L.origin;
  for (int a = 0; a < 3; ++a) {
    g.blo[a] = (int)b.lo[a];
    g.bhi[a] = (int)b.hi[a];
  }
  g.ulo = (int)(pux[1] >= pux[0] ? pux[0] : b.lo[0]);
  g.uhi = (int)(pux[1] >= pux[0] ? pux[1] : b.hi[0]);
  const bool wy = puy[1] >= puy[0], wz = p.uz[1] >= p.uz[0];
  g.uylo = (int)(wy ? puy[0] : b.lo[1]);
  g.uyhi = (int)(wy ? puy[1] : b.hi[1]);
  g.uzlo = (int)(wz ? p.uz[0] : b.lo[2]);
  g.uzhi = (int)(wz ? p.uz[1] : b.hi[2]);
  g.xlo_live = (int)-Lg0;
  g.xhi_live = (int)(Ln0 + Lg0 - 1);
  g.ylo_live = (int)-Lg1;
  g.yhi_live = (int)(Ln1 + Lg1 - 1);
  // every loaded column of every tile lies inside the row's allocation: the
  // row starts zoff >= 16 elements before k = 0 (tiles start K <= 6 columns
  // before the box) and the tail pad covers the last tile's overhang
  HEAT3D_CHECK(b.lo[2] - K >= -L.zoff, "tl: tile columns before the row start");
  HEAT3D_CHECK(g.uylo - 1 >= -Lg1 && g.uyhi <= Ln1 + Lg1 && g.uylo <= b.lo[1] && g.uyhi >= b.hi[1] &&
                   g.uzlo - 1 >= -L.gz && g.uzhi <= L.n[2] + L.gz && g.uzlo <= b.lo[2] && g.uzhi >= b.hi[2],
               "tl: y/z update range outside the ghosted layout");
  HEAT3D_CHECK(g.ulo - 1 >= g.xlo_live && g.uhi <= g.xhi_live + 1 && g.ulo <= b.lo[0] && g.uhi >= b.hi[0],
               "tl: u range [" << g.ulo << "," << g.uhi << ") outside the ghosted layout");
  // the walls in the kernel's frame (swap_xy relabels x and y as it does the box)
  TBLWalls wl{};
  {
    auto coord = [](int64_t v, int side) {
      const int none = side ? kWallNoneHi : kWallNoneLo;
      return v == kNoWall || v <= kWallNoneLo || v >= kWallNoneHi ? none : (int)v;
    };
    const int ax = swap_xy ? 1 : 0, ay = swap_xy ? 0 : 1;
    for (int e = 0; e < 2; ++e) {
      wl.x[e] = coord(p.wall[ax][e], e);
      wl.y[e] = coord(p.wall[ay][e], e);
      wl.z[e] = coord(p.wall[2][e], e);
    }
  }
  // ... and the convective coefficients (an insulated face: 0)
  TBLConv<Real> cv{};
  {
    auto beta = [&](int a, int e) { return (Real)(p.wall[a][e] != kNoWall && p.wall_beta[a][e] > 0 ? p.wall_beta[a][e] : 0); };
    const int ax = swap_xy ? 1 : 0, ay = swap_xy ? 0 : 1;
    for (int e = 0; e < 2; ++e) {
      cv.x[e] = beta(ax, e);
      cv.y[e] = beta(ay, e);
      cv.z[e] = beta(2, e);
    }
    cv.tinf = (Real)p.ambient;
  }
  constexpr int YS = TY - 2 * K;
  static const int slots = device_slots(kfn, 64 * WY);  // magic static: thread-safe under --gpus N
  constexpr int U = Q == 4 ? 12 : 6;  // the kernel's unroll (lcm(Q, 3, 2))
  const int ZS = ks.ZS > 0 ? ks.ZS
                           : lean_z_stride(b.extent(0), b.extent(1), b.extent(2), K, (int)sizeof(Real), TY, slots, U, ks.L);
  HEAT3D_CHECK(ZS >= 1 && ZS <= 64 - 2 * K, "tl: z stride " << ZS << " outside [1, " << 64 - 2 * K << "]");
  g.c00 = (int)(b.lo[2] - K);
  g.r00 = (int)(b.lo[1] - K);
  g.nyb = (int)std::max<int64_t>(1, (b.extent(1) + YS - 1) / YS);
  auto set_zs = [&](TBLArgs& ga, int zs) {
    ga.zs = zs;
    ga.nzb = (int)std::max<int64_t>(1, (b.extent(2) + zs - 1) / zs);
    return (int64_t)ga.nzb * ga.nyb;
  };
  (void)set_zs(g, ZS);
  const int64_t nxb = b.extent(0);
  HEAT3D_CHECK(ks.L != -2, "tl: the persistent walk (L = -2) was retired in round 5 (18-22% slower than the x plan)");
  HEAT3D_CHECK(!p.state || p.slot + K <= kResidualSlots, "tl: residual slots " << p.slot << "+" << K);
  auto scratch = [](const void* f) {
    hipFuncAttributes a{};
    return hipFuncGetAttributes(&a, f) == hipSuccess ? (int)a.localSizeBytes : 0;
  };
  static const int spill = scratch(kfn);
  // a spilling variant is refused (one was miscompiled on ROCm 7.2)
  HEAT3D_CHECK(spill == 0, "tl variant " << ks.str() << " spills " << spill << " B of registers per lane");
  unsigned long long* r = p.state && p.residual ? &p.state->residual[p.slot] : nullptr;
  const int* done = p.state ? &p.state->done : nullptr;
  // spec field L: > 0 fixed segments, -1 equal segments, -3 the x plan;
  // 0: the schedule timed for this box (tune_schedule: z stride and x
  // schedule), else the x plan
  auto fire = [&](int zs, int Lx) {
    TBLArgs ga = g;
    const int64_t tiles = set_zs(ga, zs);
    const XPlan xp = Lx > 0 ? fixed_xplan(nxb, tiles, Lx) : plan_x(nxb, tiles, slots, 2 * (K - 1), U, Lx == -1);
    HEAT3D_CHECK(xp.seg < (1 << 15) && xp.split < (1 << 15) && xp.r < (1 << 30), "tl: x plan out of range");
    ga.segsplit = xp.seg | (xp.split << 16);
    ga.n1 = xp.n1;
    ga.rb = xp.r | (xp.nb2 > 0 ? (1 << 30) : 0);
    const int64_t nblocks = (int64_t)xp.n1 + xp.r + xp.nb2;
    HEAT3D_CHECK(nblocks < (1LL << 31) && nblocks >= 1, "tl: bad block count " << nblocks);
    ga.fst = p.fuse_check && r ? p.state : nullptr;
    ga.fslot = p.slot;
    ga.fblocks = (int)nblocks;
    if (trace_enabled())
      std::fprintf(stderr, "[heat3d trace] tl K=%d box x %lld: zs=%d L=%d seg=%d tiles=%dx%d blocks=%lld (model %.1f)\n",
                   K, (long long)nxb, zs, Lx, xp.seg, ga.nzb, ga.nyb, (long long)nblocks,
                   xplan_makespan(xp, nxb, tiles, slots, 2 * (K - 1), U));
    // the kernels' arguments, in their order: in, out, [src,] ga, [wl, [cv,]] Dx, Dy, Dz, r, done
    const auto fields = [&] {
      const Real* in = static_cast<const Real*>(p.in);
      Real* out = static_cast<Real*>(p.out);
      if constexpr (SRC) return std::make_tuple(in, out, static_cast<const Real*>(p.src));
      else return std::make_tuple(in, out);
    }();
    const auto walls = [&] {
      if constexpr (WALL == 2) return std::make_tuple(wl, cv);
      else if constexpr (WALL == 1) return std::make_tuple(wl);
      else return std::make_tuple();
    }();
    std::apply(
        [&](const auto&... a) { hipLaunchKernelGGL(kernel, dim3((unsigned)nblocks), dim3(64 * WY), 0, s, a...); },
        std::tuple_cat(fields, std::make_tuple(ga), walls,
                       std::make_tuple((Real)p.D[0], (Real)p.D[1], (Real)p.D[2], r, done)));
    HIPK_CHECK(hipGetLastError());
  };
  if (ks.L == 0 && ks.ZS == 0 && !SW) {
    const int64_t box[3] = {b.extent(0), b.extent(1), b.extent(2)};
    if (p.tune) {
      // z strides: the model's, and the other of 64 - 2K / its 64-byte-aligned form
      std::vector<int> zs_opts{ZS};
      const int wide = 64 - 2 * K, aligned = sizeof(Real) == 8 ? wide & ~7 : wide;
      for (int z : {wide, aligned})
        if (std::find(zs_opts.begin(), zs_opts.end(), z) == zs_opts.end()) zs_opts.push_back(z);
      tune_schedule(tbl_tuning_name<Real, SRC, WALL>(), kfn, box, slots, p.cu_reserved, U, zs_opts, s, fire, g.nyb,
                    2 * (K - 1));
      return;  // every candidate computed this sweep
    }
    SchedChoice c;
    if (tuned_lookup(kfn, box, slots, p.cu_reserved, &c)) {
      fire(c.zs, c.L);
      return;
    }
    fire(ZS, 0);
    return;
  }
  fire(ZS, ks.L);
}

}  // namespace hip
}  // namespace heat3d
