// heat3d-mi355x — kernel launch API, implemented twice:
//   heat3d::hip::*  hand-written gfx950 kernels (kernels_hip.hip)
//   heat3d::cpu::*  OpenMP host kernels used by the CPU backend / oracle (kernels_cpu.cpp)
//
// Both evaluate the FTCS update through ftcs_update() below: the reference's
// per-cell expression (heat3D.cu:128-131) with the fused
// multiply-adds nvcc puts into the reference's GPU kernel, explicit, and no
// other contraction, so the GPU and CPU backends agree bit for bit.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../core/common.hpp"
#include "heat_balance.hpp"
#include "layout.hpp"
#include "steady_cg.hpp"

namespace heat3d {

struct KernelSpec {
  // Tile: the single-step kernel (kernels_hip.hip; single steps, rollback
  // recomputation, runs without temporal blocking).  Naive: one thread per
  // point, the simplest gfx950 form (a test oracle).  TBL: the K-step
  // temporally blocked lean kernel (stencil_tbl.hip; fp32 packed pairs in
  // stencil_tbp.hip), K time steps per HBM sweep.  The round-1/2 queue and
  // register-ring sweep kernels (tb2 / tbK / trK) were retired in round 3:
  // no default path used them (docs/PERFORMANCE.md keeps their numbers).
  // TBV: the K-step sweep with a conductivity field (stencil_tbv.hip; spec
  // tv2 / tv3), one shape per dtype and depth.  TBC: the tv sweep with a heat
  // capacity as well (stencil_tbc.hip; spec tc2 / tc3).
  enum Kind { Naive = 0, Tile = 2, TBL = 6, TBV = 7, TBC = 8 } kind = Tile;
  int K = 0;  // multi-step kinds: time steps per sweep
  int WZ = 0, WY = 0;  // waves per workgroup along z and y
  int V = 0;  // elements per lane along z (0 = default for dtype)
  int R = 0;  // rows per wave along y (0 = default)
  int L = 0;  // x-segment length per wave (0 = auto)
  int O = -1; // TBL: output-store cache-policy bits (2 = nt)
  int NT = 0; // TBL: T^n ring size
  int ZS = 0; // TBL: tile stride along z (stored columns per tile; 0 = chosen per box)
  int EW = 0; // TBL: edge role of a tile's two halo waves (0 = off, else 1 + the rows each also owns)
  bool multi_step() const { return kind == TBL || kind == TBV || kind == TBC; }
  static KernelSpec parse(const std::string& s);
  std::string str() const;
  // zero (default) fields replaced by the tuned defaults for dtype t
  // (profiles/kernel_sweep.md); the kernel dispatchers and kernel names use it
  KernelSpec resolved(DType t) const;
};

// StencilParams::wall: no insulated wall on this side
constexpr int64_t kNoWall = -(int64_t(1) << 40);

// Which form of the uniform update a call asks for: with a heat source or
// without, and behind which kind of wall (Convective as soon as one face is;
// the values are the lean kernels' WALL template argument).  Derived once, by
// StencilParams::form(); the CPU rows and the lean sweep's dispatch select by it.
enum class WallKind { None = 0, Insulated = 1, Convective = 2 };
struct SweepForm {
  bool src = false;
  WallKind wall = WallKind::None;
};

struct StencilParams {
  const void* in = nullptr;
  void* out = nullptr;
  Layout L;
  Box box;                  // local owned coordinates to update
  double D[3] = {0, 0, 0};  // Dx, Dy, Dz
  DeviceState* state = nullptr;
  int slot = 0;             // residual slot (multi-step kernels: first of K slots)
  // multi-step kernels only: x range [ux0, ux1) in which the intermediate
  // fields T^{n+s} are computed (beyond the box on faces with a deep
  // neighbour halo); outside it they stay T^n (Dirichlet ghosts).
  // ux1 < ux0 means "the box's x range".
  int64_t ux[2] = {0, -1};
  // same for y and z (block decompositions with deep y / z halos)
  int64_t uy[2] = {0, -1}, uz[2] = {0, -1};
  // CUs the launch stream's CU mask keeps free (persistent sweeps launch as
  // many workgroups as the remaining CUs hold)
  int cu_reserved = 0;
  // sweeps only: time the x-schedule candidates on this launch (a sweep is
  // idempotent: every candidate writes the same T^{n+K} to out) and keep the
  // fastest for this kernel and box shape (autotune_x_schedule)
  bool tune = false;
  // false: the kernel honours state->done (a no-op once converged) but
  // records no residual (Solver::preheat's idempotent warm-up sweeps)
  bool residual = true;
  // K-step sweeps of a single-subdomain run: the last workgroup to finish runs
  // the convergence check of the sweep's K residual slots (check_convergence
  // semantics, bitwise the same state) instead of a separate check kernel
  // after it, which cost ~10 us per sweep on the critical path (a one-lane
  // kernel and its dispatch; profiles/r06)
  bool fuse_check = false;
  // volumetric heat source S = dtype(dt * q): a field in the same Layout as
  // in/out (ghost shells included), added to every updated point
  // (ftcs_update_src).  nullptr: no source, the kernels without a source term.
  const void* src = nullptr;
  // relative conductivity, stored as Ch = dtype(0.5 * c) with 0 < c <= 1: a
  // static field in the same Layout (ghost shells included; a face weight
  // towards a ghost point reads Ch there).  Every updated point is evaluated
  // by ftcs_update_var.  nullptr: uniform material, the kernels above.  The
  // single-step kernels and the tv sweeps have a conductivity form (a tl sweep
  // with it is an error, as is a tv sweep without it).  Together with `wall`
  // below: cpu::stencil / stencil_multi and the wall forms of the tv sweep.
  const void* cond = nullptr;
  // Insulated (zero-flux) walls: wall[a][0] / wall[a][1] is the local
  // coordinate along axis a of the updated plane (row, column) next to the
  // insulated low / high wall of the global grid, kNoWall where that face is
  // Dirichlet or lies outside what this rank can reach.  At such a point the
  // neighbour across the wall is replaced by the centre value (the mirror
  // ghost; the flux through the face between them is exactly 0) and the update
  // is evaluated as ever.  Taken from global indices, so it also holds for
  // wall-adjacent points computed inside a neighbour's deep halo.  cpu::stencil
  // and cpu::stencil_multi honour it, also with a source and with a
  // conductivity (only the neighbour's temperature is replaced: the face
  // weights still read Ch at the wall vertex), as do the wall forms of the lean
  // sweep (stencil_tbl_wall.hip; with a source stencil_tbl_wall_src.hip) and of
  // the tv sweep (stencil_tbv_wall.hip); the single-step gfx950 kernels do not
  // take it (they run on wall planes copied from their inward neighbours,
  // which gives the same bits).
  int64_t wall[3][2] = {{kNoWall, kNoWall}, {kNoWall, kNoWall}, {kNoWall, kNoWall}};
  // Convective (Robin) walls, -k dT/dn = h (T - T_inf): a face with a wall
  // coordinate above and wall_beta[a][e] >= 0 is convective with that
  // coefficient (0 <= beta <= 1; negative: the face is insulated or has no
  // wall).  The neighbour across such a wall is replaced by
  // convective_ghost(c, Real(beta), Real(ambient)) instead of the centre value
  // c; beta = 0 gives c, the insulated wall.  Once any face is convective the
  // insulated faces of the same call are evaluated as coefficient 0 (every
  // backend alike).  Honoured where `wall` is: cpu::stencil / stencil_multi and
  // the convective forms of the lean sweep (stencil_tbl_conv.hip; with a source
  // stencil_tbl_conv_src.hip) and of the tv sweep (stencil_tbv_conv.hip).
  double wall_beta[3][2] = {{-1, -1}, {-1, -1}, {-1, -1}};
  double ambient = 0;
  // Relative volumetric heat capacity rc >= 1, stored as s = dtype(1 / rc) in
  // (0, 1]: a static field in the same Layout, of which only the centre value
  // of an updated point is read (ghosts and wall vertices hold 1).  Every
  // updated point is evaluated by cap_update below: the increment of the step
  // (steady_increment / steady_increment_var, plus the source) scaled by s in
  // one fused multiply-add onto the centre value.  nullptr: one capacity
  // everywhere, the kernels above.  Honoured by cpu::stencil / stencil_multi
  // (with `wall` / `wall_beta` too), by the single-step gfx950 kernels of
  // stencil_cap.hip (hip::stencil dispatches there) and, together with `cond`,
  // by the tc sweeps (stencil_tbc.hip: the values on the ghost layers an update
  // range reaches must then be the neighbours' 1 / rc); every other gfx950
  // stencil entry refuses it with an Error.  Not part of form().
  const void* cap = nullptr;
  // the one place that reads src, wall and wall_beta for the form of the call
  SweepForm form() const {
    SweepForm f;
    f.src = src != nullptr;
    for (int a = 0; a < 3; ++a)
      for (int e = 0; e < 2; ++e)
        if (wall[a][e] != kNoWall) {
          if (wall_beta[a][e] >= 0) f.wall = WallKind::Convective;
          else if (f.wall == WallKind::None) f.wall = WallKind::Insulated;
        }
    return f;
  }
  bool has_walls() const { return form().wall != WallKind::None; }
};

struct InitParams {
  void* field = nullptr;
  Layout L;
  int64_t gstart[3] = {0, 0, 0};  // global index of owned (0,0,0)
  int64_t N[3] = {0, 0, 0};
  double h[3] = {0, 0, 0};
};

// Apply the Dirichlet boundary value at a global vertex (heat3D.cu:414-453
// order: TOP (y = 1) <- 1.0, then LEFT/RIGHT/BACK/FRONT <- y overwrite,
// BOTTOM stays 0; interior 0).
H3D_HD inline double boundary_value(int64_t gi, int64_t gj, int64_t gk, const int64_t N[3],
                             const double h[3]) {
  if (gi == 0 || gi == N[0] - 1 || gk == 0 || gk == N[2] - 1)
    return static_cast<double>(gj) * h[1];
  if (gj == N[1] - 1) return 1.0;
  return 0.0;
}

namespace hip {
void init_field(DType t, const InitParams& p, void* stream);
void stencil(DType t, const StencilParams& p, const KernelSpec& k, void* stream);
// its conductivity forms (stencil_var.hip; stencil() dispatches here when p.cond is set)
void stencil_var(DType t, const StencilParams& p, const KernelSpec& k, void* stream);
// its heat-capacity forms (stencil_cap.hip; stencil() dispatches here when p.cap is set)
void stencil_cap(DType t, const StencilParams& p, const KernelSpec& k, void* stream);
// K-step temporally blocked sweep, lean kernel (stencil_tbl.hip), K = k.K
void stencil_lean(DType t, const StencilParams& p, const KernelSpec& k, void* stream);
// z tile stride of the lean kernel for a box (host-side choice, stencil_tbl.hip)
int lean_z_stride(int64_t nx, int64_t ny, int64_t nz, int K, int esize, int TY, int slots, int U, int L);
// The x plan the sweep kernels would take for a box of nx planes and `tiles`
// tiles on `slots` resident workgroups (seg > 0: fixed segments, -1: equal
// segments, 0: auto), with its greedy-dispatch makespan in plane steps
struct XPlanInfo {
  int seg = 1, n1 = 0, r = 0, split = 0, nb2 = 0;
  double makespan = 0;
};
XPlanInfo describe_xplan(int64_t nx, int64_t tiles, int slots, int fill, int U, int seg);
// The `count` fixed x-segment lengths (>= U planes, any length: a tile's last
// piece may be short) with the smallest modelled makespan for `tiles` tiles of
// nx planes on `slots` workgroups, best first.  Equal segments (nx / k) leave
// slots idle or add a round when tiles x k is just above a multiple of the
// slots; e.g. 1022^3 fp32 pairs (225 tiles): 918-plane segments model 932
// plane-steps per slot against the x plan's 1024 (ideal 902).
std::vector<int> best_fixed_segments(int64_t nx, int64_t tiles, int slots, int fill, int U, int count);

// sweep schedules chosen by timing (StencilParams::tune): kernel, box, the
// winning z tile stride and spec-field-L value (-3 = the model's x plan, > 0
// fixed segments) and the measured ms of the winner and of the model's choice
struct TunedSchedule {
  std::string kernel;
  int64_t nx = 0, ny = 0, nz = 0;
  int zs = 0;  // z tile stride
  int L = 0;
  double ms = 0, ms_model = 0;
  int candidates = 0;
};
std::vector<TunedSchedule> tuned_schedules();
// fp32 lean kernel on packed pairs of z columns (stencil_tbp.hip; spec tlK:2:…)
void stencil_lean_pair(DType t, const StencilParams& p, const KernelSpec& k, void* stream);
bool lean_pair_supported(DType t, const KernelSpec& k);
// z tile stride of the pair kernel for a box (host-side choice, stencil_tbp.hip)
int pair_z_stride(int64_t nx, int64_t ny, int64_t nz, int K, int TY, int slots, int U, int L, int esize);
// Is the lean kernel variant that k resolves to for dtype t instantiated in
// the given form (StencilParams::form)?
bool lean_supported(DType t, const KernelSpec& k, SweepForm form = {});
// The tile of a lean launch: R rows per wave, WY waves, SW the y-marching form
struct LeanShape {
  int R = 0, WY = 0;
  bool SW = false;
};
// The thin-slab rule of every lean dispatch: a box of few x planes and long
// rows (the boundary slabs of x-slab decompositions) under a default spec (no
// V, R, WY, Q field) runs as y-marching tiles of WY waves x R x-rows: 5 x 2 for
// the 4-plane slabs of a K = 3 sweep, 3 x 3 for its other slabs of up to 2K
// planes, 4 x 3 for slabs of up to K = 4 planes.  false: the x-marching tile.
// Why: 3-wave tiles of 9 x-rows marching along y (launch_tbl swap_xy) instead
// of 48-row tiles marching 3 planes plus a 4-plane pipeline fill along x.
// Phantom rank of the 1024^3 fp64 slab bench (64 GB/s emulated links): 8 ranks
// 0.2135 -> 0.2084 ms per step, 4 ranks 0.379 -> 0.359, 2 ranks unchanged
// (profiles/boundary_slabs_r02.md).  4-plane slabs of a K = 3 sweep before a
// long sweep (Solver::enqueue_multi thick): 5-wave tiles of 10 x-rows store all
// 4 planes in one tile; the (K+1)-plane boundary slabs of long sweeps across x
// halos (K = 4): 4-wave tiles of 12 x-rows store the 4 slab planes.
// Each tile is tied to its depth here, and every form's list has the three
// tiles at those depths (SW lines) in both dtypes.
inline bool lean_thin_slab(int K, bool default_spec, int64_t extent_x, int64_t extent_y, LeanShape* shape) {
  if (!default_spec || extent_x <= 0 || extent_y < 16 * extent_x) return false;
  if (K == 3 && extent_x == 4) *shape = {2, 5, true};
  else if (K == 3 && extent_x <= 2 * K) *shape = {3, 3, true};
  else if (K == 4 && extent_x <= K) *shape = {3, 4, true};
  else return false;
  return true;
}
// The lean sweep's dispatch of any form: launches *p with the variant k
// resolves to, or (p == nullptr) only reports whether that variant exists;
// either way *shape, if given, receives the tile that runs (unchanged for the
// packed-pair kernel of stencil_tbp.hip, which has no such tile).
bool lean_dispatch(DType t, SweepForm form, const StencilParams* p, const KernelSpec& k, void* stream,
                   LeanShape* shape = nullptr);
// Convective walls on single steps: dst box (one wall plane) <- the ghost value
// convective_ghost of the src box (the first interior plane), same field
void refresh_convective(DType t, void* f, const Layout& L, const Box& bs, const Box& bd, double beta,
                        double ambient, void* stream);
// K-step sweep with a conductivity field (stencil_tbv.hip; spec tvK): needs
// p.cond, honours p.src and p.wall / p.wall_beta (the wall forms of
// stencil_tbv_wall.hip / stencil_tbv_conv.hip; a form that is not built is an
// Error naming it, and nothing is written); no fused check, no schedule tuning
void stencil_cond_sweep(DType t, const StencilParams& p, const KernelSpec& k, void* stream);
// Is the tv kernel of k's depth built for dtype t in the given form (source
// flag and wall kind, StencilParams::form)?  *shape, if given, receives the
// tile (R rows x WY waves) that runs it.  No device access.
bool cond_sweep_supported(DType t, const KernelSpec& k, SweepForm form = {}, LeanShape* shape = nullptr);
// (the form without walls; with_source: its heat-source form)
bool cond_sweep_supported(DType t, const KernelSpec& k, bool with_source);
// deepest tv depth built for dtype t in the given form, every shallower depth
// down to 2 being built in it too (0: none)
int cond_sweep_max_depth(DType t, SweepForm form = {});
// K-step sweep with a conductivity field and a heat capacity (stencil_tbc.hip;
// spec tcK): the tv sweep whose every stage ends in cap_update.  Needs p.cond
// and p.cap (without either: an Error naming the family that runs the call),
// honours p.src and p.wall / p.wall_beta (stencil_tbc_wall.hip,
// stencil_tbc_conv.hip); a form that is not built is an Error naming it, and
// nothing is written; no fused check, no schedule tuning
void stencil_cap_sweep(DType t, const StencilParams& p, const KernelSpec& k, void* stream);
// Is the tc kernel of k's depth built for dtype t in the given form?  *shape,
// if given, receives the tile (R rows x WY waves) that runs it.  No device access.
bool cap_sweep_supported(DType t, const KernelSpec& k, SweepForm form = {}, LeanShape* shape = nullptr);
// deepest tc depth built for dtype t in the given form, every shallower depth
// down to 2 being built in it too (0: none)
int cap_sweep_max_depth(DType t, SweepForm form = {});
// Any multi-step kind -> its kernel
void sweep(DType t, const StencilParams& p, const KernelSpec& k, void* stream);
void pack_box(DType t, const void* f, const Layout& L, const Box& b, void* buf, void* stream);
void unpack_box(DType t, void* f, const Layout& L, const Box& b, const void* buf, void* stream);
void copy_box(DType t, const void* src, const Layout& Ls, const Box& bs, void* dst,
              const Layout& Ld, const Box& bd, void* stream);
void check_convergence(DeviceState* s, int slot, void* stream, int count = 1, bool last_only = false);
// kernel of `blocks` one-wave workgroups spinning for `us` microseconds on the
// 100 MHz real-time clock (each holds a wave slot of one CU while it spins)
// fat: in RCCL's device-kernel footprint (256 threads, 140 VGPRs, 20 KB LDS)
void delay(double us, void* stream, int blocks = 1, bool fat = false);
void stamp(void* slot, void* stream);
void delay_since(const void* slot, double us, void* stream, int blocks = 1, bool fat = false);
// a phantom transfer paced at the wire rate (phantom_comm.cpp, --phantom-wire
// paced): 16-byte aligned, ticks of the 100 MHz clock per 16 bytes of one
// workgroup's share
struct PacedCopy {
  const void* src = nullptr;
  void* dst = nullptr;
  int64_t bytes = 0;
  double ticks_per16 = 0.0;
};
constexpr int kPacedMax = 8;  // transfers per launch
void paced_copy(const PacedCopy* xs, int n, int per, void* stream, bool fat = false);
// placement probe: out[b] = XCC << 8 | SE/SH/CU id of workgroup b (blocks x 64 threads)
void cu_probe(unsigned* out, int blocks, double us, void* stream);
// Device-side stream dependencies of per-stream hipGraphs (hip_backend.cpp):
// signal stores 1 into *slot (release, agent scope) once the work before it on
// its stream is complete; wait spins (acquire) until its slots are != 0.  A wait that
// outlasts `timeout_s` sets st->fault = 2 and st->done (every later sweep is
// then a no-op) and returns, so a broken dependency cannot hang the GPU.
void graph_signal(unsigned* slot, void* stream);
// (wait: on every one of `n` <= 4 slots)
void graph_wait(const unsigned* const* slots, int n, DeviceState* st, void* stream);
// Adds Σ|T - y| and the point count over `box` into s->error_sum/error_count.
// `scratch` must hold at least error_scratch_elems() doubles.
void error_accumulate(DType t, const void* f, const Layout& L, const Box& box,
                      const int64_t gstart[3], double hy, double* scratch, DeviceState* s,
                      void* stream);
int64_t error_scratch_elems();
// The heat balance of one box (heat_balance.hpp; heat_balance.hip): the raw
// double-double sums, min / max keys and non-finite count of p into *out, or
// added to *out (accumulate: the next subdomain of the same process, in call
// order).  One pass over p.box on a fixed grid, per-block partials in
// `scratch` (balance_scratch_bytes() of device memory), one single-block
// kernel that combines them in a fixed order: no atomics, the same bits for
// the same call.  Wall vertices of insulated / convective faces are not read
// as temperatures.
void heat_balance(DType t, const BalanceParams& p, void* scratch, BalanceSums* out, bool accumulate, void* stream);
std::size_t balance_scratch_bytes();
// The steady solve's three operations (steady_cg.hpp; steady_cg.hip), fp64:
// q = A p (or r = b - A T) with its dot product, x += alpha p / r -= alpha q
// with r . r, p = r + beta p.  The dot products go through per-block partials
// in `scratch` (steady_scratch_bytes() of device memory) and a single-block
// kernel that combines them in a fixed order into out[0..1] = (hi, lo), or adds
// them to it (accumulate: the next subdomain of the same process).  No atomics,
// no scratch memory.  steady_scalars runs steady_scalars_step on the device.
void steady_apply(DType t, const SteadyApplyParams& p, void* scratch, double* out, bool accumulate, void* stream);
void steady_update(DType t, const SteadyUpdateParams& p, void* scratch, double* out, bool accumulate, void* stream);
void steady_direction(DType t, const SteadyDirectionParams& p, void* stream);
void steady_scalars(SteadyState* st, int phase, void* stream);
std::size_t steady_scratch_bytes();
// Fault injection (tests): write `value` at local owned point (i,j,k).
void poke(DType t, void* f, const Layout& L, int64_t i, int64_t j, int64_t k, double value,
          void* stream);
// Order-independent checksum (sum of bit patterns mod 2^64) of a box -> *out (device).
void box_bitsum(DType t, const void* f, const Layout& L, const Box& b, unsigned long long* out,
                void* stream);
// HBM calibration: kind 0 = 16 B/lane copy src->dst, 1 = 16 B/lane read of src.
void bandwidth_probe(int kind, const void* src, void* dst, int64_t bytes, int blocks, void* stream);
}  // namespace hip

namespace cpu {
void set_threads(int n);
void init_field(DType t, const InitParams& p);
void stencil(DType t, const StencilParams& p);
// Definition of the K-step sweep kernels: K single steps through two scratch
// fields (allocated by the caller, L.bytes() each).  Step s updates the box
// widened by K-1-s planes into [ux0, ux1) and accumulates into residual slot
// slot + s.
void stencil_multi(DType t, const StencilParams& p, int K, void* scratch0, void* scratch1);
void pack_box(DType t, const void* f, const Layout& L, const Box& b, void* buf);
void unpack_box(DType t, void* f, const Layout& L, const Box& b, const void* buf);
void copy_box(DType t, const void* src, const Layout& Ls, const Box& bs, void* dst,
              const Layout& Ld, const Box& bd);
void refresh_convective(DType t, void* f, const Layout& L, const Box& bs, const Box& bd, double beta,
                        double ambient);
void check_convergence(DeviceState* s, int slot);
void error_accumulate(DType t, const void* f, const Layout& L, const Box& box,
                      const int64_t gstart[3], double hy, DeviceState* s);
void poke(DType t, void* f, const Layout& L, int64_t i, int64_t j, int64_t k, double value);
unsigned long long box_bitsum(DType t, const void* f, const Layout& L, const Box& b);
// The definition of the heat balance (heat_balance.hpp): rows of p.box in fixed
// chunks, each summed in order, the chunks combined in order, so the result
// does not depend on the thread count.  *out is set, or added to (accumulate).
void heat_balance(DType t, const BalanceParams& p, BalanceSums* out, bool accumulate);
// The definitions of the steady solve's operations (steady_cg_cpu.cpp): rows of
// the box in the fixed chunks of cpu::heat_balance, each summed in order, the
// chunks combined in order: the same bits for every thread count.
void steady_apply(DType t, const SteadyApplyParams& p, double* out, bool accumulate);
void steady_update(DType t, const SteadyUpdateParams& p, double* out, bool accumulate);
void steady_direction(DType t, const SteadyDirectionParams& p);
}  // namespace cpu

// Shared scalar logic of the convergence check (heat3D.cu:1026-1073 with the
// survey's fixes: global norm, global max residual).  Used verbatim by the
// CPU backend and mirrored by the single-thread HIP kernel.
// FTCS 7-point update of heat3D.cu:128-131,
//   T + Dx*(T[i+1] - 2T + T[i-1]) + Dy*(...) + Dz*(...),
// evaluated the way nvcc compiles it for the reference's GPU kernel (default
// -fmad=true): left to right, every "acc + D*a" contracted to one fused
// multiply-add, and "T[i+1] - 2T" to fma(-2, T, T[i+1]) (2T is exact, so that
// one is the same value either way).  Written with explicit fused operations
// so that the CPU backend (libm fma, correctly rounded) and every gfx950
// kernel (v_fma_f64 / v_fma_f32) produce bitwise identical fields.
H3D_HD inline double h3d_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
H3D_HD inline float h3d_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
template <typename Real>
H3D_HD inline Real ftcs_update(Real c, Real xm, Real xp, Real ym, Real yp, Real zm, Real zp, Real Dx,
                               Real Dy, Real Dz) {
  const Real ax = h3d_fma(Real(-2), c, xp) + xm;
  const Real ay = h3d_fma(Real(-2), c, yp) + ym;
  const Real az = h3d_fma(Real(-2), c, zp) + zm;
  return h3d_fma(Dz, az, h3d_fma(Dy, ay, h3d_fma(Dx, ax, c)));
}

// The value a convective (Robin) wall presents to the update of its first
// interior point c: the ghost T_0 = T_1 + beta (T_inf - T_1), one subtraction
// and one fused multiply-add.  beta = 0 gives c (the insulated wall's mirror
// ghost), beta = 1 the ambient up to rounding.
template <typename Real>
H3D_HD inline Real convective_ghost(Real c, Real beta, Real tinf) {
  return h3d_fma(beta, tinf - c, c);
}

// FTCS update with a volumetric heat source, T_t = alpha lap(T) + q:
//   T' = ftcs_update(...) + S,  S = dtype(dt * q) rounded once when the source
// is set.  The add is a separate, rounded operation, never contracted into
// the update's last fused multiply-add (every unit is built with
// -ffp-contract=off, as the plain adds inside ftcs_update require too).
template <typename Real>
H3D_HD inline Real add_source(Real u, Real S) {
  return u + S;
}
template <typename Real>
H3D_HD inline Real ftcs_update_src(Real c, Real xm, Real xp, Real ym, Real yp, Real zm, Real zp, Real Dx,
                                   Real Dy, Real Dz, Real S) {
  return add_source<Real>(ftcs_update<Real>(c, xm, xp, ym, yp, zm, zp, Dx, Dy, Dz), S);
}

// FTCS update with a spatially varying conductivity, T_t = div(kappa grad T),
// kappa = alpha * c(x, y, z), 0 < c <= 1.  The stored field is Ch = dtype(0.5 c)
// (scaled in double, rounded once), so the weight of a face, the arithmetic
// mean of c at its two vertices, is one plain rounded add, Ch[p] + Ch[q].  The
// add commutes: both cells of a face compute the same bit pattern, and the
// flux fx = w (T[q] - T[p]) that leaves one is exactly the flux that enters
// the other (the form is conservative).  Per axis
//   f = fma(w+, T+ - T, w- * (T- - T)),
// then T' = fma(Dz, fz, fma(Dy, fy, fma(Dx, fx, T))).  Arguments: the field's
// seven points, then Ch at the same seven points.  With c == 1 everywhere it
// equals ftcs_update up to rounding, not bitwise.  With c <= 1 the centre
// weight 1 - sum_a D_a (w_a+ + w_a-) stays >= 1 - 2 (Dx + Dy + Dz) >= 0: the
// update is a convex combination under the time step of the uniform problem.
template <typename Real>
H3D_HD inline Real var_flux(Real c, Real m, Real p, Real wm, Real wp) {
  return h3d_fma(wp, p - c, wm * (m - c));
}
// the update from the six face weights (kernels that carry a weight from one
// point to the next: w- of a point is w+ of its predecessor, bit for bit)
template <typename Real>
H3D_HD inline Real ftcs_update_varw(Real c, Real xm, Real xp, Real ym, Real yp, Real zm, Real zp, Real wxm, Real wxp,
                                    Real wym, Real wyp, Real wzm, Real wzp, Real Dx, Real Dy, Real Dz) {
  const Real fx = var_flux<Real>(c, xm, xp, wxm, wxp);
  const Real fy = var_flux<Real>(c, ym, yp, wym, wyp);
  const Real fz = var_flux<Real>(c, zm, zp, wzm, wzp);
  return h3d_fma(Dz, fz, h3d_fma(Dy, fy, h3d_fma(Dx, fx, c)));
}
template <typename Real>
H3D_HD inline Real ftcs_update_var(Real c, Real xm, Real xp, Real ym, Real yp, Real zm, Real zp, Real hc, Real hxm,
                                   Real hxp, Real hym, Real hyp, Real hzm, Real hzp, Real Dx, Real Dy, Real Dz) {
  return ftcs_update_varw<Real>(c, xm, xp, ym, yp, zm, zp, hc + hxm, hc + hxp, hc + hym, hc + hyp, hc + hzm,
                                hc + hzp, Dx, Dy, Dz);
}
template <typename Real>
H3D_HD inline Real ftcs_update_var_src(Real c, Real xm, Real xp, Real ym, Real yp, Real zm, Real zp, Real hc,
                                       Real hxm, Real hxp, Real hym, Real hyp, Real hzm, Real hzp, Real Dx, Real Dy,
                                       Real Dz, Real S) {
  return add_source<Real>(
      ftcs_update_var<Real>(c, xm, xp, ym, yp, zm, zp, hc, hxm, hxp, hym, hyp, hzm, hzp, Dx, Dy, Dz), S);
}

// ---- the steady solve (steady_cg.hpp) -----------------------------------------
// The increment of one step, G(T) - T without the source: the update's fused
// chain started from zero instead of from c, so the low bits that forming G(T)
// and subtracting c would round away are kept.  A p is its negation on the
// homogeneous problem, the residual b - A T the increment itself (plus S).
template <typename Real>
H3D_HD inline Real steady_increment(Real c, Real xm, Real xp, Real ym, Real yp, Real zm, Real zp, Real Dx, Real Dy,
                                    Real Dz) {
  const Real ax = h3d_fma(Real(-2), c, xp) + xm;
  const Real ay = h3d_fma(Real(-2), c, yp) + ym;
  const Real az = h3d_fma(Real(-2), c, zp) + zm;
  return h3d_fma(Dz, az, h3d_fma(Dy, ay, Dx * ax));
}
// the same with a conductivity (ftcs_update_var's fluxes and face weights)
template <typename Real>
H3D_HD inline Real steady_increment_var(Real c, Real xm, Real xp, Real ym, Real yp, Real zm, Real zp, Real hc,
                                        Real hxm, Real hxp, Real hym, Real hyp, Real hzm, Real hzp, Real Dx, Real Dy,
                                        Real Dz) {
  const Real fx = var_flux<Real>(c, xm, xp, hc + hxm, hc + hxp);
  const Real fy = var_flux<Real>(c, ym, yp, hc + hym, hc + hyp);
  const Real fz = var_flux<Real>(c, zm, zp, hc + hzm, hc + hzp);
  return h3d_fma(Dz, fz, h3d_fma(Dy, fy, Dx * fx));
}
// ... from the six face weights (the sweep kernels form each weight where it is
// used; the same operations in the same order)
template <typename Real>
H3D_HD inline Real steady_increment_varw(Real c, Real xm, Real xp, Real ym, Real yp, Real zm, Real zp, Real wxm,
                                         Real wxp, Real wym, Real wyp, Real wzm, Real wzp, Real Dx, Real Dy, Real Dz) {
  const Real fx = var_flux<Real>(c, xm, xp, wxm, wxp);
  const Real fy = var_flux<Real>(c, ym, yp, wym, wyp);
  const Real fz = var_flux<Real>(c, zm, zp, wzm, wzp);
  return h3d_fma(Dz, fz, h3d_fma(Dy, fy, Dx * fx));
}
// One step with a heat capacity, rc T_t = div(alpha c grad T) + q: the
// increment u of the step (steady_increment or steady_increment_var, then
// add_source) scaled by s = dtype(1 / rc) and added to the centre value in one
// fused multiply-add.  s <= 1, so T' stays a convex combination of T's seven
// points under the time step of the uniform problem.  With s == 1 it equals
// ftcs_update (whose chain starts from c) up to rounding, not bitwise.
template <typename Real>
H3D_HD inline Real cap_update(Real s, Real u, Real c) {
  return h3d_fma(s, u, c);
}
// The neighbour of c across a wall of the global grid (cpu_rows.cpp's ghost
// rules): an insulated face shows the centre value, a convective one its ghost
// (towards ambient 0 in A), a Dirichlet one the stored wall value (0 in A).
template <typename Real>
H3D_HD inline Real steady_wall_neighbour(int kind, bool residual, Real c, Real stored, Real beta, Real ambient) {
  if (kind == kWallInsulated) return c;
  if (kind == kWallConvective) return convective_ghost<Real>(c, beta, residual ? ambient : Real(0));
  return residual ? stored : Real(0);
}
// y <- a x + y, one fused multiply-add (x += alpha p, r -= alpha q, p = r + beta p)
template <typename Real>
H3D_HD inline Real steady_axpy(Real a, Real x, Real y) {
  return h3d_fma(a, x, y);
}
// The shifted operator of an implicit step at one point, (R + mu A) p with
// R = diag(rc) stored as s = 1 / rc: `inc` is the increment of the homogeneous
// step at p (steady_increment / steady_increment_var, so A p = -inc), one
// correctly rounded division and one fused multiply-add.  Without a capacity
// R = I and s is not read.
template <bool CAP, typename Real>
H3D_HD inline Real implicit_apply(Real qc, Real inc, Real mu, Real s) {
  if constexpr (CAP) return h3d_fma(-mu, inc, qc / s);
  else return h3d_fma(-mu, inc, qc);
}

// Residual term of one point, |T^{n+1} - T^n|, taken in the field's
// precision as the reference takes fabs(T - T0) in its field type
// (heat3D.cu:1030-1033), then widened (exactly) to double for the max.  In
// fp32 that is one subtraction instead of two conversions and a double
// subtraction; in fp64 it is the same value as before.
H3D_HD inline double resid_abs(double nv, double c) { return __builtin_fabs(nv - c); }
H3D_HD inline double resid_abs(float nv, float c) { return (double)__builtin_fabsf(nv - c); }
H3D_HD inline float resid_abs_r(float nv, float c) { return __builtin_fabsf(nv - c); }
H3D_HD inline double resid_abs_r(double nv, double c) { return __builtin_fabs(nv - c); }

H3D_HD inline void check_convergence_scalar(DeviceState* s, double r) {
  const int64_t t = s->iter;
  if (s->hist_cap > 0) s->hist[t % s->hist_cap] = r;
  if (!s->done) {
    s->last_residual = r;
    if (!(r == r) || r > 1.7976931348623157e308) {  // NaN or Inf
      s->fault = 1;
      s->done = 1;
      s->conv_iter = t;
    } else {
      if (t == 0 && r != 0.0) s->norm = r;
      if (r / s->norm < s->eps) {
        s->done = 1;
        s->conv_iter = t;
      }
    }
  }
  s->iter = t + 1;
}

}  // namespace heat3d
