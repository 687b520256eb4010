// heat3d-mi355x — single-step gfx950 kernels with a spatially varying heat
// capacity (kernels.hpp cap_update): rc T_t = div(alpha c grad T) + q, the
// stored field s = dtype(1 / rc) in (0, 1].
//
// A translation unit of its own, next to stencil_var.hip, so that the kernels
// without a capacity keep their code.  hip::stencil dispatches here when
// StencilParams::cap is set, with or without a conductivity (template
// argument COND) and a source (SRC).  One step at an updated point:
//   u  = steady_increment(...)      or steady_increment_var(...) with COND
//   u  = u + S                      with SRC
//   T' = fma(s, u, T)
//   * stencil_cap_tile: the structure of stencil_var_tile: a workgroup of
//     WZ x WY waves marches a (rows x z) tile along x, the field's x-1 / x /
//     x+1 planes in a register queue, y neighbour rows through LDS, z
//     neighbours through DPP, one barrier per plane, fused residual, the done
//     flag, XCD-aware block order, nontemporal stores by the spec's policy.
//     With COND the conductivity travels as it does there (its plane x through
//     the same LDS exchange, one plane of x face weights carried along the
//     march).  s has no neighbours: one more aligned vector load per row
//     and no LDS exchange; without a conductivity plane x + 1 is loaded at
//     the top of iteration x, ahead of the barrier; with one (the registers
//     are the conductivity's) the row is loaded where it is used, as the
//     source is.
//     HBM traffic per step: T, s and the write (three fields, what the
//     conductivity step moves); four with COND; one more with SRC.
//   * stencil_cap_naive: one lane per (y, z) column; thin boxes (z extent
//     below 32, a single y row), --kernel naive and the test oracle.
// One tile shape per dtype, the conductivity kernel's: fp64 V=2 R=4 WZ=1 WY=4,
// fp32 V=4 R=4 WZ=1 WY=4.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hip_helpers.hpp"

namespace heat3d {
namespace hip {

// steady_increment_var from the six face weights (the tile kernel carries the
// x weight from one plane to the next: w- of plane x + 1 is w+ of plane x bit
// for bit)
template <typename Real>
__device__ __forceinline__ Real cap_increment_varw(Real c, Real xm, Real xp, Real ym, Real yp, Real zm, Real zp,
                                                   Real wxm, Real wxp, Real wym, Real wyp, Real wzm, Real wzp,
                                                   Real Dx, Real Dy, Real Dz) {
  const Real fx = var_flux<Real>(c, xm, xp, wxm, wxp);
  const Real fy = var_flux<Real>(c, ym, yp, wym, wyp);
  const Real fz = var_flux<Real>(c, zm, zp, wzm, wzp);
  return h3d_fma(Dz, fz, h3d_fma(Dy, fy, Dx * fx));
}

template <typename Real, bool COND, bool SRC>
__global__ __launch_bounds__(256) void stencil_cap_naive(const Real* __restrict__ in, Real* __restrict__ out,
                                                         const Real* __restrict__ h,
                                                         const Real* __restrict__ src,
                                                         const Real* __restrict__ cap, Layout L, Box b, Real Dx,
                                                         Real Dy, Real Dz, unsigned long long* res,
                                                         const int* done) {
  if (flag_set(done)) return;
  const int64_t k = b.lo[2] + (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const int64_t j = b.lo[1] + (int64_t)blockIdx.y * 4 + (threadIdx.x >> 6);
  const int64_t x0 = b.lo[0] + (int64_t)blockIdx.z * 64;
  const int64_t x1 = min(x0 + 64, b.hi[0]);
  double m = 0.0;
  if (k < b.hi[2] && j < b.hi[1]) {
    const int64_t sx = L.sx, sy = L.sy;
    for (int64_t i = x0; i < x1; ++i) {
      const int64_t c = L.index(i, j, k);
      const Real T = in[c];
      Real u;
      if constexpr (COND)
        u = steady_increment_var<Real>(T, in[c - sx], in[c + sx], in[c - sy], in[c + sy], in[c - 1], in[c + 1], h[c],
                                       h[c - sx], h[c + sx], h[c - sy], h[c + sy], h[c - 1], h[c + 1], Dx, Dy, Dz);
      else
        u = steady_increment<Real>(T, in[c - sx], in[c + sx], in[c - sy], in[c + sy], in[c - 1], in[c + 1], Dx, Dy,
                                   Dz);
      if constexpr (SRC) u = add_source<Real>(u, src[c]);
      const Real nv = cap_update<Real>(cap[c], u, T);
      out[c] = nv;
      m = res_max(m, resid_abs(nv, T));
    }
  }
  if (res) residual_commit(res, m);
}

struct CapGeom {
  int64_t z0a;        // first z of tile column 0 (box z0 rounded down to V)
  int nzb, nyb, nxs;  // tiles along z, y; x segments
  int seg;
  int64_t nblocks;
  int xq, xr;         // XCD remap
  int nt;
};

template <typename Real, int V, int R, int WZ, int WY, bool COND, bool SRC>
__global__ __launch_bounds__(64 * WZ * WY) void stencil_cap_tile(const Real* __restrict__ in,
                                                                Real* __restrict__ out,
                                                                const Real* __restrict__ hf,
                                                                const Real* __restrict__ src,
                                                                const Real* __restrict__ cap, Layout L, Box b,
                                                                CapGeom g, Real Dx, Real Dy, Real Dz,
                                                                unsigned long long* res, const int* done) {
  typedef typename VecOf<Real, V>::type Vec;
  constexpr int TZ = 64 * V;
  constexpr int NW = WZ * WY;
  constexpr int NF = COND ? 2 : 1;  // fields that travel through LDS: T, and Ch with COND
  // [parity][field: T, Ch][wave][bottom/top row][lane]
  __shared__ Vec s_rows[2][NF][NW][2][64];
  // [parity][field][wave][row][left/right]
  __shared__ Real s_edge[2][NF][NW][R][2];
  if (flag_set(done)) return;  // uniform across the block

  const int blk = blockIdx.x;
  const int xcd = blk & 7;
  int64_t t = xcd * g.xq + min(xcd, g.xr) + (blk >> 3);
  const int zb = (int)(t % g.nzb);
  t /= g.nzb;
  const int ybk = (int)(t % g.nyb);
  const int xs = (int)(t / g.nyb);

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int wz = wave % WZ, wy = wave / WZ;
  const int64_t kb = g.z0a + ((int64_t)zb * WZ + wz) * TZ;
  const int64_t k = kb + (int64_t)lane * V;
  const int64_t yb = b.lo[1] + ((int64_t)ybk * WY + wy) * R;
  const int ract = (int)max((int64_t)0, min((int64_t)R, b.hi[1] - yb));
  // neighbours in the tile: below (wy-1) always has R rows; above only if I am full
  const bool nb_lo = wy > 0;
  const bool nb_hi = (wy + 1 < WY) && (ract == R) && (yb + R < b.hi[1]);
  const bool nb_left = wz > 0, nb_right = wz + 1 < WZ;
  const int64_t xa = b.lo[0] + (int64_t)xs * g.seg;
  const int64_t xe = min(xa + (int64_t)g.seg, b.hi[0]);
  const int64_t sx = L.sx, sy = L.sy;

  bool valid[V];
  bool allvalid = true;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    valid[v] = (k + v >= b.lo[2]) && (k + v < b.hi[2]);
    allvalid &= valid[v];
  }
  const int64_t base0 = L.index(0, yb, k);
  // outer-edge gather: lanes [0,R) left edges (only the wz == 0 wave), lanes
  // [32,32+R) right edges (only the wz == WZ-1 wave)
  const int er = lane < 32 ? lane : lane - 32;
  const bool eload = er < ract && (lane < 32 ? !nb_left : !nb_right);
  const int64_t ebase = L.index(0, yb + er, lane < 32 ? kb - 1 : kb + TZ);

  auto ld = [&](const Real* f, int64_t plane, int r) -> Vec {
    return *reinterpret_cast<const Vec*>(f + base0 + plane * sx + (int64_t)r * sy);
  };

  Vec qm[R], qc[R], qp[R];  // T planes x-1, x, x+1
  Vec sc[R];                // s plane x
  Vec hc[R], wx[R];         // COND: Ch plane x; face weights between planes x-1 and x
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (r < ract) {
      qm[r] = ld(in, xa - 1, r);
      qc[r] = ld(in, xa, r);
      qp[r] = ld(in, xa + 1, r);
      if constexpr (!COND) sc[r] = ld(cap, xa, r);
      if constexpr (COND) {
        hc[r] = ld(hf, xa, r);
        const Vec hm = ld(hf, xa - 1, r);
#pragma unroll
        for (int v = 0; v < V; ++v) wx[r][v] = hc[r][v] + hm[v];
      }
    }
  Vec hb = {}, ht = {}, gb = {}, gt = {};  // outer halo rows of T and of Ch, plane x
  if (ract > 0 && !nb_lo) {
    hb = ld(in, xa, -1);
    if constexpr (COND) gb = ld(hf, xa, -1);
  }
  if (ract > 0 && !nb_hi) {
    ht = ld(in, xa, ract);
    if constexpr (COND) gt = ld(hf, xa, ract);
  }
  Real ed = eload ? in[ebase + xa * sx] : Real(0);
  Real eg = Real(0);
  if constexpr (COND) eg = eload ? hf[ebase + xa * sx] : Real(0);

  double m = 0.0;
  int par = 0;
  for (int64_t x = xa; x < xe; ++x) {
    // publish this wave's boundary rows / edge points of plane x, T and Ch
    if (ract > 0) {
      s_rows[par][0][wave][0][lane] = qc[0];
      if constexpr (COND) s_rows[par][NF - 1][wave][0][lane] = hc[0];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r == ract - 1) {  // static register index
          s_rows[par][0][wave][1][lane] = qc[r];
          if constexpr (COND) s_rows[par][NF - 1][wave][1][lane] = hc[r];
        }
        if (r < ract) {
          if (lane == 0) {
            s_edge[par][0][wave][r][0] = qc[r][0];
            if constexpr (COND) s_edge[par][NF - 1][wave][r][0] = hc[r][0];
          }
          if (lane == 63) {
            s_edge[par][0][wave][r][1] = qc[r][V - 1];
            if constexpr (COND) s_edge[par][NF - 1][wave][r][1] = hc[r][V - 1];
          }
        }
      }
    }
    // Ch of plane x+1 (this plane's w+); prefetch T plane x+2, s of plane x+1
    // (without a conductivity) and the outer halo of plane x+1
    Vec hn[R], qn[R], sn[R];
    Vec hbn = {}, htn = {}, gbn = {}, gtn = {};
    Real edn = Real(0), egn = Real(0);
    const bool more = x + 1 < xe;
    if (ract > 0) {
      if constexpr (COND) {
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (r < ract) hn[r] = ld(hf, x + 1, r);
      }
      if (more) {
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (r < ract) {
            qn[r] = ld(in, x + 2, r);
            if constexpr (!COND) sn[r] = ld(cap, x + 1, r);
          }
        if (!nb_lo) {
          hbn = ld(in, x + 1, -1);
          if constexpr (COND) gbn = ld(hf, x + 1, -1);
        }
        if (!nb_hi) {
          htn = ld(in, x + 1, ract);
          if constexpr (COND) gtn = ld(hf, x + 1, ract);
        }
        if (eload) {
          edn = in[ebase + (x + 1) * sx];
          if constexpr (COND) egn = hf[ebase + (x + 1) * sx];
        }
      }
    }
    __syncthreads();
    if (ract > 0) {
      const Vec ylo = nb_lo ? s_rows[par][0][wave - WZ][1][lane] : hb;
      const Vec yhi = nb_hi ? s_rows[par][0][wave + WZ][0][lane] : ht;
      Vec glo = {}, ghi = {};
      if constexpr (COND) {
        glo = nb_lo ? s_rows[par][NF - 1][wave - WZ][1][lane] : gb;
        ghi = nb_hi ? s_rows[par][NF - 1][wave + WZ][0][lane] : gt;
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r < ract) {
          const Vec c = qc[r];
          Vec sv = {};
          if constexpr (SRC) sv = *reinterpret_cast<const Vec*>(src + base0 + x * sx + (int64_t)r * sy);
          // (with a conductivity s is loaded here, as the source is: no registers for a plane ahead)
          if constexpr (COND) sc[r] = ld(cap, x, r);
          const Vec ym = r == 0 ? ylo : qc[r > 0 ? r - 1 : 0];
          const Vec yp = (r == ract - 1) ? yhi : qc[r + 1 < R ? r + 1 : R - 1];
          const Real left = nb_left ? s_edge[par][0][wave - 1][r][1] : readlane(ed, r);
          const Real right = nb_right ? s_edge[par][0][wave + 1][r][0] : readlane(ed, 32 + r);
          Vec zm, zp, nv;
#pragma unroll
          for (int v = 0; v < V; ++v) {
            zm[v] = v == 0 ? dpp_shr1(left, c[V - 1]) : c[v > 0 ? v - 1 : 0];
            zp[v] = v == V - 1 ? dpp_shl1(right, c[0]) : c[v + 1 < V ? v + 1 : 0];
          }
          Vec u;
          if constexpr (COND) {
            const Vec h = hc[r];
            const Vec gm = r == 0 ? glo : hc[r > 0 ? r - 1 : 0];
            const Vec gp = (r == ract - 1) ? ghi : hc[r + 1 < R ? r + 1 : R - 1];
            const Real hleft = nb_left ? s_edge[par][NF - 1][wave - 1][r][1] : readlane(eg, r);
            const Real hright = nb_right ? s_edge[par][NF - 1][wave + 1][r][0] : readlane(eg, 32 + r);
            Vec hzm, hzp, wxp;
#pragma unroll
            for (int v = 0; v < V; ++v) {
              hzm[v] = v == 0 ? dpp_shr1(hleft, h[V - 1]) : h[v > 0 ? v - 1 : 0];
              hzp[v] = v == V - 1 ? dpp_shl1(hright, h[0]) : h[v + 1 < V ? v + 1 : 0];
            }
#pragma unroll
            for (int v = 0; v < V; ++v) {
              wxp[v] = h[v] + hn[r][v];
              u[v] = cap_increment_varw<Real>(c[v], qm[r][v], qp[r][v], ym[v], yp[v], zm[v], zp[v], wx[r][v], wxp[v],
                                              h[v] + gm[v], h[v] + gp[v], h[v] + hzm[v], h[v] + hzp[v], Dx, Dy, Dz);
            }
            wx[r] = wxp;  // w- of plane x+1
          } else {
#pragma unroll
            for (int v = 0; v < V; ++v)
              u[v] = steady_increment<Real>(c[v], qm[r][v], qp[r][v], ym[v], yp[v], zm[v], zp[v], Dx, Dy, Dz);
          }
#pragma unroll
          for (int v = 0; v < V; ++v) {
            if constexpr (SRC) u[v] = add_source<Real>(u[v], sv[v]);
            nv[v] = cap_update<Real>(sc[r][v], u[v], c[v]);
            if (valid[v]) m = res_max(m, resid_abs(nv[v], c[v]));
          }
          Real* dst = out + base0 + x * sx + (int64_t)r * sy;
          if (allvalid) {
            if (g.nt) __builtin_nontemporal_store(nv, reinterpret_cast<Vec*>(dst));
            else *reinterpret_cast<Vec*>(dst) = nv;
          } else {
#pragma unroll
            for (int v = 0; v < V; ++v)
              if (valid[v]) dst[v] = nv[v];
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      qm[r] = qc[r];
      qc[r] = qp[r];
      qp[r] = qn[r];
      if constexpr (COND) hc[r] = hn[r];
      else sc[r] = sn[r];
    }
    hb = hbn;
    ht = htn;
    gb = gbn;
    gt = gtn;
    ed = edn;
    eg = egn;
    par ^= 1;
  }
  if (res) residual_commit(res, m);
}

template <typename Real, bool COND, bool SRC>
static void launch_cap_naive(const StencilParams& p, hipStream_t s) {
  const Box& b = p.box;
  dim3 grid((unsigned)((b.extent(2) + 63) / 64), (unsigned)((b.extent(1) + 3) / 4),
            (unsigned)((b.extent(0) + 63) / 64));
  unsigned long long* res = p.state && p.residual ? &p.state->residual[p.slot] : nullptr;
  const int* done = p.state ? &p.state->done : nullptr;
  hipLaunchKernelGGL((stencil_cap_naive<Real, COND, SRC>), grid, dim3(256), 0, s, static_cast<const Real*>(p.in),
                     static_cast<Real*>(p.out), static_cast<const Real*>(p.cond), static_cast<const Real*>(p.src),
                     static_cast<const Real*>(p.cap), p.L, b, (Real)p.D[0], (Real)p.D[1], (Real)p.D[2], res, done);
  HIPK_CHECK(hipGetLastError());
}

template <typename Real, int V, int R, int WZ, int WY, bool COND, bool SRC>
static void launch_cap_tile(const StencilParams& p, const KernelSpec& k, hipStream_t s) {
  const Box& b = p.box;
  constexpr int TZ = 64 * V;
  CapGeom g;
  g.nt = k.NT;
  g.z0a = (b.lo[2] / V) * V;
  const int64_t nzt = (b.hi[2] - g.z0a + TZ - 1) / TZ;
  g.nzb = (int)((nzt + WZ - 1) / WZ);
  g.nyb = (int)((b.extent(1) + (int64_t)R * WY - 1) / ((int64_t)R * WY));
  int seg = k.L;
  if (seg <= 0) {
    static const int slots =
        device_slots(reinterpret_cast<const void*>(&stencil_cap_tile<Real, V, R, WZ, WY, COND, SRC>), 64 * WZ * WY);
    seg = choose_segment(b.extent(0), (int64_t)g.nzb * g.nyb, slots);
  }
  g.seg = (int)std::min<int64_t>(seg, std::max<int64_t>(1, b.extent(0)));
  g.nxs = (int)((b.extent(0) + g.seg - 1) / g.seg);
  g.nblocks = (int64_t)g.nzb * g.nyb * g.nxs;
  HEAT3D_CHECK(g.nblocks < (1LL << 31), "too many blocks");
  g.xq = (int)(g.nblocks / 8);
  g.xr = (int)(g.nblocks % 8);
  unsigned long long* res = p.state && p.residual ? &p.state->residual[p.slot] : nullptr;
  const int* done = p.state ? &p.state->done : nullptr;
  hipLaunchKernelGGL((stencil_cap_tile<Real, V, R, WZ, WY, COND, SRC>), dim3((unsigned)g.nblocks),
                     dim3(64 * WZ * WY), 0, s, static_cast<const Real*>(p.in), static_cast<Real*>(p.out),
                     static_cast<const Real*>(p.cond), static_cast<const Real*>(p.src),
                     static_cast<const Real*>(p.cap), p.L, b, g, (Real)p.D[0], (Real)p.D[1], (Real)p.D[2], res, done);
  HIPK_CHECK(hipGetLastError());
}

template <typename Real, bool COND, bool SRC>
static void dispatch_cap(const StencilParams& p, const KernelSpec& k, hipStream_t s) {
  // thin boxes as in the conductivity dispatch (dispatch_var)
  if (k.kind == KernelSpec::Naive || p.box.extent(2) < 32 || p.box.extent(1) < 2)
    return launch_cap_naive<Real, COND, SRC>(p, s);
  // (the spec's tile-shape fields belong to the uniform kernel; L and the
  // store policy apply)
  if constexpr (sizeof(Real) == 8) launch_cap_tile<Real, 2, 4, 1, 4, COND, SRC>(p, k, s);
  else launch_cap_tile<Real, 4, 4, 1, 4, COND, SRC>(p, k, s);
}

template <typename Real>
static void dispatch_cap_form(const StencilParams& p, const KernelSpec& k, hipStream_t s) {
  if (p.cond) {
    if (p.src) dispatch_cap<Real, true, true>(p, k, s);
    else dispatch_cap<Real, true, false>(p, k, s);
  } else {
    if (p.src) dispatch_cap<Real, false, true>(p, k, s);
    else dispatch_cap<Real, false, false>(p, k, s);
  }
}

void stencil_cap(DType t, const StencilParams& p, const KernelSpec& k, void* stream) {
  if (p.box.empty()) return;
  HEAT3D_CHECK(p.cap, "stencil_cap needs a heat-capacity field");
  // (never Dirichlet arithmetic next to an insulated wall)
  HEAT3D_CHECK(!p.has_walls(), "the single-step kernels take no StencilParams::wall: copy the wall planes from their "
                               "inward neighbours before the step (Solver::refresh_walls)");
  HEAT3D_CHECK(k.kind == KernelSpec::Naive || k.kind == KernelSpec::Tile, "single-step kernels: naive | tile");
  if (t == DType::F64) dispatch_cap_form<double>(p, k, S(stream));
  else dispatch_cap_form<float>(p, k, S(stream));
}

}  // namespace hip
}  // namespace heat3d
