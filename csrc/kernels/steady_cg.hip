// heat3d-mi355x — the steady solve's kernels on gfx950 (steady_cg.hpp; the
// definitions are in steady_cg_cpu.cpp).  fp64 only.
//
//   steady_apply_kernel   q = A p (or r = b - A T), one pass: a workgroup of
//       four waves owns a tile of 4 rows x 64 z columns and marches it along an
//       x segment with the planes x - 1, x, x + 1 of its own column in
//       registers (and of Ch, when there is a conductivity); the y and z
//       neighbours of plane x are loads that the rows of the same tile have just
//       brought into the cache.  Walls are substituted by value
//       (steady_wall_neighbour), never multiplied away, so a wall vertex may
//       hold anything.  Conductivity, residual form, source and "any wall in
//       reach" are template arguments.  Every lane adds its float64 products
//       p q (or r r) to one double-double accumulator.  The shifted A-forms of
//       an implicit step, q = (R + mu A) p (implicit_apply; with or without the
//       capacity field), are one more template argument.
//   steady_update_kernel  x += alpha p, r -= alpha q and r . r: a wave per z
//       row, four pieces loaded ahead of the arithmetic.  Two more forms: r
//       alone (r -= q, the true residual of an implicit step) and x alone
//       (T' = fma(m, d, T)).
//   steady_direction_kernel  p = r + beta p, the same shape.
//   steady_final_kernel   one workgroup combines the per-workgroup partials in a
//       fixed order (thread t takes t, t + 256, ...; then shuffles; then the
//       four waves in order).
//   steady_scalars_kernel one lane runs steady_scalars_step.
// Grids are fixed by the box alone, nothing is atomic: the same call returns
// the same bits.  alpha, beta and the stop flag are read from the device state
// by the kernel that consumes them; a set flag makes every kernel return at
// once.  No kernel uses scratch memory (tools/kres.sh).
#include "hip_helpers.hpp"

namespace heat3d {
namespace hip {

constexpr int kCgThreads = 256;
constexpr int kCgWaves = kCgThreads / 64;
constexpr int kCgMaxBlocks = 4096;  // partials per launch: 16 workgroups per CU
constexpr int kCgAhead = 4;

std::size_t steady_scratch_bytes() { return sizeof(DD) * kCgMaxBlocks; }

__device__ __forceinline__ DD cg_shfl_down(const DD& a, int o) {
  DD b;
  b.hi = __shfl_down(a.hi, o, 64);
  b.lo = __shfl_down(a.lo, o, 64);
  return b;
}

// thread 0 <- the workgroup's sum: lanes by shuffles, then the waves in order
__device__ __forceinline__ DD cg_block_sum(DD a, DD* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = dd_combine(a, cg_shfl_down(a, o));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    a = red[0];
    for (int w = 1; w < kCgWaves; ++w) a = dd_combine(a, red[w]);
  }
  return a;
}

__device__ __forceinline__ bool cg_done(const SteadyState* st) { return st != nullptr && st->done != 0; }

struct ApplyGeom {
  int nzb, nyb, nxs;  // tiles along z and y, x segments
  int seg;            // planes per x segment
  int64_t ntasks;
};

// SHIFT: 0 the plain forms, 1 the shifted A-form of an implicit step
// (implicit_apply), 2 the same with a capacity: s is one more streamed load at
// the centre of each updated point, issued where it is used
template <bool COND, bool RESID, bool SRC, bool WALLS, int SHIFT = 0>
__global__ __launch_bounds__(kCgThreads) void steady_apply_kernel(SteadyApplyParams p, ApplyGeom g, DD* partial) {
  static_assert(!(RESID && SHIFT), "the residual form is not shifted");
  __shared__ DD red[kCgWaves];
  if (cg_done(p.state)) return;  // uniform across the grid
  const double* __restrict__ in = static_cast<const double*>(p.in);
  double* __restrict__ out = static_cast<double*>(p.out);
  const double* __restrict__ h = static_cast<const double*>(p.cond);
  const double* __restrict__ S = static_cast<const double*>(p.src);
  const double* __restrict__ cap = static_cast<const double*>(p.cap);
  const Layout& L = p.L;
  const Box& b = p.box;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t sx = L.sx, sy = L.sy;
  const double Dx = p.D[0], Dy = p.D[1], Dz = p.D[2], tinf = p.ambient;
  DD acc{0.0, 0.0};
  for (int64_t task = blockIdx.x; task < g.ntasks; task += gridDim.x) {
    int64_t t = task;
    const int zb = (int)(t % g.nzb);
    t /= g.nzb;
    const int yb = (int)(t % g.nyb);
    const int xs = (int)(t / g.nyb);
    const int64_t k = b.lo[2] + (int64_t)zb * 64 + lane;
    const int64_t j = b.lo[1] + (int64_t)yb * kCgWaves + wave;
    const int64_t xa = b.lo[0] + (int64_t)xs * g.seg;
    const int64_t xe = min(xa + (int64_t)g.seg, b.hi[0]);
    if (k >= b.hi[2] || j >= b.hi[1]) continue;  // (no barrier inside the march)
    // walls of this column: y per wave, z per lane
    bool wym = false, wyp = false, wzm = false, wzp = false;
    if constexpr (WALLS) {
      wym = j == p.wall[1][0];
      wyp = j == p.wall[1][1];
      wzm = k == p.wall[2][0];
      wzp = k == p.wall[2][1];
    }
    int64_t c = L.index(xa, j, k);
    double qm = in[c - sx], qc = in[c], qp = in[c + sx];
    double hm = 0.0, hc = 0.0, hp = 0.0;
    if constexpr (COND) hm = h[c - sx], hc = h[c], hp = h[c + sx];
    for (int64_t x = xa; x < xe; ++x, c += sx) {
      // the next plane of this column, ahead of the arithmetic
      double qn = 0.0, hn = 0.0;
      if (x + 1 < xe) {
        qn = in[c + 2 * sx];
        if constexpr (COND) hn = h[c + 2 * sx];
      }
      double xm = qm, xp = qp;
      double ym = in[c - sy], yp = in[c + sy], zm = in[c - 1], zp = in[c + 1];
      if constexpr (WALLS) {
        if (x == p.wall[0][0]) xm = steady_wall_neighbour<double>(p.kind[0][0], RESID, qc, xm, p.beta[0][0], tinf);
        if (x == p.wall[0][1]) xp = steady_wall_neighbour<double>(p.kind[0][1], RESID, qc, xp, p.beta[0][1], tinf);
        if (wym) ym = steady_wall_neighbour<double>(p.kind[1][0], RESID, qc, ym, p.beta[1][0], tinf);
        if (wyp) yp = steady_wall_neighbour<double>(p.kind[1][1], RESID, qc, yp, p.beta[1][1], tinf);
        if (wzm) zm = steady_wall_neighbour<double>(p.kind[2][0], RESID, qc, zm, p.beta[2][0], tinf);
        if (wzp) zp = steady_wall_neighbour<double>(p.kind[2][1], RESID, qc, zp, p.beta[2][1], tinf);
      }
      double inc;
      if constexpr (COND)
        inc = steady_increment_var<double>(qc, xm, xp, ym, yp, zm, zp, hc, hm, hp, h[c - sy], h[c + sy], h[c - 1],
                                           h[c + 1], Dx, Dy, Dz);
      else
        inc = steady_increment<double>(qc, xm, xp, ym, yp, zm, zp, Dx, Dy, Dz);
      double v;
      if constexpr (RESID) {
        v = inc;
        if constexpr (SRC) v = add_source<double>(inc, S[c]);
      } else if constexpr (SHIFT == 2) {
        v = implicit_apply<true, double>(qc, inc, p.mu, cap[c]);
      } else if constexpr (SHIFT == 1) {
        v = implicit_apply<false, double>(qc, inc, p.mu, 0.0);
      } else {
        v = -inc;
      }
      out[c] = v;
      dd_add(acc, RESID ? v * v : qc * v);
      qm = qc;
      qc = qp;
      qp = qn;
      if constexpr (COND) {
        hm = hc;
        hc = hp;
        hp = hn;
      }
    }
  }
  acc = cg_block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// rows of the box, a wave each (row = wave of the grid, + waves of the grid, ...)
template <typename Body>
__device__ __forceinline__ void cg_rows(const Layout& L, const Box& b, Body body) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t ey = b.extent(1);
  const int64_t rows = b.extent(2) > 0 ? b.extent(0) * ey : 0;
  for (int64_t row = (int64_t)blockIdx.x * kCgWaves + wave; row < rows; row += (int64_t)gridDim.x * kCgWaves) {
    const int64_t base = L.index(b.lo[0] + row / ey, b.lo[1] + row % ey, 0);
    for (int64_t k0 = b.lo[2] + lane; k0 < b.hi[2]; k0 += (int64_t)64 * kCgAhead) body(base, k0, b.hi[2]);
  }
}

// XU: x += alpha p; RU: r -= alpha q with r . r (one of them at least)
template <bool XU, bool RU>
__global__ __launch_bounds__(kCgThreads) void steady_update_kernel(SteadyUpdateParams p, DD* partial) {
  __shared__ DD red[kCgWaves];
  if (cg_done(p.state)) return;
  const double alpha = p.state ? p.state->alpha : p.alpha;
  double* __restrict__ x = static_cast<double*>(p.x);
  double* __restrict__ r = static_cast<double*>(p.r);
  const double* __restrict__ d = static_cast<const double*>(p.p);
  const double* __restrict__ q = static_cast<const double*>(p.q);
  DD acc{0.0, 0.0};
  cg_rows(p.L, p.box, [&](int64_t base, int64_t k0, int64_t hi) {
    double xv[kCgAhead], rv[kCgAhead], dv[kCgAhead], qv[kCgAhead];
#pragma unroll
    for (int u = 0; u < kCgAhead; ++u) {
      const int64_t k = k0 + (int64_t)u * 64;
      if (k < hi) {
        if constexpr (XU) {
          xv[u] = x[base + k];
          dv[u] = d[base + k];
        }
        if constexpr (RU) {
          rv[u] = r[base + k];
          qv[u] = q[base + k];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kCgAhead; ++u) {
      const int64_t k = k0 + (int64_t)u * 64;
      if (k < hi) {
        if constexpr (XU) x[base + k] = steady_axpy<double>(alpha, dv[u], xv[u]);
        if constexpr (RU) {
          const double rn = steady_axpy<double>(-alpha, qv[u], rv[u]);
          r[base + k] = rn;
          dd_add(acc, rn * rn);
        }
      }
    }
  });
  acc = cg_block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kCgThreads) void steady_direction_kernel(SteadyDirectionParams p) {
  if (cg_done(p.state)) return;
  const double beta = p.state ? p.state->beta : p.beta;
  const bool copy = p.copy;
  double* __restrict__ d = static_cast<double*>(p.p);
  const double* __restrict__ r = static_cast<const double*>(p.r);
  cg_rows(p.L, p.box, [&](int64_t base, int64_t k0, int64_t hi) {
    double dv[kCgAhead], rv[kCgAhead];
#pragma unroll
    for (int u = 0; u < kCgAhead; ++u) {
      const int64_t k = k0 + (int64_t)u * 64;
      if (k < hi) {
        rv[u] = r[base + k];
        dv[u] = copy ? 0.0 : d[base + k];
      }
    }
#pragma unroll
    for (int u = 0; u < kCgAhead; ++u) {
      const int64_t k = k0 + (int64_t)u * 64;
      if (k < hi) d[base + k] = copy ? rv[u] : steady_axpy<double>(beta, dv[u], rv[u]);
    }
  });
}

__global__ __launch_bounds__(kCgThreads) void steady_final_kernel(const DD* partial, int n, double* out, int accumulate,
                                                                  const SteadyState* st) {
  __shared__ DD red[kCgWaves];
  if (cg_done(st)) return;
  DD mine{0.0, 0.0};
  for (int q = threadIdx.x; q < n; q += kCgThreads) mine = dd_combine(mine, partial[q]);
  mine = cg_block_sum(mine, red);
  if (threadIdx.x == 0) {
    if (accumulate) mine = dd_combine(DD{out[0], out[1]}, mine);
    out[0] = mine.hi;
    out[1] = mine.lo;
  }
}

__global__ void steady_scalars_kernel(SteadyState* st, int phase) {
  if (threadIdx.x == 0 && blockIdx.x == 0) steady_scalars_step(st, phase);
}

static void check_f64(DType t, const char* what) { HEAT3D_CHECK(t == DType::F64, what << ": fp64 fields only"); }

static void check_box(const Layout& L, const Box& b, int64_t reach, const char* what) {
  if (b.empty()) return;
  HEAT3D_CHECK(b.lo[0] - reach >= -L.gx && b.hi[0] + reach <= L.n[0] + L.gx && b.lo[1] - reach >= -L.gy &&
                   b.hi[1] + reach <= L.n[1] + L.gy && b.lo[2] - reach >= -L.gz && b.hi[2] + reach <= L.n[2] + L.gz,
               what << ": box " << b.str() << (reach ? " with its neighbours" : "") << " outside the layout");
}

static void launch_final(DD* partial, int n, double* out, bool accumulate, const SteadyState* st, hipStream_t s) {
  if (!out) return;
  hipLaunchKernelGGL(steady_final_kernel, dim3(1), dim3(kCgThreads), 0, s, partial, n, out, accumulate ? 1 : 0, st);
  HIPK_CHECK(hipGetLastError());
}

template <bool COND, bool RESID, bool SRC, int SHIFT = 0>
static void launch_apply(const SteadyApplyParams& p, const ApplyGeom& g, int blocks, bool walls, DD* partial,
                         hipStream_t s) {
  const dim3 gr((unsigned)blocks), bl(kCgThreads);
  if (walls) hipLaunchKernelGGL((steady_apply_kernel<COND, RESID, SRC, true, SHIFT>), gr, bl, 0, s, p, g, partial);
  else hipLaunchKernelGGL((steady_apply_kernel<COND, RESID, SRC, false, SHIFT>), gr, bl, 0, s, p, g, partial);
}

void steady_apply(DType t, const SteadyApplyParams& p, void* scratch, double* out, bool accumulate, void* stream) {
  check_f64(t, "steady_apply");
  HEAT3D_CHECK(p.in && p.out && p.in != p.out && scratch, "steady_apply: two distinct fields and the partials");
  HEAT3D_CHECK(!(p.shift && p.residual), "steady_apply: the residual form is not shifted");
  HEAT3D_CHECK(p.shift || !p.cap, "steady_apply: a capacity goes with the shifted form only");
  check_box(p.L, p.box, 1, "steady_apply");
  const Box& b = p.box;
  DD* partial = static_cast<DD*>(scratch);
  int blocks = 0;
  if (!b.empty()) {
    ApplyGeom g;
    g.nzb = (int)((b.extent(2) + 63) / 64);
    g.nyb = (int)((b.extent(1) + kCgWaves - 1) / kCgWaves);
    // x segments: enough tasks to fill the device, never fewer than 8 planes each
    const int64_t tiles = (int64_t)g.nzb * g.nyb;
    int64_t nxs = std::max<int64_t>(1, std::min<int64_t>((kCgMaxBlocks + tiles - 1) / tiles, (b.extent(0) + 7) / 8));
    g.seg = (int)((b.extent(0) + nxs - 1) / nxs);
    g.nxs = (int)((b.extent(0) + g.seg - 1) / g.seg);
    g.ntasks = tiles * g.nxs;
    blocks = (int)std::min<int64_t>(kCgMaxBlocks, g.ntasks);
    bool walls = false;
    for (int a = 0; a < 3; ++a)
      for (int e = 0; e < 2; ++e) walls |= p.wall[a][e] >= b.lo[a] && p.wall[a][e] < b.hi[a];
    const bool src = p.residual && p.src;
    if (p.shift) {
      if (p.cond && p.cap) launch_apply<true, false, false, 2>(p, g, blocks, walls, partial, S(stream));
      else if (p.cond) launch_apply<true, false, false, 1>(p, g, blocks, walls, partial, S(stream));
      else if (p.cap) launch_apply<false, false, false, 2>(p, g, blocks, walls, partial, S(stream));
      else launch_apply<false, false, false, 1>(p, g, blocks, walls, partial, S(stream));
    } else if (p.cond) {
      if (!p.residual) launch_apply<true, false, false>(p, g, blocks, walls, partial, S(stream));
      else if (src) launch_apply<true, true, true>(p, g, blocks, walls, partial, S(stream));
      else launch_apply<true, true, false>(p, g, blocks, walls, partial, S(stream));
    } else {
      if (!p.residual) launch_apply<false, false, false>(p, g, blocks, walls, partial, S(stream));
      else if (src) launch_apply<false, true, true>(p, g, blocks, walls, partial, S(stream));
      else launch_apply<false, true, false>(p, g, blocks, walls, partial, S(stream));
    }
    HIPK_CHECK(hipGetLastError());
  }
  launch_final(partial, blocks, out, accumulate, p.state, S(stream));
}

static int row_blocks(const Box& b) {
  const int64_t rows = b.empty() ? 0 : b.extent(0) * b.extent(1);
  return (int)std::min<int64_t>(kCgMaxBlocks, (rows + kCgWaves - 1) / kCgWaves);
}

void steady_update(DType t, const SteadyUpdateParams& p, void* scratch, double* out, bool accumulate, void* stream) {
  check_f64(t, "steady_update");
  HEAT3D_CHECK((p.x != nullptr) == (p.p != nullptr) && (p.r != nullptr) == (p.q != nullptr) && (p.x || p.r) && scratch,
               "steady_update: four fields (or x and p alone, or r and q alone) and the partials");
  check_box(p.L, p.box, 0, "steady_update");
  DD* partial = static_cast<DD*>(scratch);
  const int blocks = row_blocks(p.box);
  if (blocks > 0) {
    const dim3 gr((unsigned)blocks), bl(kCgThreads);
    if (p.x && p.r) hipLaunchKernelGGL((steady_update_kernel<true, true>), gr, bl, 0, S(stream), p, partial);
    else if (p.r) hipLaunchKernelGGL((steady_update_kernel<false, true>), gr, bl, 0, S(stream), p, partial);
    else hipLaunchKernelGGL((steady_update_kernel<true, false>), gr, bl, 0, S(stream), p, partial);
    HIPK_CHECK(hipGetLastError());
  }
  launch_final(partial, blocks, out, accumulate, p.state, S(stream));
}

void steady_direction(DType t, const SteadyDirectionParams& p, void* stream) {
  check_f64(t, "steady_direction");
  HEAT3D_CHECK(p.p && p.r, "steady_direction: two fields");
  check_box(p.L, p.box, 0, "steady_direction");
  const int blocks = row_blocks(p.box);
  if (blocks == 0) return;
  hipLaunchKernelGGL(steady_direction_kernel, dim3((unsigned)blocks), dim3(kCgThreads), 0, S(stream), p);
  HIPK_CHECK(hipGetLastError());
}

void steady_scalars(SteadyState* st, int phase, void* stream) {
  HEAT3D_CHECK(st, "steady_scalars: the device state");
  hipLaunchKernelGGL(steady_scalars_kernel, dim3(1), dim3(64), 0, S(stream), st, phase);
  HIPK_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace heat3d
