// heat3d-mi355x — the heat balance on gfx950 (heat_balance.hpp; the definition
// is cpu::heat_balance, kernels_cpu.cpp).
//
// One pass over the box.  A wave owns whole z rows (row = wave, wave + waves of
// the grid, ...) and reads them in 16-byte pieces per lane from the aligned
// start below the box (the elements outside [lo, hi) are masked, and lie inside
// the row's pitch); four pieces are loaded ahead of the arithmetic.  The source
// the conductivity and the heat capacity are template arguments: the plain form
// reads one field.
// Face terms are formed on wall-adjacent rows only: the x and y faces under
// wave-uniform branches (the neighbour row is one more vector load), the two
// z faces of a row by lanes 0 and 1 after the row.  Every lane keeps eight
// double-double accumulators (constant indices throughout: registers, no
// scratch memory); a wave combines them by shuffles, a block through one LDS
// stage, and a single-block kernel combines the blocks' partials in a fixed
// order.  No atomics: the same call gives the same bits.
//
// Wall vertices of insulated and convective faces are never read from T (K-step
// sweeps leave those planes stale); Ch is read there (it is static).
#include "hip_helpers.hpp"

namespace heat3d {
namespace hip {

constexpr int kBalBlocks = 2048;   // 8 blocks of 256 threads per CU
constexpr int kBalThreads = 256;
constexpr int kBalAhead = 4;       // row pieces loaded before the arithmetic

std::size_t balance_scratch_bytes() { return sizeof(BalanceSums) * kBalBlocks; }

template <typename Real>
struct KeyOf;
template <> struct KeyOf<double> { typedef long long type; };
template <> struct KeyOf<float> { typedef int type; };

// per-lane state
template <typename Real>
struct LaneSums {
  DD acc[kBalanceSums];
  typename KeyOf<Real>::type kmin, kmax;
  unsigned bad;
};

__device__ __forceinline__ DD dd_shfl_down(const DD& a, int o) {
  DD b;
  b.hi = __shfl_down(a.hi, o, 64);
  b.lo = __shfl_down(a.lo, o, 64);
  return b;
}

// lane 0 of each wave <- the wave's sums; thread 0 <- the block's (waves in order)
__device__ __forceinline__ void block_combine(BalanceSums& mine, BalanceSums* red) {
#pragma unroll
  for (int q = 0; q < kBalanceSums; ++q) {
    DD a{mine.hi[q], mine.lo[q]};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = dd_combine(a, dd_shfl_down(a, o));
    mine.hi[q] = a.hi;
    mine.lo[q] = a.lo;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long n = __shfl_down(mine.kmin, o, 64), x = __shfl_down(mine.kmax, o, 64);
    mine.kmin = n < mine.kmin ? n : mine.kmin;
    mine.kmax = x > mine.kmax ? x : mine.kmax;
    mine.nonfinite += __shfl_down(mine.nonfinite, o, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    mine = red[0];
    for (int w = 1; w < kBalThreads / 64; ++w) bal_merge(mine, red[w]);
  }
}

// the terms of face F of one loaded piece: nb = the neighbour row's piece
// (Dirichlet), hn = Ch there
template <typename Real, int V, bool COND, int F>
__device__ __forceinline__ void face_piece(LaneSums<Real>& s, const BalanceParams& p, const Real* T, const Real* Ch,
                                           int64_t at, int64_t off, const Real (&c)[V], const bool (&ok)[V]) {
  typedef typename VecOf<Real, V>::type Vec;
  const int kind = p.kind[F / 2][F % 2];
  if (kind == kWallInsulated) return;  // the neighbour is the centre: no flow, exactly
  Real n[V], w[V];
  if (kind == kWallDirichlet) {
    const Vec nb = *reinterpret_cast<const Vec*>(T + at + off);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if constexpr (V == 1) n[v] = nb;
      else n[v] = nb[v];
    }
  } else {
    const Real beta = static_cast<Real>(p.beta[F / 2][F % 2]), tinf = static_cast<Real>(p.ambient);
#pragma unroll
    for (int v = 0; v < V; ++v) n[v] = convective_ghost<Real>(c[v], beta, tinf);
  }
  if constexpr (COND) {
    const Vec hc = *reinterpret_cast<const Vec*>(Ch + at);
    const Vec hn = *reinterpret_cast<const Vec*>(Ch + at + off);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if constexpr (V == 1) w[v] = hc + hn;
      else w[v] = hc[v] + hn[v];
    }
  }
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const double d = static_cast<double>(n[v]) - static_cast<double>(c[v]);
    double term = d;
    if constexpr (COND) term = static_cast<double>(w[v]) * d;
    dd_add(s.acc[2 + F], ok[v] ? term : 0.0);
  }
}

// one z face of a row, by one lane: the point at idx
template <typename Real, bool COND, int F>
__device__ __forceinline__ void face_point(LaneSums<Real>& s, const BalanceParams& p, const Real* T, const Real* Ch,
                                           int64_t idx) {
  const int kind = p.kind[2][F % 2];
  if (kind == kWallInsulated) return;
  const int64_t q = idx + (F % 2 ? 1 : -1);
  const Real c = T[idx];
  const Real n = kind == kWallDirichlet
                     ? T[q]
                     : convective_ghost<Real>(c, static_cast<Real>(p.beta[2][F % 2]), static_cast<Real>(p.ambient));
  const double d = static_cast<double>(n) - static_cast<double>(c);
  double term = d;
  if constexpr (COND) {
    const Real w = Ch[idx] + Ch[q];
    term = static_cast<double>(w) * d;
  }
  dd_add(s.acc[2 + F], term);
}

template <typename Real, int V, bool SRC, bool COND, bool CAP>
__global__ __launch_bounds__(kBalThreads) void balance_partial_kernel(BalanceParams p, BalanceSums* partial) {
  typedef typename VecOf<Real, V>::type Vec;
  typedef typename KeyOf<Real>::type Key;
  constexpr Key kNone = sizeof(Real) == 8 ? (Key)kBalKeyNone : (Key)0x7fffffff;
  __shared__ BalanceSums red[kBalThreads / 64];
  const Real* T = static_cast<const Real*>(p.field);
  const Real* S = static_cast<const Real*>(p.src);
  const Real* Ch = static_cast<const Real*>(p.cond);
  [[maybe_unused]] const Real* Cs = static_cast<const Real*>(p.cap);
  const Layout& L = p.L;
  const Box& b = p.box;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t ey = b.extent(1);
  const int64_t rows = b.extent(2) > 0 ? b.extent(0) * ey : 0;
  const int64_t lo = b.lo[2], hi = b.hi[2];
  // the first piece starts at the multiple of V at or below lo (row starts are
  // multiples of 16 elements of an aligned allocation)
  const int64_t kb = lo - ((lo % V + V) % V);
  LaneSums<Real> s;
#pragma unroll
  for (int q = 0; q < kBalanceSums; ++q) s.acc[q] = DD{0.0, 0.0};
  s.kmin = kNone;
  s.kmax = ~kNone;
  s.bad = 0;
  for (int64_t row = (int64_t)blockIdx.x * (kBalThreads / 64) + wave; row < rows;
       row += (int64_t)gridDim.x * (kBalThreads / 64)) {
    const int64_t i = b.lo[0] + row / ey, j = b.lo[1] + row % ey;
    const int64_t base = L.index(i, j, 0);
    // wave-uniform: is this row next to an x or y wall?
    const bool xm = i == p.wall[0][0], xp = i == p.wall[0][1], ym = j == p.wall[1][0], yp = j == p.wall[1][1];
    const bool faces = xm | xp | ym | yp;
    for (int64_t k0 = kb + (int64_t)lane * V; k0 < hi; k0 += (int64_t)64 * V * kBalAhead) {
      Vec t[kBalAhead], q[kBalAhead];
      [[maybe_unused]] Vec sc[kBalAhead];
#pragma unroll
      for (int u = 0; u < kBalAhead; ++u) {
        const int64_t k = k0 + (int64_t)u * 64 * V;
        if (k < hi) {
          t[u] = *reinterpret_cast<const Vec*>(T + base + k);
          if constexpr (SRC) q[u] = *reinterpret_cast<const Vec*>(S + base + k);
          if constexpr (CAP) sc[u] = *reinterpret_cast<const Vec*>(Cs + base + k);
        }
      }
#pragma unroll
      for (int u = 0; u < kBalAhead; ++u) {
        const int64_t k = k0 + (int64_t)u * 64 * V;
        if (k >= hi) break;
        Real c[V];
        bool ok[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
          ok[v] = k + v >= lo && k + v < hi;
          Real tv, qv = Real(0);
          if constexpr (V == 1) tv = t[u];
          else tv = t[u][v];
          if constexpr (SRC) {
            if constexpr (V == 1) qv = q[u];
            else qv = q[u][v];
          }
          c[v] = ok[v] ? tv : Real(0);
          if constexpr (CAP) {
            // stored heat rc T = T / s, the quotient in double (s = 1 outside the box)
            Real sv;
            if constexpr (V == 1) sv = sc[u];
            else sv = sc[u][v];
            dd_add(s.acc[0], static_cast<double>(c[v]) / static_cast<double>(ok[v] ? sv : Real(1)));
          } else {
            dd_add(s.acc[0], static_cast<double>(c[v]));
          }
          s.bad += bal_nonfinite(c[v]) ? 1u : 0u;
          const Key key = bal_key(c[v]);
          const bool num = ok[v] && c[v] == c[v];
          s.kmin = num && key < s.kmin ? key : s.kmin;
          s.kmax = num && key > s.kmax ? key : s.kmax;
          if constexpr (SRC) dd_add(s.acc[1], static_cast<double>(ok[v] ? qv : Real(0)));
        }
        if (faces) {
          if (xm) face_piece<Real, V, COND, 0>(s, p, T, Ch, base + k, -L.sx, c, ok);
          if (xp) face_piece<Real, V, COND, 1>(s, p, T, Ch, base + k, L.sx, c, ok);
          if (ym) face_piece<Real, V, COND, 2>(s, p, T, Ch, base + k, -L.sy, c, ok);
          if (yp) face_piece<Real, V, COND, 3>(s, p, T, Ch, base + k, L.sy, c, ok);
        }
      }
    }
    // the row's two z faces: lane 0 the low one, lane 1 the high one
    if (lane == 0 && p.wall[2][0] >= lo && p.wall[2][0] < hi)
      face_point<Real, COND, 4>(s, p, T, Ch, base + p.wall[2][0]);
    if (lane == 1 && p.wall[2][1] >= lo && p.wall[2][1] < hi)
      face_point<Real, COND, 5>(s, p, T, Ch, base + p.wall[2][1]);
  }
  BalanceSums mine;
#pragma unroll
  for (int q = 0; q < kBalanceSums; ++q) mine.hi[q] = s.acc[q].hi, mine.lo[q] = s.acc[q].lo;
  mine.kmin = s.kmin == kNone ? kBalKeyNone : bal_key(static_cast<double>(bal_unkey(s.kmin)));
  mine.kmax = s.kmax == (Key)~kNone ? ~kBalKeyNone : bal_key(static_cast<double>(bal_unkey(s.kmax)));
  mine.nonfinite = s.bad;
  block_combine(mine, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = mine;
}

// one block: thread t combines partials t, t + 256, ... in order, then the block
__global__ __launch_bounds__(kBalThreads) void balance_final_kernel(const BalanceSums* partial, int n, BalanceSums* out,
                                                                    int accumulate) {
  __shared__ BalanceSums red[kBalThreads / 64];
  BalanceSums mine;
  bal_clear(mine);
  for (int q = threadIdx.x; q < n; q += kBalThreads) bal_merge(mine, partial[q]);
  block_combine(mine, red);
  if (threadIdx.x == 0) {
    if (accumulate) {
      BalanceSums total = *out;
      bal_merge(total, mine);
      *out = total;
    } else {
      *out = mine;
    }
  }
}

template <typename Real, int V, bool CAP>
static void launch_partial_cap(const BalanceParams& p, int blocks, BalanceSums* partial, hipStream_t q) {
  const dim3 g((unsigned)blocks), b(kBalThreads);
  if (p.src && p.cond) hipLaunchKernelGGL((balance_partial_kernel<Real, V, true, true, CAP>), g, b, 0, q, p, partial);
  else if (p.src) hipLaunchKernelGGL((balance_partial_kernel<Real, V, true, false, CAP>), g, b, 0, q, p, partial);
  else if (p.cond) hipLaunchKernelGGL((balance_partial_kernel<Real, V, false, true, CAP>), g, b, 0, q, p, partial);
  else hipLaunchKernelGGL((balance_partial_kernel<Real, V, false, false, CAP>), g, b, 0, q, p, partial);
}

template <typename Real, int V>
static void launch_partial(const BalanceParams& p, int blocks, BalanceSums* partial, hipStream_t q) {
  if (p.cap) launch_partial_cap<Real, V, true>(p, blocks, partial, q);
  else launch_partial_cap<Real, V, false>(p, blocks, partial, q);
}

void heat_balance(DType t, const BalanceParams& p, void* scratch, BalanceSums* out, bool accumulate, void* stream) {
  HEAT3D_CHECK(p.field && scratch && out, "heat_balance: field, scratch and result pointers");
  const Box& b = p.box;
  HEAT3D_CHECK(b.empty() || (b.lo[0] >= -p.L.gx && b.hi[0] <= p.L.n[0] + p.L.gx && b.lo[1] >= -p.L.gy &&
                             b.hi[1] <= p.L.n[1] + p.L.gy && b.lo[2] >= -p.L.gz && b.hi[2] <= p.L.n[2] + p.L.gz),
               "heat_balance: box " << b.str() << " outside the layout");
  const int64_t rows = b.empty() ? 0 : b.extent(0) * b.extent(1);
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(kBalBlocks, (rows + 3) / 4));
  BalanceSums* partial = static_cast<BalanceSums*>(scratch);
  // 16-byte pieces need 16-byte aligned fields (rows start at multiples of 16 elements)
  const auto al = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; };
  const bool wide = al(p.field) && al(p.src) && al(p.cond) && al(p.cap);
  if (t == DType::F64) {
    if (wide) launch_partial<double, 2>(p, blocks, partial, S(stream));
    else launch_partial<double, 1>(p, blocks, partial, S(stream));
  } else {
    if (wide) launch_partial<float, 4>(p, blocks, partial, S(stream));
    else launch_partial<float, 1>(p, blocks, partial, S(stream));
  }
  HIPK_CHECK(hipGetLastError());
  hipLaunchKernelGGL(balance_final_kernel, dim3(1), dim3(kBalThreads), 0, S(stream), partial, blocks, out,
                     accumulate ? 1 : 0);
  HIPK_CHECK(hipGetLastError());
}

}  // namespace hip
}  // namespace heat3d
