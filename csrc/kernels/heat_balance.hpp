// heat3d-mi355x — the heat balance of a subdomain: types and the arithmetic
// that cpu::heat_balance (kernels_cpu.cpp, the definition) and the gfx950
// kernel (heat_balance.hip) share.
//
// Over the updated points U of a box (docs/ARCHITECTURE.md "Heat balance"):
//   sum 0      Σ T                      (stored heat / (hx hy hz); with a heat
//              capacity Σ T / s, s = dtype(1 / rc), each term double(T) / double(s))
//   sum 1      Σ S                      (source power * dt / (hx hy hz))
//   sum 2 + f  Σ w (n - c) over the points whose neighbour across face f is a
//              wall vertex (flow / (alpha h_b h_c / h_a))
// every term a float64 formed from the stored values widened exactly, every sum
// accumulated in double-double (TwoSum per term, renormalised when partials
// are combined), plus min / max over the non-NaN values and the count of
// NaN / Inf values.  The caller scales.
#pragma once

#include <cstdint>

#include "../core/common.hpp"
#include "layout.hpp"

namespace heat3d {

constexpr int kBalanceSums = 8;  // heat, source, six faces

// A face of the global grid as the box sees it
enum BalanceWall : int { kWallDirichlet = 0, kWallInsulated = 1, kWallConvective = 2 };
constexpr int64_t kNoBalanceWall = -(int64_t(1) << 40);  // = kNoWall

struct BalanceParams {
  const void* field = nullptr;  // T
  const void* src = nullptr;    // S = dtype(dt q) in the same Layout, or nullptr
  const void* cond = nullptr;   // Ch = dtype(0.5 c) in the same Layout, or nullptr
  const void* cap = nullptr;    // s = dtype(1 / rc) in the same Layout, or nullptr
  Layout L;
  Box box;  // local coordinates of the updated points to sum (inside the owned block)
  // local coordinate along axis a of the updated plane next to the low / high
  // wall of the global grid (global index 1 / N - 2), kNoBalanceWall where that
  // plane is not in the box; what the wall is, and a convective wall's coefficient
  int64_t wall[3][2] = {{kNoBalanceWall, kNoBalanceWall}, {kNoBalanceWall, kNoBalanceWall},
                        {kNoBalanceWall, kNoBalanceWall}};
  int kind[3][2] = {{0, 0}, {0, 0}, {0, 0}};
  double beta[3][2] = {{0, 0}, {0, 0}, {0, 0}};
  double ambient = 0;
};

// The raw result: (hi, lo) pairs with hi = fl(hi + lo), min / max as ordered
// integer keys of the float64 values (bal_key; no value: the initial keys, NaN
// patterns), the count of non-finite values.  Lives in device memory on HIP.
struct BalanceSums {
  double hi[kBalanceSums];
  double lo[kBalanceSums];
  long long kmin, kmax;
  unsigned long long nonfinite;
};

// ---- double-double ------------------------------------------------------------
struct DD {
  double hi, lo;
};
// acc += x: TwoSum of the leading parts, the error into the tail
H3D_HD inline void dd_add(DD& a, double x) {
  const double s = a.hi + x;
  const double bb = s - a.hi;
  const double e = (a.hi - (s - bb)) + (x - bb);
  a.hi = s;
  a.lo += e;
}
// a + b, renormalised (hi = fl(hi + lo))
H3D_HD inline DD dd_combine(const DD& a, const DD& b) {
  const double s = a.hi + b.hi;
  const double bb = s - a.hi;
  double e = (a.hi - (s - bb)) + (b.hi - bb);
  e += a.lo + b.lo;
  DD r;
  r.hi = s + e;
  const double cc = r.hi - s;
  r.lo = (s - (r.hi - cc)) + (e - cc);
  return r;
}

// ---- ordered keys: k(a) < k(b) <=> a < b, with -0 < +0 -------------------------
H3D_HD inline long long bal_key(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  return b ^ ((b >> 63) & 0x7fffffffffffffffLL);
}
H3D_HD inline double bal_unkey(long long k) {
  return __builtin_bit_cast(double, k ^ ((k >> 63) & 0x7fffffffffffffffLL));
}
H3D_HD inline int bal_key(float v) {
  const int b = __builtin_bit_cast(int, v);
  return b ^ ((b >> 31) & 0x7fffffff);
}
H3D_HD inline float bal_unkey(int k) { return __builtin_bit_cast(float, k ^ ((k >> 31) & 0x7fffffff)); }
constexpr long long kBalKeyNone = 0x7fffffffffffffffLL;  // min starts here, max at ~it

H3D_HD inline bool bal_nonfinite(double v) {
  return (__builtin_bit_cast(unsigned long long, v) & 0x7ff0000000000000ULL) == 0x7ff0000000000000ULL;
}
H3D_HD inline bool bal_nonfinite(float v) { return (__builtin_bit_cast(unsigned, v) & 0x7f800000u) == 0x7f800000u; }

H3D_HD inline void bal_clear(BalanceSums& s) {
  for (int q = 0; q < kBalanceSums; ++q) s.hi[q] = s.lo[q] = 0.0;
  s.kmin = kBalKeyNone;
  s.kmax = ~kBalKeyNone;
  s.nonfinite = 0;
}
// a <- a + b
H3D_HD inline void bal_merge(BalanceSums& a, const BalanceSums& b) {
  for (int q = 0; q < kBalanceSums; ++q) {
    const DD r = dd_combine(DD{a.hi[q], a.lo[q]}, DD{b.hi[q], b.lo[q]});
    a.hi[q] = r.hi;
    a.lo[q] = r.lo;
  }
  a.kmin = b.kmin < a.kmin ? b.kmin : a.kmin;
  a.kmax = b.kmax > a.kmax ? b.kmax : a.kmax;
  a.nonfinite += b.nonfinite;
}

}  // namespace heat3d
