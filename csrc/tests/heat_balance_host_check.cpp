// heat3d-mi355x — stand-alone host check of cpu::heat_balance, meant for a
// sanitizer build (no Python, no GPU):
//
//   g++ -std=c++17 -O1 -g -fopenmp -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -Icsrc csrc/tests/heat_balance_host_check.cpp csrc/kernels/kernels_cpu.cpp csrc/kernels/cpu_rows.cpp \
//       csrc/kernels/cpu_rows_fma.cpp csrc/core/config.cpp -o heat_balance_host_check && ./heat_balance_host_check
//   (cpu_rows_fma.cpp with -mfma -mavx2)
//
// The three boxes of the tests (z extents below a wave, a wave plus a tail, a
// block plus an odd tail), ghost depth 1 and 4, both dtypes, the four material
// cases, a wall of each kind on every axis.  Every field is an allocation of
// exactly Layout::bytes(), so a read outside it is a sanitizer report; the sums
// are compared with plain long double sums.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../kernels/kernels.hpp"

using namespace heat3d;

static double rnd(unsigned long long& s) {
  s = s * 6364136223846793005ULL + 1442695040888963407ULL;
  return (double)(s >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

template <typename Real>
static int run(const int64_t n[3], int64_t depth, bool with_src, bool with_cond) {
  const Layout L = Layout::make(n, sizeof(Real), depth, depth, depth);
  std::vector<Real*> bufs;
  auto field = [&](double lo, double hi, unsigned long long seed) {
    Real* p = static_cast<Real*>(std::malloc(L.bytes()));
    for (int64_t q = 0; q < L.elems; ++q) p[q] = (Real)(lo + (hi - lo) * 0.5 * (rnd(seed) + 1.0));
    bufs.push_back(p);
    return p;
  };
  BalanceParams p;
  p.field = field(-1, 1, 1);
  p.src = with_src ? field(-1e-3, 1e-3, 2) : nullptr;
  p.cond = with_cond ? field(0.125, 0.5, 3) : nullptr;
  p.L = L;
  for (int a = 0; a < 3; ++a) {
    p.box.lo[a] = 0;
    p.box.hi[a] = n[a];
    p.wall[a][0] = 0;
    p.wall[a][1] = n[a] - 1;
  }
  // x- convective, x+ insulated, y- Dirichlet, y+ convective, z- insulated, z+ Dirichlet
  const int kind[6] = {kWallConvective, kWallInsulated, kWallDirichlet, kWallConvective, kWallInsulated, kWallDirichlet};
  const double beta[6] = {0.5, 0, 0, 0.3, 0, 0};
  for (int f = 0; f < 6; ++f) p.kind[f / 2][f % 2] = kind[f], p.beta[f / 2][f % 2] = beta[f];
  p.ambient = 1.75;
  const DType t = sizeof(Real) == 8 ? DType::F64 : DType::F32;
  BalanceSums s, twice;
  cpu::heat_balance(t, p, &s, false);
  twice = s;
  cpu::heat_balance(t, p, &twice, true);  // accumulate: every sum doubles
  long double heat = 0, src = 0, zp = 0;
  const Real* T = static_cast<const Real*>(p.field);
  const Real* S = static_cast<const Real*>(p.src);
  const Real* C = static_cast<const Real*>(p.cond);
  for (int64_t i = 0; i < n[0]; ++i)
    for (int64_t j = 0; j < n[1]; ++j)
      for (int64_t k = 0; k < n[2]; ++k) {
        const int64_t q = L.index(i, j, k);
        heat += T[q];
        if (S) src += S[q];
        if (k == n[2] - 1) {
          const double w = C ? (double)(Real)(C[q] + C[q + 1]) : 1.0;
          zp += (long double)(w * ((double)T[q + 1] - (double)T[q]));
        }
      }
  int bad = 0;
  auto near = [&](double got, long double want, const char* what) {
    if (std::fabs((double)((long double)got - want)) > 1e-9 * (1.0 + std::fabs((double)want))) {
      std::printf("MISMATCH %s: got %.17g want %.17Lg\n", what, got, want);
      ++bad;
    }
  };
  near(s.hi[0] + s.lo[0], heat, "heat");
  near(s.hi[1] + s.lo[1], src, "source");
  near(s.hi[7] + s.lo[7], zp, "flow z+");
  near(twice.hi[0] + twice.lo[0], 2 * heat, "heat twice");
  if (s.hi[3] != 0.0 || s.hi[6] != 0.0 || s.nonfinite != 0) ++bad, std::printf("MISMATCH insulated / nonfinite\n");
  for (Real* b : bufs) std::free(b);
  return bad;
}

int main() {
  const int64_t boxes[3][3] = {{7, 6, 5}, {9, 8, 70}, {6, 7, 261}};
  int bad = 0, cases = 0;
  for (int threads : {1, 3}) {
    cpu::set_threads(threads);
    for (auto& n : boxes)
      for (int64_t depth : {1, 4})
        for (int m = 0; m < 4; ++m) {
          bad += run<double>(n, depth, m & 1, m & 2);
          bad += run<float>(n, depth, m & 1, m & 2);
          cases += 2;
        }
  }
  std::printf("heat_balance host check: %d cases, %d mismatches\n", cases, bad);
  return bad ? 1 : 0;
}
