// heat3d-mi355x — the steady solve's three operations on the host: the
// definitions (steady_cg.hpp; the gfx950 kernels are steady_cg.hip).
//
// Rows (i, j) of the box in chunks of kSteadyChunkRows, each chunk worked and
// summed in row order and z order by one thread, the chunks' double-double
// sums combined in chunk order (the shape of cpu::heat_balance): the same bits
// for every thread count.  fp64 fields only.
#include <algorithm>
#include <vector>

#include "kernels.hpp"

namespace heat3d {
namespace cpu {

namespace {

constexpr int64_t kSteadyChunkRows = 64;

inline bool omp_worth(int64_t points) { return points >= (int64_t(1) << 15); }

void check_f64(DType t, const char* what) {
  HEAT3D_CHECK(t == DType::F64, what << ": fp64 fields only");
}

// the box grown by one point along every axis must lie inside the allocation
void check_reach(const Layout& L, const Box& b, const char* what) {
  if (b.empty()) return;
  HEAT3D_CHECK(b.lo[0] - 1 >= -L.gx && b.hi[0] + 1 <= L.n[0] + L.gx && b.lo[1] - 1 >= -L.gy &&
                   b.hi[1] + 1 <= L.n[1] + L.gy && b.lo[2] - 1 >= -L.gz && b.hi[2] + 1 <= L.n[2] + L.gz,
               what << ": box " << b.str() << " with its neighbours outside the layout");
}

void check_inside(const Layout& L, const Box& b, const char* what) {
  if (b.empty()) return;
  HEAT3D_CHECK(b.lo[0] >= -L.gx && b.hi[0] <= L.n[0] + L.gx && b.lo[1] >= -L.gy && b.hi[1] <= L.n[1] + L.gy &&
                   b.lo[2] >= -L.gz && b.hi[2] <= L.n[2] + L.gz,
               what << ": box " << b.str() << " outside the layout");
}

// chunks of rows -> one (hi, lo) pair, set or added
template <typename Chunk>
void reduce_rows(const Box& b, double* out, bool accumulate, Chunk chunk) {
  const int64_t rows = b.empty() ? 0 : b.extent(0) * b.extent(1);
  const int64_t chunks = (rows + kSteadyChunkRows - 1) / kSteadyChunkRows;
  std::vector<DD> part(static_cast<std::size_t>(chunks));
#pragma omp parallel for schedule(static) if (omp_worth(b.volume()))
  for (int64_t ch = 0; ch < chunks; ++ch)
    part[ch] = chunk(ch * kSteadyChunkRows, std::min(rows, (ch + 1) * kSteadyChunkRows));
  DD total{0.0, 0.0};
  for (int64_t ch = 0; ch < chunks; ++ch) total = dd_combine(total, part[ch]);
  if (!out) return;
  if (accumulate) total = dd_combine(DD{out[0], out[1]}, total);
  out[0] = total.hi;
  out[1] = total.lo;
}

// SHIFT: 0 the plain forms, 1 the shifted A-form (implicit_apply), 2 with a capacity
template <bool COND, bool RESID, int SHIFT = 0>
DD apply_chunk(const SteadyApplyParams& p, int64_t r0, int64_t r1) {
  static_assert(!(RESID && SHIFT), "the residual form is not shifted");
  const double* in = static_cast<const double*>(p.in);
  double* out = static_cast<double*>(p.out);
  const double* h = static_cast<const double*>(p.cond);
  const double* S = RESID ? static_cast<const double*>(p.src) : nullptr;
  const double* cap = static_cast<const double*>(p.cap);
  const double mu = p.mu;
  const Layout& L = p.L;
  const Box& b = p.box;
  const int64_t ey = b.extent(1), sx = L.sx, sy = L.sy;
  const double Dx = p.D[0], Dy = p.D[1], Dz = p.D[2], tinf = p.ambient;
  DD acc{0.0, 0.0};
  for (int64_t r = r0; r < r1; ++r) {
    const int64_t i = b.lo[0] + r / ey, j = b.lo[1] + r % ey;
    const bool wxm = i == p.wall[0][0], wxp = i == p.wall[0][1], wym = j == p.wall[1][0], wyp = j == p.wall[1][1];
    for (int64_t k = b.lo[2]; k < b.hi[2]; ++k) {
      const int64_t c = L.index(i, j, k);
      const double T = in[c];
      double xm = in[c - sx], xp = in[c + sx], ym = in[c - sy], yp = in[c + sy], zm = in[c - 1], zp = in[c + 1];
      if (wxm) xm = steady_wall_neighbour<double>(p.kind[0][0], RESID, T, xm, p.beta[0][0], tinf);
      if (wxp) xp = steady_wall_neighbour<double>(p.kind[0][1], RESID, T, xp, p.beta[0][1], tinf);
      if (wym) ym = steady_wall_neighbour<double>(p.kind[1][0], RESID, T, ym, p.beta[1][0], tinf);
      if (wyp) yp = steady_wall_neighbour<double>(p.kind[1][1], RESID, T, yp, p.beta[1][1], tinf);
      if (k == p.wall[2][0]) zm = steady_wall_neighbour<double>(p.kind[2][0], RESID, T, zm, p.beta[2][0], tinf);
      if (k == p.wall[2][1]) zp = steady_wall_neighbour<double>(p.kind[2][1], RESID, T, zp, p.beta[2][1], tinf);
      double inc;
      if constexpr (COND)
        inc = steady_increment_var<double>(T, xm, xp, ym, yp, zm, zp, h[c], h[c - sx], h[c + sx], h[c - sy],
                                           h[c + sy], h[c - 1], h[c + 1], Dx, Dy, Dz);
      else
        inc = steady_increment<double>(T, xm, xp, ym, yp, zm, zp, Dx, Dy, Dz);
      double v;
      if constexpr (RESID) v = S ? add_source<double>(inc, S[c]) : inc;
      else if constexpr (SHIFT == 2) v = implicit_apply<true, double>(T, inc, mu, cap[c]);
      else if constexpr (SHIFT == 1) v = implicit_apply<false, double>(T, inc, mu, 0.0);
      else v = -inc;
      out[c] = v;
      dd_add(acc, RESID ? v * v : T * v);
    }
  }
  return acc;
}

}  // namespace

void steady_apply(DType t, const SteadyApplyParams& p, double* out, bool accumulate) {
  check_f64(t, "steady_apply");
  HEAT3D_CHECK(p.in && p.out && p.in != p.out, "steady_apply: two distinct fields");
  check_reach(p.L, p.box, "steady_apply");
  if (p.state && p.state->done) return;
  HEAT3D_CHECK(!(p.shift && p.residual), "steady_apply: the residual form is not shifted");
  HEAT3D_CHECK(p.shift || !p.cap, "steady_apply: a capacity goes with the shifted form only");
  auto run = [&](auto chunk) { reduce_rows(p.box, out, accumulate, chunk); };
  if (p.shift && p.cond && p.cap) run([&](int64_t a, int64_t b) { return apply_chunk<true, false, 2>(p, a, b); });
  else if (p.shift && p.cond) run([&](int64_t a, int64_t b) { return apply_chunk<true, false, 1>(p, a, b); });
  else if (p.shift && p.cap) run([&](int64_t a, int64_t b) { return apply_chunk<false, false, 2>(p, a, b); });
  else if (p.shift) run([&](int64_t a, int64_t b) { return apply_chunk<false, false, 1>(p, a, b); });
  else if (p.cond && p.residual) run([&](int64_t a, int64_t b) { return apply_chunk<true, true>(p, a, b); });
  else if (p.cond) run([&](int64_t a, int64_t b) { return apply_chunk<true, false>(p, a, b); });
  else if (p.residual) run([&](int64_t a, int64_t b) { return apply_chunk<false, true>(p, a, b); });
  else run([&](int64_t a, int64_t b) { return apply_chunk<false, false>(p, a, b); });
}

void steady_update(DType t, const SteadyUpdateParams& p, double* out, bool accumulate) {
  check_f64(t, "steady_update");
  HEAT3D_CHECK((p.x != nullptr) == (p.p != nullptr) && (p.r != nullptr) == (p.q != nullptr) && (p.x || p.r),
               "steady_update: four fields, or x and p alone, or r and q alone");
  check_inside(p.L, p.box, "steady_update");
  if (p.state && p.state->done) return;
  const double alpha = p.state ? p.state->alpha : p.alpha;
  double* x = static_cast<double*>(p.x);
  double* r = static_cast<double*>(p.r);
  const double* d = static_cast<const double*>(p.p);
  const double* q = static_cast<const double*>(p.q);
  const Layout& L = p.L;
  const Box& b = p.box;
  const int64_t ey = b.extent(1);
  reduce_rows(b, out, accumulate, [&](int64_t r0, int64_t r1) {
    DD acc{0.0, 0.0};
    for (int64_t row = r0; row < r1; ++row) {
      const int64_t base = L.index(b.lo[0] + row / ey, b.lo[1] + row % ey, 0);
      for (int64_t k = b.lo[2]; k < b.hi[2]; ++k) {
        if (x) x[base + k] = steady_axpy<double>(alpha, d[base + k], x[base + k]);
        if (!r) continue;
        const double rn = steady_axpy<double>(-alpha, q[base + k], r[base + k]);
        r[base + k] = rn;
        dd_add(acc, rn * rn);
      }
    }
    return acc;
  });
}

void steady_direction(DType t, const SteadyDirectionParams& p) {
  check_f64(t, "steady_direction");
  HEAT3D_CHECK(p.p && p.r, "steady_direction: two fields");
  check_inside(p.L, p.box, "steady_direction");
  if (p.state && p.state->done) return;
  const double beta = p.state ? p.state->beta : p.beta;
  double* d = static_cast<double*>(p.p);
  const double* r = static_cast<const double*>(p.r);
  const Layout& L = p.L;
  const Box& b = p.box;
  const int64_t ey = b.extent(1);
  const int64_t rows = b.empty() ? 0 : b.extent(0) * ey;
  const bool copy = p.copy;
#pragma omp parallel for schedule(static) if (omp_worth(b.volume()))
  for (int64_t row = 0; row < rows; ++row) {
    const int64_t base = L.index(b.lo[0] + row / ey, b.lo[1] + row % ey, 0);
    for (int64_t k = b.lo[2]; k < b.hi[2]; ++k)
      d[base + k] = copy ? r[base + k] : steady_axpy<double>(beta, d[base + k], r[base + k]);
  }
}

}  // namespace cpu
}  // namespace heat3d
