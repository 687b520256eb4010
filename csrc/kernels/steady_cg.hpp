// heat3d-mi355x — the direct steady-state solve (conjugate gradients): types
// and the scalar logic that the cpu:: definitions (steady_cg_cpu.cpp) and the
// gfx950 kernels (steady_cg.hip) share.  docs/ARCHITECTURE.md "Steady solve".
//
// One time step G of the current mode defines the system: r(T) = G(T) - T =
// b - A T over the updated points.  A p is the negated increment of the
// homogeneous step (wall vertices 0, ambient 0, no source); the pointwise
// arithmetic is steady_increment / steady_increment_var in kernels.hpp.
// Dot products: every term a float64 product, summed in double-double
// (heat_balance.hpp) on a fixed reduction shape, no atomics.  fp64 fields only.
#pragma once

#include <cstdint>

#include "../core/common.hpp"
#include "heat_balance.hpp"
#include "layout.hpp"

namespace heat3d {

// The scalars of a solve, in device memory on HIP.  The reduction kernels
// write the (hi, lo) pairs; steady_scalars turns them into alpha, beta, the
// squared norms and the stop flag.  Kernels given a state return at once when
// done is set.
struct SteadyState {
  double pq[2];   // p . A p of this iteration (hi, lo)
  double rrn[2];  // r . r after this iteration's update (hi, lo)
  double rr;      // r . r the current direction was built from
  double rr0;     // r . r of the initial residual (< 0: not set yet)
  double alpha, beta;
  double tol2;    // tol^2
  long long iter, max_iter;
  int done;       // set: every later kernel of the stream is a no-op
  int status;     // SteadyStatus
};
enum SteadyStatus : int { kSteadyRunning = 0, kSteadyConverged = 1, kSteadyMaxIter = 2, kSteadyBreakdown = 3 };
enum SteadyPhase : int { kSteadyInit = 0, kSteadyAlpha = 1, kSteadyBeta = 2 };

// The scalar step at a launch boundary (one thread on the GPU, the same code
// on the CPU), after the reduction (and the processes' all-reduce) it consumes.
//   Init:  rr <- rrn (rr0 too, the first time); beta <- 0; already within tol: done
//   Alpha: alpha <- rr / pq; pq not positive and finite: breakdown
//   Beta:  iter + 1; beta <- rrn / rr; rr <- rrn; rr <= tol^2 rr0: converged;
//          iter = max_iter: stopped
H3D_HD inline void steady_scalars_step(SteadyState* s, int phase) {
  if (phase == kSteadyInit) {
    const double rr = s->rrn[0] + s->rrn[1];
    s->rr = rr;
    if (s->rr0 < 0.0) s->rr0 = rr;
    s->beta = 0.0;
    s->alpha = 0.0;
    if (!(rr == rr) || rr > 1.7976931348623157e308) {
      s->done = 1;
      s->status = kSteadyBreakdown;
    } else if (rr <= s->tol2 * s->rr0) {
      s->done = 1;
      s->status = kSteadyConverged;
    } else if (s->iter >= s->max_iter) {
      s->done = 1;
      s->status = kSteadyMaxIter;
    }
    return;
  }
  if (s->done) return;
  if (phase == kSteadyAlpha) {
    const double pq = s->pq[0] + s->pq[1];
    if (!(pq > 0.0) || pq > 1.7976931348623157e308) {
      s->done = 1;
      s->status = kSteadyBreakdown;
      return;
    }
    s->alpha = s->rr / pq;
    return;
  }
  const double rn = s->rrn[0] + s->rrn[1];
  s->iter = s->iter + 1;
  if (!(rn == rn) || rn > 1.7976931348623157e308) {
    s->rr = rn;
    s->done = 1;
    s->status = kSteadyBreakdown;
    return;
  }
  s->beta = rn / s->rr;
  s->rr = rn;
  if (rn <= s->tol2 * s->rr0) {
    s->done = 1;
    s->status = kSteadyConverged;
  } else if (s->iter >= s->max_iter) {
    s->done = 1;
    s->status = kSteadyMaxIter;
  }
}

// out = A in (residual false) or out = b - A in (residual true) over a box,
// fused with a dot product: in . out, or out . out.
struct SteadyApplyParams {
  const void* in = nullptr;    // p, or the field T
  void* out = nullptr;         // q, or r; same Layout
  const void* cond = nullptr;  // Ch = 0.5 c in the same Layout, or nullptr
  const void* src = nullptr;   // S = dt q in the same Layout, or nullptr (read by the residual form only)
  Layout L;
  Box box;  // updated points, local coordinates; box grown by one point lies inside the Layout
  double D[3] = {0, 0, 0};
  // as BalanceParams: local coordinate of the updated plane next to each wall
  // of the global grid (kNoBalanceWall: not in reach), what the wall is, and a
  // convective wall's coefficient.  The neighbour across a wall: Dirichlet the
  // stored wall value (residual) or 0 (A); insulated the centre value;
  // convective convective_ghost(c, beta, ambient) (residual) or (c, beta, 0) (A).
  int64_t wall[3][2] = {{kNoBalanceWall, kNoBalanceWall}, {kNoBalanceWall, kNoBalanceWall},
                        {kNoBalanceWall, kNoBalanceWall}};
  int kind[3][2] = {{0, 0}, {0, 0}, {0, 0}};
  double beta[3][2] = {{0, 0}, {0, 0}, {0, 0}};
  double ambient = 0;
  bool residual = false;
  const SteadyState* state = nullptr;  // its done flag is honoured (nullptr: always runs)
  // The shifted A-form of an implicit step (docs/ARCHITECTURE.md "Implicit
  // steps"): out = (R + mu A) in, R = diag(1 / s) with s = `cap` in the same
  // Layout (read at the centre of an updated point only), R = I when cap is
  // nullptr; the dot product is in . out.  Not with the residual form.
  bool shift = false;
  double mu = 0;
  const void* cap = nullptr;
};

// x += alpha p, r -= alpha q over a box, fused with r . r of the new r.  With
// x and p both nullptr only r is updated (alpha = 1: r -= q, the true residual
// of an implicit step); with r and q both nullptr only x (the sum is 0).
struct SteadyUpdateParams {
  void* x = nullptr;
  const void* p = nullptr;
  void* r = nullptr;
  const void* q = nullptr;
  Layout L;
  Box box;
  double alpha = 0;                    // used when state is nullptr
  const SteadyState* state = nullptr;  // alpha = state->alpha, done honoured
};

// p = r + beta p over a box (copy: p = r, whatever p holds)
struct SteadyDirectionParams {
  void* p = nullptr;
  const void* r = nullptr;
  Layout L;
  Box box;
  double beta = 0;
  bool copy = false;
  const SteadyState* state = nullptr;  // beta = state->beta, done honoured
};

}  // namespace heat3d
