// heat3d-mi355x — Solver::solve_steady: the direct steady-state solve by
// conjugate gradients on the device (kernels/steady_cg.hpp,
// docs/ARCHITECTURE.md "Steady solve").
//
// x is the current field, p lives in the spare time-step buffer (so that
// enqueue_halo moves its ghosts), r and q are two extra fields per subdomain,
// allocated on first use and kept.  Per iteration, on the compute stream:
//   halo of p;  q = A p and p . q per subdomain, combined on the device in
//   order;  [all-reduce of the pair];  scalars: alpha;
//   x += alpha p, r -= alpha q and r . r;  [all-reduce];  scalars: beta, the
//   iteration count, the stop flag;  p = r + beta p.
// Once the flag is set every later kernel returns at once; the host reads the
// state every kPoll iterations, so the reported iteration is exact.
//
// Solver::step_implicit (docs/ARCHITECTURE.md "Implicit steps") runs the same
// loop (cg_solve) on (R + mu A) d = r(T): the unknown d is a third extra field,
// the field T stays in the current buffer until T' = fma(m, d, T) is formed.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "solver.hpp"

namespace heat3d {

namespace {
constexpr int kPoll = 8;          // iterations between two reads of the stop flag
constexpr int kMaxRestarts = 3;   // restarts from the true residual
}  // namespace

SteadyApplyParams Solver::steady_params(const Local& l) const {
  SteadyApplyParams sp;
  sp.L = l.L;
  sp.cond = has_cond_ ? l.cond : nullptr;
  sp.src = has_source_ ? l.source : nullptr;
  sp.ambient = cfg_.ambient;
  const auto& N = dec_.N;
  for (int a = 0; a < 3; ++a) {
    sp.D[a] = phys_.D[a];
    // the updated points of this subdomain: global indices 1 .. N - 2
    sp.box.lo[a] = std::max<int64_t>(l.owned.lo[a], 1 - l.sd.gstart[a]);
    sp.box.hi[a] = std::min<int64_t>(l.owned.hi[a], N[a] - 1 - l.sd.gstart[a]);
    for (int e = 0; e < 2; ++e) {
      const int f = 2 * a + e;
      const int64_t w = (e ? N[a] - 2 : 1) - l.sd.gstart[a];
      sp.wall[a][e] = w >= sp.box.lo[a] && w < sp.box.hi[a] ? w : kNoBalanceWall;
      sp.kind[a][e] = ((conv_ >> f) & 1u) ? kWallConvective : ((walls_ >> f) & 1u) ? kWallInsulated : kWallDirichlet;
      sp.beta[a][e] = ((conv_ >> f) & 1u) ? conv_beta_[f] : 0.0;
    }
  }
  return sp;
}

// the pair at `pair` (device): the sum over this process's subdomains -> the job's
void Solver::steady_allreduce(double* pair) {
  if (comm_->all_local() || comm_->size() <= 1) return;
  comm_token_wait(kCompute);
  comm_->allreduce(pair, 2, RedType::F64, RedOp::Sum, *be_, kCompute);
  comm_token_signal(kCompute);
}

void Solver::steady_workspace(bool with_d) {
  // r and q (and d): extra fields per local subdomain, kept for later calls
  std::size_t extra = 0;
  for (const auto& l : local_) {
    if (!l.steady_r) extra += 2 * l.L.bytes();
    if (with_d && !l.steady_d) extra += l.L.bytes();
  }
  if (extra) preflight_extra_field(with_d ? "implicit steps (three work fields)" : "steady solve (two work fields)", extra);
  for (auto& l : local_) {
    if (!l.steady_r) {
      l.steady_r = be_->alloc(l.L.bytes());
      l.steady_q = be_->alloc(l.L.bytes());
      be_->memset(l.steady_r, 0, l.L.bytes(), kCompute);
      be_->memset(l.steady_q, 0, l.L.bytes(), kCompute);
    }
    if (with_d && !l.steady_d) l.steady_d = be_->alloc(l.L.bytes());
  }
  if (!cg_state_) {
    cg_state_ = static_cast<SteadyState*>(be_->alloc(sizeof(SteadyState)));
    cg_host_ = static_cast<SteadyState*>(be_->alloc_host(sizeof(SteadyState)));
  }
}

Solver::CgOutcome Solver::cg_solve(double tol, int64_t max_iter, int pb, const std::function<void*(Local&)>& x_of,
                                   const std::function<void(SteadyApplyParams&, const Local&)>& shape,
                                   const std::function<void(bool)>& true_residual) {
  CgOutcome o;
  SteadyState& hs = o.hs;
  std::memset(&hs, 0, sizeof(hs));
  hs.rr0 = -1.0;
  hs.tol2 = tol * tol;
  hs.max_iter = max_iter;
  auto push_state = [&]() {
    std::memcpy(cg_host_, &hs, sizeof(hs));
    be_->copy(cg_state_, cg_host_, sizeof(SteadyState), CopyKind::H2D, kCompute);
    be_->sync(kCompute);
  };
  auto pull_state = [&]() {
    be_->copy(cg_host_, cg_state_, sizeof(SteadyState), CopyKind::D2H, kCompute);
    be_->sync(kCompute);
    std::memcpy(&hs, cg_host_, sizeof(hs));
  };
  push_state();

  auto iteration = [&]() {
    if (has_halo_) enqueue_halo(pb, kCompute);
    for (std::size_t i = 0; i < local_.size(); ++i) {
      auto& l = local_[i];
      SteadyApplyParams sp = steady_params(l);
      sp.in = l.field[pb];
      sp.out = l.steady_q;
      sp.state = cg_state_;
      shape(sp, l);
      be_->steady_apply(sp, cg_state_->pq, i > 0, kCompute);
    }
    steady_allreduce(cg_state_->pq);
    be_->steady_scalars(cg_state_, kSteadyAlpha, kCompute);
    for (std::size_t i = 0; i < local_.size(); ++i) {
      auto& l = local_[i];
      SteadyUpdateParams up;
      up.x = x_of(l);
      up.p = l.field[pb];
      up.r = l.steady_r;
      up.q = l.steady_q;
      up.L = l.L;
      up.box = steady_params(l).box;
      up.state = cg_state_;
      be_->steady_update(up, cg_state_->rrn, i > 0, kCompute);
    }
    steady_allreduce(cg_state_->rrn);
    be_->steady_scalars(cg_state_, kSteadyBeta, kCompute);
    for (auto& l : local_) {
      SteadyDirectionParams dp;
      dp.p = l.field[pb];
      dp.r = l.steady_r;
      dp.L = l.L;
      dp.box = steady_params(l).box;
      dp.state = cg_state_;
      be_->steady_direction(dp, kCompute);
    }
  };

  for (bool first = true;; first = false) {
    true_residual(first);
    pull_state();
    o.true_rr = hs.rrn[0] + hs.rrn[1];
    if (first) hs.rr0 = -1.0;  // (Init sets it from this residual)
    const double rr0 = first ? o.true_rr : hs.rr0;
    // A finished call never reports kSteadyRunning: both exits below can be
    // taken before the first kSteadyInit, while the status is still unset.
    o.finite = o.true_rr == o.true_rr && o.true_rr <= 1.7976931348623157e308;
    if (!o.finite) {
      // a NaN or Inf in the field (or r . r overflows): nothing to iterate on
      hs.status = kSteadyBreakdown;
      break;
    }
    if (o.true_rr <= hs.tol2 * rr0) {
      // (the first residual is its own reference: with tol < 1, met when it is zero)
      if (first) hs.status = kSteadyConverged;
      break;
    }
    if (!first) {
      // the recurrence stopped: at the cap or broken down for good, or within
      // tol while the true residual is not: start again from the true residual
      if (hs.status != kSteadyConverged || o.restarts == kMaxRestarts) break;
      ++o.restarts;
    }
    hs.done = 0;
    hs.status = kSteadyRunning;
    push_state();
    be_->steady_scalars(cg_state_, kSteadyInit, kCompute);
    for (auto& l : local_) {
      SteadyDirectionParams dp;
      dp.p = l.field[pb];
      dp.r = l.steady_r;
      dp.L = l.L;
      dp.box = steady_params(l).box;
      dp.copy = true;
      dp.state = cg_state_;
      be_->steady_direction(dp, kCompute);
    }
    do {
      for (int it = 0; it < kPoll; ++it) iteration();
      pull_state();
    } while (!hs.done);
  }
  return o;
}

// The field in buffer xb becomes the state of iteration 0, as after set_field:
// the insulated / convective wall planes show what they show after time steps,
// the ghosts are filled at full depth, every buffer of the rotation holds it.
void Solver::steady_publish(int xb, bool all) {
  refresh_walls(xb, kCompute);
  if (has_halo_) enqueue_halo(xb, kCompute, long_halo_ ? 1 : 0);
  refresh_walls(xb, kCompute);
  if (!all) return;
  for (auto& l : local_)
    for (int b = 0; b < nbuf_; ++b)
      if (b != xb) be_->copy(l.field[b], l.field[xb], l.L.bytes(), CopyKind::D2D, kCompute);
  be_->sync(kCompute);
  reset_state(false);
}

SteadyResult Solver::solve_steady(double tol, int64_t max_iter) {
  if (cfg_.compat || cfg_.scheme == "reference")
    throw UsageError("the steady solve is not part of --compat / --scheme reference (the reference only steps in time)");
  if (dt_ != DType::F64)
    throw UsageError("the steady solve needs fp64 fields: in fp32 conjugate gradients cannot get below about "
                     "kappa * 2^-24 (kappa ~ 4e5 at 1024^3); use --dtype fp64");
  if (!(tol > 0.0) || !std::isfinite(tol)) throw UsageError("the steady solve's tolerance must be positive and finite");
  {
    bool anchored = false;
    for (int f = 0; f < kNumFaces; ++f) {
      const bool dirichlet = !((walls_ >> f) & 1u);
      const bool convective = ((conv_ >> f) & 1u) && conv_beta_[f] > 0.0;
      anchored |= dirichlet || convective;
    }
    if (!anchored)
      throw UsageError("the steady solve needs a Dirichlet face or a convective face with a positive coefficient: "
                       "with every face insulated the system is singular");
  }
  HEAT3D_CHECK(initialized_, "solve_steady: initialize() first");
  if (max_iter <= 0) max_iter = 10 * (dec_.N[0] + dec_.N[1] + dec_.N[2]);

  be_->sync_all();
  pending_.valid = false;
  steady_workspace(false);
  const int xb = cur(), pb = nxt(xb);
  // the direction's buffer starts as zeros: its wall vertices and the ghosts
  // beyond the grid are never written and never used, but stay finite
  for (auto& l : local_) be_->memset(l.field[pb], 0, l.L.bytes(), kCompute);

  // r = b - A x and r . r (into rrn), whatever the flag says
  auto residual = [&](bool) {
    if (has_halo_) enqueue_halo(xb, kCompute);
    for (std::size_t i = 0; i < local_.size(); ++i) {
      auto& l = local_[i];
      SteadyApplyParams sp = steady_params(l);
      sp.in = l.field[xb];
      sp.out = l.steady_r;
      sp.residual = true;
      be_->steady_apply(sp, cg_state_->rrn, i > 0, kCompute);
    }
    steady_allreduce(cg_state_->rrn);
  };

  const auto t0 = std::chrono::steady_clock::now();
  const CgOutcome o = cg_solve(
      tol, max_iter, pb, [&](Local& l) { return l.field[xb]; }, [](SteadyApplyParams&, const Local&) {}, residual);
  const SteadyState& hs = o.hs;
  be_->sync_all();
  comm_->check_async_error();
  SteadyResult res;
  res.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

  const double rr0 = hs.rr0 >= 0.0 ? hs.rr0 : o.true_rr;
  res.iterations = hs.iter;
  res.status = hs.status;
  res.restarts = o.restarts;
  res.r0_norm = std::sqrt(rr0);
  // (before any iteration the recurrence's residual is the initial one)
  const double rec_rr = hs.rr0 >= 0.0 ? hs.rr : o.true_rr;
  res.residual = rr0 > 0.0 ? std::sqrt(rec_rr / rr0) : 0.0;
  res.true_residual = rr0 > 0.0 ? std::sqrt(o.true_rr / rr0) : 0.0;
  res.converged = o.finite && o.true_rr <= hs.tol2 * rr0;

  steady_publish(xb, true);
  return res;
}

ImplicitResult Solver::step_implicit(int64_t steps, double m, double theta, double tol, int64_t max_iter) {
  if (cfg_.compat || cfg_.scheme == "reference")
    throw UsageError("implicit steps are not part of --compat / --scheme reference (the reference's explicit step)");
  if (dt_ != DType::F64)
    throw UsageError("implicit steps need fp64 fields: in fp32 conjugate gradients cannot get below about "
                     "kappa * 2^-24; use --dtype fp64");
  if (!(m > 0.0) || !std::isfinite(m))
    throw UsageError("an implicit step's length m (in explicit time steps) must be positive and finite");
  if (!(theta >= 0.5 && theta <= 1.0))
    throw UsageError("an implicit step's theta must lie in [0.5, 1] (1: backward Euler, 0.5: Crank-Nicolson; "
                     "below 0.5 the step is not unconditionally stable)");
  if (!(tol > 0.0) || !std::isfinite(tol)) throw UsageError("the implicit steps' tolerance must be positive and finite");
  if (steps < 0) throw UsageError("the number of implicit steps must not be negative");
  HEAT3D_CHECK(initialized_, "step_implicit: initialize() first");
  if (max_iter <= 0) max_iter = 10 * (dec_.N[0] + dec_.N[1] + dec_.N[2]);

  be_->sync_all();
  pending_.valid = false;
  steady_workspace(true);
  const int xb = cur(), pb = nxt(xb);
  const double mu = theta * m;
  // (as in solve_steady: the direction's wall vertices and outer ghosts stay finite)
  for (auto& l : local_) be_->memset(l.field[pb], 0, l.L.bytes(), kCompute);

  // M = R + mu A
  auto shape = [&](SteadyApplyParams& sp, const Local& l) {
    sp.shift = true;
    sp.mu = mu;
    sp.cap = has_cap_ ? l.cap : nullptr;
  };
  // r = r(T) - M d and r . r (into rrn), whatever the flag says; d = 0 the first time
  auto residual = [&](bool first) {
    if (has_halo_) enqueue_halo(xb, kCompute);
    for (std::size_t i = 0; i < local_.size(); ++i) {
      auto& l = local_[i];
      SteadyApplyParams sp = steady_params(l);
      sp.in = l.field[xb];
      sp.out = l.steady_r;
      sp.residual = true;
      be_->steady_apply(sp, first ? cg_state_->rrn : nullptr, i > 0, kCompute);
    }
    if (!first) {
      // (the recurrence has stopped: the direction's buffer is free)
      for (auto& l : local_) be_->copy(l.field[pb], l.steady_d, l.L.bytes(), CopyKind::D2D, kCompute);
      if (has_halo_) enqueue_halo(pb, kCompute);
      for (auto& l : local_) {
        SteadyApplyParams sp = steady_params(l);
        sp.in = l.field[pb];
        sp.out = l.steady_q;
        shape(sp, l);
        be_->steady_apply(sp, nullptr, false, kCompute);
      }
      for (std::size_t i = 0; i < local_.size(); ++i) {
        auto& l = local_[i];
        SteadyUpdateParams up;
        up.r = l.steady_r;
        up.q = l.steady_q;
        up.L = l.L;
        up.box = steady_params(l).box;
        up.alpha = 1.0;
        be_->steady_update(up, cg_state_->rrn, i > 0, kCompute);
      }
    }
    steady_allreduce(cg_state_->rrn);
  };

  const auto t0 = std::chrono::steady_clock::now();
  ImplicitResult res;
  res.converged = true;
  res.status = kSteadyConverged;
  for (int64_t n = 0; n < steps; ++n) {
    for (auto& l : local_) be_->memset(l.steady_d, 0, l.L.bytes(), kCompute);
    const CgOutcome o = cg_solve(tol, max_iter, pb, [](Local& l) { return l.steady_d; }, shape, residual);
    const SteadyState& hs = o.hs;
    const double rr0 = hs.rr0 >= 0.0 ? hs.rr0 : o.true_rr;
    const double rec_rr = hs.rr0 >= 0.0 ? hs.rr : o.true_rr;
    const bool ok = o.finite && o.true_rr <= hs.tol2 * rr0;
    res.status = hs.status;
    res.restarts += o.restarts;
    res.r0_norm = std::sqrt(rr0);
    res.residual = rr0 > 0.0 ? std::sqrt(rec_rr / rr0) : 0.0;
    res.true_residual = rr0 > 0.0 ? std::sqrt(o.true_rr / rr0) : 0.0;
    res.converged = res.converged && ok;
    // r . r not finite (in r(T), or after iterations on it): the field stays as
    // it was before this step
    if (!o.finite || (hs.status == kSteadyBreakdown && !ok)) {
      res.status = kSteadyBreakdown;
      res.converged = false;
      break;
    }
    res.iterations += hs.iter;
    res.step_iterations.push_back(hs.iter);
    ++res.steps_done;
    if (hs.iter > 0) {
      // T' = fma(m, d, T) (no iteration: d = 0, the field's bits stay)
      for (auto& l : local_) {
        SteadyUpdateParams up;
        up.x = l.field[xb];
        up.p = l.steady_d;
        up.L = l.L;
        up.box = steady_params(l).box;
        up.alpha = m;
        be_->steady_update(up, nullptr, false, kCompute);
      }
      steady_publish(xb, false);
    }
    if (!ok) break;  // stopped at max_iter: applied, and the call ends here
  }
  be_->sync_all();
  comm_->check_async_error();
  res.time_advanced = (double)res.steps_done * m;
  // Intended on every exit, with no step done or a breakdown in the first one
  // too: the call always leaves the state of iteration 0, as solve_steady does.
  // (After an applied step this repeats that step's wall refresh and halo fill:
  // one exchange per call, kept so that there is one way out.)
  steady_publish(xb, true);
  res.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return res;
}

}  // namespace heat3d
