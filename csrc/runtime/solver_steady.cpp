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
  // r and q: two more fields per local subdomain, kept for later calls
  {
    std::size_t extra = 0;
    for (const auto& l : local_)
      if (!l.steady_r) extra += 2 * l.L.bytes();
    if (extra) preflight_extra_field("steady solve (two work fields)", extra);
    for (auto& l : local_)
      if (!l.steady_r) {
        l.steady_r = be_->alloc(l.L.bytes());
        l.steady_q = be_->alloc(l.L.bytes());
        be_->memset(l.steady_r, 0, l.L.bytes(), kCompute);
        be_->memset(l.steady_q, 0, l.L.bytes(), kCompute);
      }
  }
  if (!cg_state_) {
    cg_state_ = static_cast<SteadyState*>(be_->alloc(sizeof(SteadyState)));
    cg_host_ = static_cast<SteadyState*>(be_->alloc_host(sizeof(SteadyState)));
  }
  const int xb = cur(), pb = nxt(xb);
  // the direction's buffer starts as zeros: its wall vertices and the ghosts
  // beyond the grid are never written and never used, but stay finite
  for (auto& l : local_) be_->memset(l.field[pb], 0, l.L.bytes(), kCompute);

  SteadyState hs;
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

  // r = b - A x and r . r (into rrn), whatever the flag says
  auto residual = [&]() {
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
  auto iteration = [&]() {
    if (has_halo_) enqueue_halo(pb, kCompute);
    for (std::size_t i = 0; i < local_.size(); ++i) {
      auto& l = local_[i];
      SteadyApplyParams sp = steady_params(l);
      sp.in = l.field[pb];
      sp.out = l.steady_q;
      sp.state = cg_state_;
      be_->steady_apply(sp, cg_state_->pq, i > 0, kCompute);
    }
    steady_allreduce(cg_state_->pq);
    be_->steady_scalars(cg_state_, kSteadyAlpha, kCompute);
    for (std::size_t i = 0; i < local_.size(); ++i) {
      auto& l = local_[i];
      SteadyUpdateParams up;
      up.x = l.field[xb];
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

  const auto t0 = std::chrono::steady_clock::now();
  SteadyResult res;
  double true_rr = 0.0;
  bool finite = true;
  for (bool first = true;; first = false) {
    residual();
    pull_state();
    true_rr = hs.rrn[0] + hs.rrn[1];
    if (first) hs.rr0 = -1.0;  // (Init sets it from this residual)
    const double rr0 = first ? true_rr : hs.rr0;
    // A finished call never reports kSteadyRunning: both exits below can be
    // taken before the first kSteadyInit, while the status is still unset.
    finite = true_rr == true_rr && true_rr <= 1.7976931348623157e308;
    if (!finite) {
      // a NaN or Inf in the field (or r . r overflows): nothing to iterate on
      hs.status = kSteadyBreakdown;
      break;
    }
    if (true_rr <= hs.tol2 * rr0) {
      // (the first residual is its own reference: with tol < 1, met when it is zero)
      if (first) hs.status = kSteadyConverged;
      break;
    }
    if (!first) {
      // the recurrence stopped: at the cap or broken down for good, or within
      // tol while the true residual is not: start again from the true residual
      if (hs.status != kSteadyConverged || res.restarts == kMaxRestarts) break;
      ++res.restarts;
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
  be_->sync_all();
  comm_->check_async_error();
  res.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

  const double rr0 = hs.rr0 >= 0.0 ? hs.rr0 : true_rr;
  res.iterations = hs.iter;
  res.status = hs.status;
  res.r0_norm = std::sqrt(rr0);
  // (before any iteration the recurrence's residual is the initial one)
  const double rec_rr = hs.rr0 >= 0.0 ? hs.rr : true_rr;
  res.residual = rr0 > 0.0 ? std::sqrt(rec_rr / rr0) : 0.0;
  res.true_residual = rr0 > 0.0 ? std::sqrt(true_rr / rr0) : 0.0;
  res.converged = finite && true_rr <= hs.tol2 * rr0;

  // The solution becomes the state of iteration 0, as after set_field: the
  // insulated / convective wall planes show what they show after time steps,
  // the ghosts are filled at full depth, every buffer of the rotation holds it.
  refresh_walls(xb, kCompute);
  if (has_halo_) enqueue_halo(xb, kCompute, long_halo_ ? 1 : 0);
  refresh_walls(xb, kCompute);
  for (auto& l : local_)
    for (int b = 0; b < nbuf_; ++b)
      if (b != xb) be_->copy(l.field[b], l.field[xb], l.L.bytes(), CopyKind::D2D, kCompute);
  be_->sync(kCompute);
  reset_state(false);
  return res;
}

}  // namespace heat3d
