"""Cases and checks shared by tests/test_implicit_cpu.py and tests/test_gpu_implicit.py
(implicit time steps, docs/ARCHITECTURE.md "Implicit steps").

The host side of every check uses the existing residual form r(T) = b - A T
(ops.steady_apply(residual=True), the CPU definition) and NumPy only: nothing
below calls the shifted operator it checks."""
import numpy as np
import torch

import _steady_cases as sc

TOL = 1e-8
EPS = sc.EPS
ROUND = 2.0 ** -40  # the rounding allowance of the defect check (far below TOL, far above EPS)
FACES = ["x-", "x+", "y-", "y+", "z-", "z+"]
MS = (1.0, 64.0, 4096.0)
THETAS = (1.0, 0.5)


class _Recorder:
    """Forwards to a HeatSolver and keeps what a case's setup hands to it."""

    def __init__(self, s):
        self._s, self.q, self.c = s, None, None

    def set_source(self, q):
        self.q = np.array(q, dtype=np.float64)
        self._s.set_source(q)

    def set_conductivity(self, c):
        self.c = np.array(c, dtype=np.float64)
        self._s.set_conductivity(c)

    def __getattr__(self, name):
        return getattr(self._s, name)


class Case:
    """A solver with the arrays that define its mode, for the host-side residual."""

    def __init__(self, h3d, s, N, kw, q=None, c=None, rc=None, exact=None):
        self.h3d, self.s, self.N, self.q, self.c, self.rc, self.exact = h3d, s, tuple(N), q, c, rc, exact
        ins = kw.get("insulated", "")
        ins = FACES if ins == "all" else [f for f in ins.split(",") if f]
        conv = kw.get("convective", {}) or {}
        self.kind = [2 if f in conv else 1 if f in ins else 0 for f in FACES]
        self.beta = [float(conv.get(f, 0.0)) for f in FACES]
        self.ambient = float(kw.get("ambient", 0.0))
        self.D = sc.physics_D(h3d, N)

    def R(self):
        return 1.0 if self.rc is None else self.rc[1:-1, 1:-1, 1:-1]

    def residual(self, T):
        """r(T) = G(T) - T over the updated points, by the existing residual form on the host"""
        from heat3d_amd import ops

        h3d, N = self.h3d, self.N
        Tf = sc.padded(h3d, N, T, "cpu")
        rf = sc.padded(h3d, N, np.zeros(N), "cpu")
        kw = {}
        if self.q is not None:
            kw["source"] = sc.padded(h3d, N, self.s.model.dt * self.q, "cpu")
        if self.c is not None:
            kw["cond"] = sc.padded(h3d, N, 0.5 * self.c, "cpu")
        ops.steady_apply(Tf, rf, self.D, kind=self.kind, beta=self.beta, ambient=self.ambient, residual=True, **kw)
        return sc.owned_np(rf).copy()


def make_case(h3d, name, backend, cap=False, **extra):
    """A case of _steady_cases.solver_cases, with a random capacity in [1, 8] when asked"""
    N, kw, setup = sc.solver_cases(h3d)[name]
    kw = dict(kw)
    kw.update(extra)
    if backend == "hip":
        kw.setdefault("device", 0)
    s = h3d.HeatSolver(N, 100, 1e-5, backend=backend, dtype="fp64", **kw)
    s.initialize()
    rec = _Recorder(s)
    exact, _ = setup(rec, s.model)
    rc = None
    if cap:
        rc = np.random.default_rng(5).uniform(1.0, 8.0, N)
        s.set_capacity(rc)
    return Case(h3d, s, N, kw, rec.q, rec.c, rc, exact)


def norm(a):
    return float(np.linalg.norm(np.asarray(a).ravel()))


def defect(case, T0, T1, m, theta):
    """||e||, e = R (T' - T) / m - theta r(T') - (1 - theta) r(T), and the rounding allowance"""
    r0, r1 = case.residual(T0), case.residual(T1)
    a = case.R() * (T1 - T0)[1:-1, 1:-1, 1:-1] / m
    e = a - theta * r1 - (1.0 - theta) * r0
    return norm(e), ROUND * (norm(a) + norm(r1) + norm(r0)), norm(r0)


def check_defect(case, m, theta, T0=None):
    """One step from T0 (default: the current field); asserts the defect bound and
    that the report's true residual is that defect; returns (result, T0, T')."""
    s = case.s
    if T0 is None:
        T0 = s.gather()
    else:
        s.set_field(T0)
        T0 = s.gather()
    r = s.step_implicit(1, m, theta, tol=TOL)
    T1 = s.gather()
    e, allow, r0n = defect(case, T0, T1, m, theta)
    print(f"  m {m:g} theta {theta}: iterations {r['iterations']} ||e|| {e:.3e} bound {TOL * r['r0_norm'] + allow:.3e} "
          f"(rounding {allow:.3e}) reported {r['true_residual'] * r['r0_norm']:.3e} r0 {r['r0_norm']:.6e} host {r0n:.6e}")
    assert r["converged"] and r["status"] == "converged" and r["steps_done"] == 1, r
    assert r["time_advanced"] == m and r["step_iterations"] == [r["iterations"]], r
    assert abs(r["r0_norm"] - r0n) <= allow
    assert e <= TOL * r["r0_norm"] + allow
    assert abs(r["true_residual"] * r["r0_norm"] - e) <= allow
    return r, T0, T1


MODE_N, MODE_VEC, MODE_RC = (17, 33, 65), (1, 2, 3), 4.0


def mode_solver(h3d, backend, **extra):
    """dirichlet_mode between zero walls in a body of uniform capacity rc = 4"""
    if backend == "hip":
        extra.setdefault("device", 0)
    s = h3d.HeatSolver(MODE_N, 100, 1e-5, backend=backend, dtype="fp64", **extra)
    s.initialize()
    T, _ = s.model.dirichlet_mode(MODE_VEC)
    s.set_capacity(np.full(MODE_N, MODE_RC))
    return s, T


def check_mode_factor(h3d, backend, m, theta):
    """An eigenvector of A (and of R = rc I): one step multiplies it by
    implicit_factor.  The solve's error in d is at most ||residual|| /
    lambda_min(M) <= tol r0_norm (lambda_min(M) >= 1 as R >= I), m times that in
    T'; r is an eigenvector, so CG ends in one iteration (two allowed)."""
    s, T = mode_solver(h3d, backend)
    s.set_field(T)
    r = s.step_implicit(1, m, theta, tol=TOL)
    g = s.model.implicit_factor(MODE_VEC, m, theta, s=1.0 / MODE_RC)
    err = norm(s.gather() - g * T)
    bound = m * TOL * r["r0_norm"]
    print(f"mode {backend} m {m:g} theta {theta}: factor {g!r} err {err:.3e} bound {bound:.3e} iterations {r['iterations']}")
    assert r["converged"] and 1 <= r["iterations"] <= 2, r
    assert err <= bound
    return r, s.gather()


BAL_N = (11, 9, 14)
BAL_KW = dict(insulated="x-,z+", convective={"x+": 0.3, "y-": 0.5}, ambient=0.25)


def balance_case(h3d, backend, N=BAL_N, **extra):
    """A source, a conductivity, insulated / convective / Dirichlet faces and a layered capacity"""
    N = tuple(N)
    kw = dict(BAL_KW)
    kw.update(extra)
    if backend == "hip":
        kw.setdefault("device", 0)
    s = h3d.HeatSolver(N, 100, 1e-5, backend=backend, dtype="fp64", **kw)
    s.initialize()
    rng = np.random.default_rng(9)
    s.set_field(rng.uniform(0.0, 1.0, N))
    q, c, rc = rng.uniform(0.0, 2.0, N), rng.uniform(0.25, 1.0, N), s.model.layered_capacity(1.0, 8.0)
    s.set_source(q)
    s.set_conductivity(c)
    s.set_capacity(rc)
    return Case(h3d, s, N, kw, q, c, rc)


def check_balance_identity(case, m, theta, steps=1):
    """heat(T') - heat(T) = m dt [theta imbalance(T') + (1 - theta) imbalance(T)].
    Summing the step's equation over the points leaves m * sum(e), |sum e| <=
    sqrt(points) ||e||_2 <= sqrt(points) tol r0_norm; the rounding allowance is
    the balance tests' (tests/test_heat_balance_cpu.py test_per_step_identity):
    8 eps max|T| |U| hx hy hz."""
    s, N = case.s, case.N
    mdl = s.model
    U = (N[0] - 2) * (N[1] - 2) * (N[2] - 2)
    vol = mdl.h[0] * mdl.h[1] * mdl.h[2]
    b = s.heat_balance()
    out = []
    for n in range(steps):
        r = s.step_implicit(1, m, theta, tol=TOL)
        assert r["converged"], r
        nb = s.heat_balance()
        tmax = max(abs(b["t_min"]), abs(b["t_max"]), abs(nb["t_min"]), abs(nb["t_max"]))
        bound = vol * m * np.sqrt(U) * TOL * r["r0_norm"] + 8 * EPS * tmax * U * vol
        dheat = nb["heat"] - b["heat"]
        d = abs(dheat - m * mdl.dt * (theta * nb["imbalance"] + (1.0 - theta) * b["imbalance"]))
        print(f"  step {n} m {m:g} theta {theta}: dheat {dheat:.6e} defect {d:.3e} bound {bound:.3e}")
        assert d <= bound
        out.append((dheat, bound, r))
        b = nb
    return out


def fields_agree(Ta, Tb, m, r0_norm, what=""):
    """'to the tolerance': 10 m tol r0_norm in the 2-norm"""
    d, bound = norm(Ta - Tb), 10.0 * m * TOL * r0_norm
    print(f"  {what}: ||difference|| {d:.3e} bound {bound:.3e}")
    assert d <= bound


def report(r):
    return {k: v for k, v in r.items() if k != "seconds"}


def to_torch(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)
