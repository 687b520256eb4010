"""Cases and checks shared by tests/test_steady_cpu.py and tests/test_gpu_steady.py
(the direct steady-state solve, docs/ARCHITECTURE.md "Steady solve").

Solver level: tol = 1e-10, max_iter = 1000 (a NumPy model of the scheme needs at
most 182 iterations on these cases; the cap is a failure).  Check 1: the error
against the exact discrete steady state is at most kappa_hat * tol * the initial
error, kappa_hat = 6 (N_max - 1)^2 / c_min, a bound of the condition number
(largest eigenvalue <= 12 / h_min^2, smallest >= c_min pi^2 / 4).  Check 2: one
time step after the solve leaves a max-norm residual of at most
tol * r0_norm + 4 * 2^-52 (max norm <= 2-norm; the floor is the rounding of
T' - T at |T| <= 1)."""
import math

import numpy as np
import torch

TOL, CAP = 1e-10, 1000
EPS = 2.0 ** -52


def _interior(a):
    return a[1:-1, 1:-1, 1:-1]


def solver_cases(h3d):
    """name -> (N, solver keywords, setup(solver, model) -> (exact field or None, c_min))"""

    def reference(s, m):
        return m.steady_state(), 1.0

    def sine(s, m):
        s.set_source(m.sine_source(0.25))
        x, y, z = (np.arange(n) * h for n, h in zip(m.n, m.h))
        mode = np.sin(np.pi * x)[:, None, None] * np.sin(np.pi * y)[None, :, None] * np.sin(np.pi * z)[None, None, :]
        return m.steady_state() + 0.25 * mode, 1.0

    def layered(s, m):
        c = m.layered_conductivity(0.25, 1.0)
        s.set_conductivity(c)
        # the walls of the layered state, a zero interior as the initial guess
        exact = m.layered_steady(c)
        guess = exact.copy()
        guess[1:-1, 1:-1, 1:-1] = 0.0
        s.set_field(guess)
        return exact, 0.25

    def slab(s, m):
        return m.convective_slab_steady(0.5, 0.25), 1.0

    def open_form(s, m):
        # no closed form: a 3-D source, one convective face, a non-uniform conductivity
        rng = np.random.default_rng(7)
        s.set_source(m.sine_source(0.25))
        s.set_conductivity(rng.uniform(0.25, 1.0, m.n))
        return None, 0.25

    slab_kw = dict(insulated="x-,x+,z-,z+", convective={"y-": 0.5}, ambient=0.25)
    return {
        "reference33": ((33, 33, 33), {}, reference),
        "reference17x33x65": ((17, 33, 65), {}, reference),
        "sine_source": ((18, 21, 67), {}, sine),
        "layered": ((18, 33, 19), {}, layered),
        "convective_slab": ((17, 33, 19), slab_kw, slab),
        "open_form": ((18, 21, 67), dict(convective={"x+": 0.5}, ambient=0.25), open_form),
    }


def make_solver(h3d, name, backend, **extra):
    N, kw, setup = solver_cases(h3d)[name]
    kw = dict(kw)
    kw.update(extra)
    if backend == "hip":
        kw.setdefault("device", 0)
    s = h3d.HeatSolver(N, 100, 1e-5, backend=backend, dtype="fp64", **kw)
    s.initialize()
    exact, c_min = setup(s, s.model)
    return s, exact, c_min


def solve_and_check(h3d, name, backend, **extra):
    """Runs the case and asserts checks 1 and 2; returns (solver, result, field)."""
    s, exact, c_min = make_solver(h3d, name, backend, **extra)
    T0 = s.gather()
    r = s.solve_steady(TOL, CAP)
    T = s.gather()
    print(f"{name} {backend} {extra}: {r}")
    assert r["converged"] and r["status"] == "converged", r
    assert 0 < r["iterations"] < CAP, r
    assert r["true_residual"] <= TOL and r["residual"] <= TOL, r
    for key in ("converged", "iterations", "residual", "true_residual", "r0_norm", "seconds"):
        assert key in r
    if s.is_root and exact is not None:
        kappa = 6.0 * (max(s.model.n) - 1) ** 2 / c_min
        err = float(np.linalg.norm(_interior(T - exact)))
        err0 = float(np.linalg.norm(_interior(T0 - exact)))
        print(f"  error {err:.3e} bound {kappa * TOL * err0:.3e}")
        assert err <= kappa * TOL * err0
    s.step(1)
    last = s.state()["last_residual"]
    bound = TOL * r["r0_norm"] + 4 * EPS
    print(f"  residual of a step {last:.3e} bound {bound:.3e}")
    assert last <= bound
    return s, r, T


# ---- kernel level -------------------------------------------------------------
SHAPES = [(5, 5, 5), (18, 21, 67), (17, 33, 65)]
# kind per face (x-, x+, y-, y+, z-, z+): 0 Dirichlet, 1 insulated, 2 convective
WALLED = dict(kind=[1, 2, 0, 1, 2, 0], beta=[0.0, 0.5, 0.0, 0.0, 0.3, 0.0])
FORMS = {
    "uniform": dict(),
    "conductivity": dict(cond=True),
    "walls": dict(**WALLED),
    "conductivity_walls": dict(cond=True, **WALLED),
}


def physics_D(h3d, N):
    m = h3d.HeatEquation3D(N)
    return [m.alpha * m.dt / h ** 2 for h in m.h]


def padded(h3d, N, arr, device):
    """PaddedField of a grid N whose owned block is the interior; arr: the (N) array."""
    from heat3d_amd.ops import PaddedField

    f = PaddedField([n - 2 for n in N], torch.float64, device)
    f.ghosted().copy_(torch.from_numpy(np.ascontiguousarray(arr)).to(device))
    return f


def random_fields(N, seed, count):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1.0, 1.0, N) for _ in range(count)]


def form_fields(h3d, N, form, device, seed=3):
    rng = np.random.default_rng(seed)
    kw = {k: v for k, v in FORMS[form].items() if k != "cond"}
    if FORMS[form].get("cond"):
        kw["cond"] = padded(h3d, N, 0.5 * rng.uniform(0.25, 1.0, N), device)
    return kw


def owned_np(f, box=None):
    a = f.owned().cpu().numpy()
    if box is not None:
        a = a[box[0]:box[1], box[2]:box[3], box[4]:box[5]]
    return a


def fsum_bound(a, b):
    terms = (a.astype(np.float64) * b.astype(np.float64)).ravel().tolist()
    return math.fsum(terms), math.fsum(abs(t) for t in terms)


def sub_box(n):
    """a box that touches the block's low x, high y and high z sides only"""
    return [0, max(1, n[0] - 1), min(1, n[1] - 1), n[1], min(2, n[2] - 1), n[2]]
