"""The implementation-independent checks of the heat capacity, written once for
every backend: tests/test_capacity_cpu.py runs them on the CPU backend,
tests/test_gpu_capacity.py on the gfx950 one."""
import numpy as np
import torch

EPS = {"fp64": 2.0 ** -52, "fp32": 2.0 ** -23}


def solver(h3d, backend, N, dtype="fp64", iters=1000, eps=0.0, **kw):
    return h3d.HeatSolver(N, iters, eps, dtype=dtype, backend=backend, **kw)


def eigenmode_decay(h3d, backend, dtype, rc):
    """The product sine mode decays by g = 1 - s 4 sum_a D_a sin^2(...) per step.
    The tolerance of tests/test_walls_cpu.py test_eigenmode: an update is about
    10 roundings of at most one half ulp on values <= 1, so after n steps
    |err| <= 10 n u * 4, u = 2^-53 (fp64) or 2^-24 (fp32); in fp32 the factor g
    is the one of the rounded D, which the bound's slack of 4 covers."""
    N, n = (17, 21, 19), 40
    s = solver(h3d, backend, N, dtype, extra_args=["--temporal", "1"])
    T0, g = s.model.dirichlet_mode((1, 2, 1), 1.0 / rc)
    _, g1 = s.model.dirichlet_mode((1, 2, 1))
    assert 0.0 < g1 < g < 1.0 if rc > 1 else g == g1
    T0 = T0.astype(np.float32).astype(np.float64) if dtype == "fp32" else T0
    s.set_field(T0)
    s.set_capacity(np.full(N, rc))
    s.step(n)
    s.synchronize()
    if dtype == "fp32":  # the factor of the diffusion numbers as the kernel holds them
        D32 = [float(np.float32(d)) for d in s.model.D]
        lam = sum(D32[a] * np.sin(np.pi * (1, 2, 1)[a] / (2.0 * (N[a] - 1))) ** 2 for a in range(3))
        g = 1.0 - float(np.float32(1.0 / rc)) * 4.0 * lam
    err = np.abs(s.gather() - g ** n * T0)[1:-1, 1:-1, 1:-1].max()
    bound = 10 * n * (EPS[dtype] / 2) * 4
    print(f"dirichlet mode rc {rc} {dtype}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound


def weighted_heat_is_conserved(h3d, backend):
    """All faces insulated, two layers of capacity 1 and 8: the weighted heat
    hx hy hz sum rc T moves by rounding only, within the bound the insulated
    cube's test (tests/test_walls_cpu.py test_heat_is_conserved) allows for
    sum T, 10 n M 2^-53 (times the cell volume); sum T itself moves by far more.
    At every checked step heat(n+1) - heat(n) = dt * imbalance(n) within the
    bound of tests/test_heat_balance_cpu.py test_per_step_identity."""
    N, n = (17, 17, 17), 200
    s = solver(h3d, backend, N, insulated="all", extra_args=["--temporal", "1"])
    m = s.model
    rng = np.random.default_rng(3)
    T0 = rng.uniform(0.0, 1.0, N)
    s.set_field(T0)
    s.set_capacity(m.layered_capacity(1.0, 8.0))
    U = (N[0] - 2) ** 3
    vol = m.h[0] * m.h[1] * m.h[2]
    b0 = s.heat_balance()
    assert b0["capacity"] is True
    sum0 = s.gather()[1:-1, 1:-1, 1:-1].sum()
    b = b0
    for k in range(6):
        s.step(1)
        nb = s.heat_balance()
        tmax = max(abs(b["t_min"]), abs(b["t_max"]), abs(nb["t_min"]), abs(nb["t_max"]))
        # (the terms of the weighted heat are rc T <= 8 max|T|)
        bound = 8 * EPS["fp64"] * tmax * U * vol
        defect = abs(nb["heat"] - b["heat"] - m.dt * b["imbalance"])
        print(f"step {k}: defect {defect:.3e} bound {bound:.3e}")
        assert defect <= bound
        b = nb
    s.step(n - 6)
    end = s.heat_balance()
    drift = abs(end["heat"] - b0["heat"])
    bound = 10 * n * U * 2.0 ** -53 * vol
    moved = abs(s.gather()[1:-1, 1:-1, 1:-1].sum() - sum0)
    print(f"weighted heat drift {drift:.3e} bound {bound:.3e}; sum T moved {moved * vol:.3e}")
    assert drift <= bound
    assert moved * vol > 1000 * bound  # the weighting is what conserves


SLAB = (9, 15, 9)


def _slab(h3d, backend, eps, iters=400000):
    return solver(h3d, backend, SLAB, "fp64", iters, eps, insulated="x-,x+,z-,z+", convective={"y-": 0.5}, ambient=0.25)


def steady_state_does_not_depend_on_the_capacity(h3d, backend):
    """The convective slab: with layered_capacity(1, 8) run() to eps 1e-10 lands on
    convective_slab_steady as closely as the run without a capacity does (the
    error is proportional to the residual once the slowest mode dominates, the
    bound of tests/test_convective_cpu.py: 10x closer from eps 1e-6 to 1e-8, so
    at most the plain run's eps 1e-8 error here), after more iterations."""
    want = None
    out = {}
    for cap in (False, True):
        s = _slab(h3d, backend, 1e-10)
        want = s.model.convective_slab_steady(0.5, 0.25)
        s.initialize()
        if cap:
            s.set_capacity(s.model.layered_capacity(1.0, 8.0))
        r = s.run()
        assert r["converged"]
        out[cap] = (r["conv_iter"], np.abs(s.gather() - want)[1:-1, 1:-1, 1:-1].max())
    ref = _slab(h3d, backend, 1e-8)
    assert ref.run()["converged"]
    e8 = np.abs(ref.gather() - want)[1:-1, 1:-1, 1:-1].max()
    print(f"slab: plain {out[False]}, capacity {out[True]}, plain at eps 1e-8 {e8:.3e}")
    assert out[True][0] > out[False][0]
    assert out[False][1] * 10 <= e8 and out[True][1] * 10 <= e8


def solve_steady_ignores_the_capacity(h3d, backend):
    res = []
    for cap in (False, True):
        s = _slab(h3d, backend, 1e-10)
        s.initialize()
        if cap:
            s.set_capacity(s.model.layered_capacity(1.0, 8.0))
        r = s.solve_steady(1e-10)
        assert r["converged"]
        res.append((r["iterations"], s.gather().tobytes()))
    assert res[0] == res[1]


def _definition_step(T, ch, S, sv, D, beta_ym, tinf):
    """One step of the issue's four lines on a ghosted float64 block (torch),
    walls x- insulated and y- convective handled as refreshed wall planes."""
    from heat3d_amd.utils.fma import fma

    T = T.clone()
    T[0, :, 1:-1] = T[1, :, 1:-1]  # x- insulated: a copy of the inward neighbour (z faces Dirichlet)
    c1 = T[:-1, 1, 1:-1].clone()   # y- convective: the ghost of the first interior row (x+ Dirichlet)
    T[:-1, 0, 1:-1] = fma(beta_ym, torch.tensor(tinf, dtype=T.dtype) - c1, c1)

    def seven(F):
        return (F[1:-1, 1:-1, 1:-1], F[:-2, 1:-1, 1:-1], F[2:, 1:-1, 1:-1], F[1:-1, :-2, 1:-1], F[1:-1, 2:, 1:-1],
                F[1:-1, 1:-1, :-2], F[1:-1, 1:-1, 2:])

    c, xm, xp, ym, yp, zm, zp = seven(T)
    hc, hxm, hxp, hym, hyp, hzm, hzp = seven(ch)
    fx = fma(hc + hxp, xp - c, (hc + hxm) * (xm - c))
    fy = fma(hc + hyp, yp - c, (hc + hym) * (ym - c))
    fz = fma(hc + hzp, zp - c, (hc + hzm) * (zm - c))
    u = fma(D[2], fz, fma(D[1], fy, D[0] * fx))
    u = u + S[1:-1, 1:-1, 1:-1]
    new = T.clone()
    new[1:-1, 1:-1, 1:-1] = fma(sv[1:-1, 1:-1, 1:-1], u, c)
    return new


def layered_transient_matches_the_definition(h3d, backend):
    N = (13, 15, 17)
    s = solver(h3d, backend, N, insulated="x-", convective={"y-": 0.5}, ambient=0.25, extra_args=["--temporal", "1"])
    m = s.model
    rng = np.random.default_rng(8)
    T0 = rng.uniform(0.0, 1.0, N)
    c, rc, q = m.layered_conductivity(0.25, 1.0), m.layered_capacity(1.0, 8.0), rng.uniform(-50.0, 50.0, N)
    s.set_field(T0)
    s.set_conductivity(c)
    s.set_source(q)
    s.set_capacity(rc)
    T = torch.from_numpy(s.gather().copy())
    ch, S, sv = torch.from_numpy(0.5 * c), torch.from_numpy(m.dt * q), torch.from_numpy(1.0 / rc)
    for k in range(5):
        s.step(1)
        s.synchronize()
        T = _definition_step(T, ch, S, sv, m.D, 0.5, 0.25)
        got = s.gather()
        assert np.array_equal(got[1:-1, 1:-1, 1:-1], T[1:-1, 1:-1, 1:-1].numpy()), f"step {k}"
