"""Implicit time steps (backward Euler / Crank-Nicolson by conjugate gradients,
docs/ARCHITECTURE.md "Implicit steps") on the CPU backend: the shifted operator
against the existing one, and whole steps against checks that use the existing
residual form and NumPy only.  Bounds: tests/_implicit_checks.py."""
import json
import math

import numpy as np
import pytest
import torch.multiprocessing as mp

import _implicit_checks as ic
import _steady_cases as sc
from conftest import free_port
from _implicit_workers import implicit_cpu_worker

CPU = "cpu"
CASES = ["reference33", "reference17x33x65", "sine_source", "layered", "convective_slab", "open_form"]


def _bits(f):
    return f.flat.cpu().numpy().view(np.int64)


@pytest.mark.parametrize("cap", [False, True])
@pytest.mark.parametrize("form", list(sc.FORMS))
@pytest.mark.parametrize("N", sc.SHAPES)
def test_shifted_operator(h3d, N, form, cap):
    """M p = (R + mu A) p agrees pointwise with p / s + mu (A p) from the existing
    operator within 2 * 2^-52 (|p / s| + |mu A p|); p . M q == q . M p within the
    fsum bound of tests/test_gpu_steady.py; M with mu = 1 and R = I is p + A p
    rounded once, which ties the shifted form bitwise to the default output (that
    the default output itself keeps its bits is what the existing steady tests
    pin; passing shift=None explicitly is only checked to be the same call)."""
    from heat3d_amd import ops

    D = sc.physics_D(h3d, N)
    mu = 37.5
    a, b = sc.random_fields(N, 11, 2)
    k = sc.form_fields(h3d, N, form, CPU)
    sv = np.random.default_rng(13).uniform(2.0 ** -10, 1.0, N)
    kc = dict(k, cap=sc.padded(h3d, N, sv, CPU)) if cap else dict(k)
    p, q = sc.padded(h3d, N, a, CPU), sc.padded(h3d, N, b, CPU)
    Ap, Mp, Mq = (sc.padded(h3d, N, 0 * a, CPU) for _ in range(3))
    ops.steady_apply(p, Ap, D, **k)
    dot = ops.steady_apply(p, Mp, D, shift=mu, **kc)
    ops.steady_apply(q, Mq, D, shift=mu, **kc)
    pv, Apv, Mpv = sc.owned_np(p), sc.owned_np(Ap), sc.owned_np(Mp)
    ps = pv / sv[1:-1, 1:-1, 1:-1] if cap else pv
    excess = np.abs(Mpv - (ps + mu * Apv)) - 2 * sc.EPS * (np.abs(ps) + np.abs(mu * Apv))
    print(f"{N} {form} cap {cap}: worst excess over the pointwise bound {excess.max():.3e}")
    assert (excess <= 0).all()
    ref, sabs = sc.fsum_bound(pv, Mpv)
    assert abs(dot[0] + dot[1] - ref) <= sc.EPS * sabs
    l, sl = sc.fsum_bound(pv, sc.owned_np(Mq))
    r, sr = sc.fsum_bound(sc.owned_np(q), Mpv)
    print(f"  p.Mq {l!r} q.Mp {r!r} diff {abs(l - r):.3e} bound {4 * sc.EPS * max(sl, sr):.3e}")
    assert abs(l - r) <= 4 * sc.EPS * max(sl, sr)
    # the default is the unshifted operator
    again, one = sc.padded(h3d, N, 0 * a, CPU), sc.padded(h3d, N, 0 * a, CPU)
    ops.steady_apply(p, again, D, shift=None, cap=None, **k)
    assert np.array_equal(_bits(again), _bits(Ap))
    ops.steady_apply(p, one, D, shift=1.0, **k)
    assert np.array_equal(sc.owned_np(one), pv + Apv)
    with pytest.raises(ValueError):
        ops.steady_apply(p, one, D, shift=1.0, residual=True, **k)
    with pytest.raises(ValueError):
        ops.steady_apply(p, one, D, cap=sc.padded(h3d, N, sv, CPU), **k)


def test_helper_operations(h3d):
    """r -= q with r . r (steady_update without x) and T' = fma(m, d, T)
    (steady_update without r): NumPy's single roundings."""
    from heat3d_amd import ops

    N = (18, 21, 67)
    r0, q0, T0, d0 = sc.random_fields(N, 29, 4)
    r, q, T, d = (sc.padded(h3d, N, f, CPU) for f in (r0, q0, T0, d0))
    dot = ops.steady_update(None, None, r, q, 1.0)
    want = (r0 - q0)[1:-1, 1:-1, 1:-1]
    assert np.array_equal(sc.owned_np(r), want) and np.array_equal(sc.owned_np(q), q0[1:-1, 1:-1, 1:-1])
    ref, sabs = sc.fsum_bound(want, want)
    assert abs(dot[0] + dot[1] - ref) <= sc.EPS * sabs
    m = 64.0  # (a power of two: m d is exact, so fma(m, d, T) is NumPy's m * d + T)
    assert ops.steady_update(T, d, None, None, m) == (0.0, 0.0)
    assert np.array_equal(sc.owned_np(T), (m * d0 + T0)[1:-1, 1:-1, 1:-1])
    assert np.array_equal(sc.owned_np(d), d0[1:-1, 1:-1, 1:-1])
    with pytest.raises(ValueError):
        ops.steady_update(T, None, r, q, 1.0)


@pytest.mark.parametrize("cap", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_defect_of_a_step(h3d, name, cap):
    """e = R (T' - T) / m - theta r(T') - (1 - theta) r(T), evaluated on the host
    with the existing residual form, is minus the CG residual:
    ||e|| <= tol r0_norm + 2^-40 (||R (T' - T) / m|| + ||r(T')|| + ||r(T)||)."""
    case = ic.make_case(h3d, name, CPU, cap=cap)
    T0 = case.s.gather()
    print(f"{name} cap {cap}")
    for m in ic.MS:
        for theta in ic.THETAS:
            ic.check_defect(case, m, theta, T0)


@pytest.mark.parametrize("theta", ic.THETAS)
@pytest.mark.parametrize("m", ic.MS)
def test_exact_mode_factor(h3d, m, theta):
    ic.check_mode_factor(h3d, CPU, m, theta)


def test_implicit_factor_is_the_explicit_one_at_theta_0(h3d):
    mdl = h3d.HeatEquation3D(ic.MODE_N)
    _, g = mdl.dirichlet_mode(ic.MODE_VEC, s=0.25)
    assert abs(mdl.implicit_factor(ic.MODE_VEC, 1.0, 0.0, s=0.25) - g) <= 2 * sc.EPS


@pytest.mark.parametrize("theta", ic.THETAS)
def test_heat_balance_identity(h3d, theta):
    case = ic.balance_case(h3d, CPU)
    got = ic.check_balance_identity(case, 16.0, theta, steps=2)
    assert abs(got[0][0]) > 100 * got[0][1]  # the identity says something


def test_weighted_heat_is_conserved_with_every_face_insulated(h3d):
    """No source, every face insulated (a mode solve_steady refuses): sum rc T
    moves by the identity's bound only, over 5 steps."""
    N = (11, 9, 14)
    s = h3d.HeatSolver(N, 100, 1e-5, backend=CPU, dtype="fp64", insulated="all")
    s.initialize()
    s.set_field(np.random.default_rng(4).uniform(0.0, 1.0, N))
    rc = s.model.layered_capacity(1.0, 8.0)
    s.set_capacity(rc)
    case = ic.Case(h3d, s, N, dict(insulated="all"), rc=rc)
    T0 = s.gather()
    got = ic.check_balance_identity(case, 16.0, 1.0, steps=5)
    assert all(abs(dheat) <= bound for dheat, bound, _ in got)
    assert ic.norm(s.gather() - T0) > 1.0  # (the field itself moved)


@pytest.mark.parametrize("name", ["reference33", "sine_source"])
def test_large_step_is_the_steady_state(h3d, name):
    """theta = 1, m = 1e9: one step lands on the exact steady field within the
    bound of _steady_cases.solve_and_check, kappa_hat * tol * the initial error."""
    case = ic.make_case(h3d, name, CPU)
    T0 = case.s.gather()
    r = case.s.step_implicit(1, 1e9, 1.0, tol=sc.TOL, max_iter=sc.CAP)
    assert r["converged"], r
    kappa = 6.0 * (max(case.N) - 1) ** 2
    err = ic.norm((case.s.gather() - case.exact)[1:-1, 1:-1, 1:-1])
    err0 = ic.norm((T0 - case.exact)[1:-1, 1:-1, 1:-1])
    print(f"{name}: {r['iterations']} iterations, error {err:.3e} bound {kappa * sc.TOL * err0:.3e}")
    assert err <= kappa * sc.TOL * err0


def _run(h3d, name, m, theta, steps=1, **extra):
    case = ic.make_case(h3d, name, CPU, cap=True, **extra)
    r = case.s.step_implicit(steps, m, theta, tol=ic.TOL)
    return r, case.s.gather()


@pytest.mark.parametrize("m,theta", [(64.0, 1.0), (4096.0, 0.5)])
def test_determinism_and_decompositions(h3d, m, theta):
    r1, T1 = _run(h3d, "open_form", m, theta, steps=2)
    r2, T2 = _run(h3d, "open_form", m, theta, steps=2)
    assert r1["converged"] and ic.report(r1) == ic.report(r2) and np.array_equal(T1, T2)
    _, T3 = _run(h3d, "open_form", m, theta, steps=2, threads=3)
    assert np.array_equal(T1, T3)
    one, To = _run(h3d, "open_form", m, theta)
    for ranks, decomp in ((2, (2, 1, 1)), (8, (2, 2, 2))):
        r, T = _run(h3d, "open_form", m, theta, virtual_ranks=ranks, decomp=decomp)
        assert r["converged"] and abs(r["iterations"] - one["iterations"]) <= 2
        ic.fields_agree(T, To, m, one["r0_norm"], f"{ranks} virtual ranks")


def test_two_processes(h3d, tmp_path):
    m, theta = 64.0, 0.5
    mp.start_processes(implicit_cpu_worker, args=(2, free_port(), str(tmp_path), "open_form", (1, 1, 2), m, theta),
                       nprocs=2, join=True, start_method="spawn")
    got = [json.loads((tmp_path / f"implicit{r}.json").read_text()) for r in range(2)]
    assert got[0] == got[1] and got[0]["converged"] and got[0]["steps_done"] == 1
    one, To = _run(h3d, "open_form", m, theta)
    assert abs(got[0]["iterations"] - one["iterations"]) <= 2
    ic.fields_agree(np.load(tmp_path / "field.npy"), To, m, one["r0_norm"], "two processes")


def test_state_after_steps(h3d, tmp_path):
    """The result is the state of iteration 0: run(), step(), gather() and a
    checkpoint round trip work on it, and solve_steady keeps its bits."""
    before, _, _ = sc.make_solver(h3d, "convective_slab", CPU)
    rb = before.solve_steady(sc.TOL, sc.CAP)
    Tb = before.gather()

    case = ic.make_case(h3d, "convective_slab", CPU, cap=True)
    s = case.s
    T0 = s.gather()
    r = s.step_implicit(3, 32.0, 1.0, tol=ic.TOL)
    assert r["converged"] and r["steps_done"] == 3 and len(r["step_iterations"]) == 3
    assert r["time_advanced"] == 96.0 and r["iterations"] == sum(r["step_iterations"])
    assert s.state()["iter"] == 0
    G = s.gather()
    assert np.array_equal(G[0, 1:-1, 1:-1], G[1, 1:-1, 1:-1])  # (the insulated sides mirror)
    b = s.heat_balance()
    assert math.isfinite(b["imbalance"]) and b["nonfinite"] == 0
    s.save_checkpoint(str(tmp_path / "ck"))
    s3 = ic.make_case(h3d, "convective_slab", CPU, cap=True).s
    s3.load_checkpoint(str(tmp_path / "ck"))
    assert np.array_equal(s3.gather(), G)
    s.step(2)
    s.synchronize()
    assert s.state()["iter"] == 2 and not np.array_equal(s.gather(), G)
    out = s.run()
    assert not out["fault"]
    # solve_steady after implicit steps: from the same field, the bits it had before
    s.clear_capacity()
    s.set_field(T0)
    ra = s.solve_steady(sc.TOL, sc.CAP)
    assert ic.report(ra) == ic.report(rb) and np.array_equal(s.gather(), Tb)


def test_breakdown_and_steady_field(h3d):
    case = ic.make_case(h3d, "reference33", CPU)
    s = case.s
    # a steady field: no iteration, the bits stay
    s.set_field(case.exact)
    T = s.gather()
    r = s.step_implicit(2, 100.0, 0.5, tol=ic.TOL)
    print(r)
    assert r["converged"] and r["status"] == "converged" and r["iterations"] == 0 and r["steps_done"] == 2
    assert np.array_equal(s.gather().view(np.int64), T.view(np.int64))
    # a NaN in the field: breakdown, the field unchanged, no step done
    s.set_field(np.random.default_rng(1).uniform(0.0, 1.0, case.N))
    s.native.inject(0, 4, 5, 6, float("nan"))  # (local owned coordinates: global point 5, 6, 7)
    T = s.gather()
    assert np.isnan(T[5, 6, 7]) and np.isnan(T).sum() == 1
    r = s.step_implicit(3, 8.0, 1.0, tol=ic.TOL)
    print(r)
    assert r["status"] == "breakdown" and not r["converged"] and r["steps_done"] == 0 and r["time_advanced"] == 0.0
    assert np.array_equal(s.gather().view(np.int64), T.view(np.int64))
    # the cap: the step is applied, reported unconverged, and the call ends there
    s.set_field(np.random.default_rng(1).uniform(0.0, 1.0, case.N))
    r = s.step_implicit(3, 4096.0, 1.0, tol=1e-12, max_iter=3)
    print(r)
    assert r["status"] == "max_iter" and not r["converged"] and r["steps_done"] == 1 and r["iterations"] == 3


def test_usage_errors(h3d):
    with pytest.raises(Exception, match="fp64"):
        h3d.HeatSolver((9, 9, 9), 10, 1e-5, backend=CPU, dtype="fp32").step_implicit(1, 2.0)
    with pytest.raises(Exception, match="compat"):
        h3d.HeatSolver((9, 9, 9), 10, 1e-5, backend=CPU, extra_args=["--compat"]).step_implicit(1, 2.0)
    s = h3d.HeatSolver((9, 9, 9), 10, 1e-5, backend=CPU)
    for m in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(Exception, match="positive and finite"):
            s.step_implicit(1, m)
    for theta in (0.0, 0.49, 1.01, float("nan")):
        with pytest.raises(Exception, match="theta"):
            s.step_implicit(1, 2.0, theta)
    for tol in (0.0, -1e-8, float("nan"), float("inf")):
        with pytest.raises(Exception, match="tolerance"):
            s.step_implicit(1, 2.0, 1.0, tol)
    with pytest.raises(Exception, match="negative"):
        s.step_implicit(-1, 2.0)
    r = s.step_implicit(0, 2.0)
    assert r["steps_done"] == 0 and r["converged"] and r["status"] == "converged"
