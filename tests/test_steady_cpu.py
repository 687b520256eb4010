"""The direct steady-state solve on the CPU backend, the oracle of the gfx950
path (tests/test_gpu_steady.py runs the same cases there): the definitions of
the three operations (fsum bound of the dot products, symmetry of A), the solve
against the exact discrete steady states, decompositions, processes, the state
after a solve, usage errors and the CLI.  Bounds: tests/_steady_cases.py."""
import json
import math

import numpy as np
import pytest
import torch.multiprocessing as mp

import _steady_cases as sc
from conftest import free_port, run_cli
from _steady_workers import steady_cpu_worker

CPU = "cpu"


@pytest.mark.parametrize("form", list(sc.FORMS))
@pytest.mark.parametrize("N", sc.SHAPES)
def test_dot_products_and_symmetry(h3d, N, form):
    """p . A p and r . r within 2^-52 fsum|terms| of fsum, the same bits twice;
    p . (A q) == q . (A p) to 2^-50 fsum|terms|."""
    from heat3d_amd import ops

    D = sc.physics_D(h3d, N)
    a, b = sc.random_fields(N, 11, 2)
    kw = sc.form_fields(h3d, N, form, CPU)
    p, q = sc.padded(h3d, N, a, CPU), sc.padded(h3d, N, b, CPU)
    Ap, Aq = sc.padded(h3d, N, 0 * a, CPU), sc.padded(h3d, N, 0 * a, CPU)
    hi, lo = ops.steady_apply(p, Ap, D, **kw)
    assert (hi, lo) == ops.steady_apply(p, Ap, D, **kw)
    ref, sabs = sc.fsum_bound(sc.owned_np(p), sc.owned_np(Ap))
    print(f"{N} {form}: p.Ap {hi + lo!r} fsum {ref!r} diff {abs(hi + lo - ref):.3e} bound {sc.EPS * sabs:.3e}")
    assert abs((hi + lo) - ref) <= sc.EPS * sabs
    assert hi + lo > 0.0  # A is positive definite
    ops.steady_apply(q, Aq, D, **kw)
    l, sl = sc.fsum_bound(sc.owned_np(p), sc.owned_np(Aq))
    r, sr = sc.fsum_bound(sc.owned_np(q), sc.owned_np(Ap))
    print(f"  p.Aq {l!r} q.Ap {r!r} diff {abs(l - r):.3e} bound {4 * sc.EPS * max(sl, sr):.3e}")
    assert abs(l - r) <= 4 * sc.EPS * max(sl, sr)
    # the update's r . r
    x, rr = sc.padded(h3d, N, a, CPU), sc.padded(h3d, N, b, CPU)
    hi, lo = ops.steady_update(x, p, rr, Ap, 0.375)
    ref, sabs = sc.fsum_bound(sc.owned_np(rr), sc.owned_np(rr))
    assert abs((hi + lo) - ref) <= sc.EPS * sabs
    # one fused multiply-add per point: within half an ulp of the exact a + 0.375 p
    assert np.allclose(sc.owned_np(x), a[1:-1, 1:-1, 1:-1] + 0.375 * sc.owned_np(p), rtol=0, atol=2 * sc.EPS)


def test_apply_is_the_negated_homogeneous_step(h3d):
    """A p against NumPy on the uniform form: -(Dx dxx + Dy dyy + Dz dzz) p with
    zero walls, to rounding; the residual form is the increment of one step."""
    from heat3d_amd import ops

    N = (18, 21, 67)
    D = sc.physics_D(h3d, N)
    (a,) = sc.random_fields(N, 5, 1)
    p, Ap = sc.padded(h3d, N, a, CPU), sc.padded(h3d, N, 0 * a, CPU)
    ops.steady_apply(p, Ap, D)
    z = a.copy()
    z[0], z[-1], z[:, 0], z[:, -1], z[:, :, 0], z[:, :, -1] = 0, 0, 0, 0, 0, 0
    c = z[1:-1, 1:-1, 1:-1]
    lap = (D[0] * (z[2:, 1:-1, 1:-1] - 2 * c + z[:-2, 1:-1, 1:-1]) + D[1] * (z[1:-1, 2:, 1:-1] - 2 * c + z[1:-1, :-2, 1:-1])
           + D[2] * (z[1:-1, 1:-1, 2:] - 2 * c + z[1:-1, 1:-1, :-2]))
    assert np.allclose(sc.owned_np(Ap), -lap, rtol=0, atol=64 * sc.EPS)
    # residual form: G(T) - T of the time stepper
    r = sc.padded(h3d, N, 0 * a, CPU)
    ops.steady_apply(p, r, D, residual=True)
    out = sc.padded(h3d, N, a, CPU)
    ops.ftcs_step(p, out, D)
    assert np.allclose(sc.owned_np(r), sc.owned_np(out) - sc.owned_np(p), rtol=0, atol=8 * sc.EPS)


@pytest.mark.parametrize("name", ["reference33", "reference17x33x65", "sine_source", "layered", "convective_slab",
                                  "open_form"])
def test_solve_reaches_the_steady_state(h3d, name):
    sc.solve_and_check(h3d, name, CPU)


@pytest.mark.parametrize("ranks", [2, 8])
def test_decompositions(h3d, ranks):
    decomp = (2, 1, 1) if ranks == 2 else (2, 2, 2)
    _, single, _ = sc.solve_and_check(h3d, "sine_source", CPU)
    _, r, T = sc.solve_and_check(h3d, "sine_source", CPU, virtual_ranks=ranks, decomp=decomp)
    assert abs(r["iterations"] - single["iterations"]) <= 2
    _, r2, T2 = sc.solve_and_check(h3d, "sine_source", CPU, virtual_ranks=ranks, decomp=decomp)
    assert np.array_equal(T, T2)
    assert {k: v for k, v in r.items() if k != "seconds"} == {k: v for k, v in r2.items() if k != "seconds"}


def test_thread_count_does_not_change_the_bits(h3d):
    _, r1, T1 = sc.solve_and_check(h3d, "open_form", CPU, threads=1)
    _, r3, T3 = sc.solve_and_check(h3d, "open_form", CPU, threads=3)
    assert np.array_equal(T1, T3) and r1["iterations"] == r3["iterations"]


def test_two_processes(h3d, tmp_path):
    """Two processes over the socket transport: the (hi, lo) pairs are all-reduced."""
    mp.start_processes(steady_cpu_worker, args=(2, free_port(), str(tmp_path), "sine_source", (1, 1, 2)), nprocs=2,
                       join=True, start_method="spawn")
    got = [json.loads((tmp_path / f"steady{r}.json").read_text()) for r in range(2)]
    assert got[0] == got[1]
    _, single, _ = sc.solve_and_check(h3d, "sine_source", CPU)
    assert abs(got[0]["iterations"] - single["iterations"]) <= 2


def test_state_after_a_solve(h3d, tmp_path):
    """The solution is the state of iteration 0: the heat balance is finite, a
    checkpoint restarts to the same field, and run() goes on from it without a
    fault.  (run() measures its residual against its own first one, so it does
    not stop at once on a solved field; its residuals stay at the solve's.)"""
    s, r, T = sc.solve_and_check(h3d, "convective_slab", CPU)
    s2, exact, _ = sc.make_solver(h3d, "convective_slab", CPU)
    s2.solve_steady(sc.TOL, sc.CAP)
    assert s2.state()["iter"] == 0
    b = s2.heat_balance()
    assert math.isfinite(b["imbalance"]) and b["nonfinite"] == 0
    # the wall planes show what they show after time steps: the insulated sides mirror
    G = s2.gather()
    assert np.array_equal(G[0, 1:-1, 1:-1], G[1, 1:-1, 1:-1])
    s2.save_checkpoint(str(tmp_path / "ck"))
    s3, _, _ = sc.make_solver(h3d, "convective_slab", CPU)
    s3.load_checkpoint(str(tmp_path / "ck"))
    assert np.array_equal(s3.gather(), G)
    out = s2.run()
    assert not out["fault"]
    assert s2.state()["last_residual"] <= sc.TOL * r["r0_norm"] + 4 * sc.EPS


def test_initial_guess_is_the_current_field(h3d):
    """set_field gives the initial guess: near the steady state the initial
    residual is small in proportion, and the same solve returns the same bits."""
    s, exact, _ = sc.make_solver(h3d, "layered", CPU)
    far = s.solve_steady(1e-6, sc.CAP)
    near = exact.copy()
    near[1:-1, 1:-1, 1:-1] += 1e-6 * np.random.default_rng(2).uniform(-1, 1, near[1:-1, 1:-1, 1:-1].shape)
    s.set_field(near)
    first = s.solve_steady(1e-6, sc.CAP)
    T1 = s.gather()
    s.set_field(near)
    r = s.solve_steady(1e-6, sc.CAP)
    assert r == dict(first, seconds=r["seconds"]) and np.array_equal(T1, s.gather())
    assert r["converged"] and r["r0_norm"] < 1e-4 * far["r0_norm"]
    assert np.abs(T1 - exact).max() < 1e-6


def test_usage_errors(h3d):
    with pytest.raises(Exception, match="fp64"):
        h3d.HeatSolver((9, 9, 9), 10, 1e-5, backend=CPU, dtype="fp32").solve_steady()
    with pytest.raises(Exception, match="compat"):
        h3d.HeatSolver((9, 9, 9), 10, 1e-5, backend=CPU, extra_args=["--compat"]).solve_steady()
    with pytest.raises(Exception, match="singular"):
        h3d.HeatSolver((9, 9, 9), 10, 1e-5, backend=CPU, insulated="all").solve_steady()
    with pytest.raises(Exception, match="singular"):
        h3d.HeatSolver((9, 9, 9), 10, 1e-5, backend=CPU, insulated="x-,x+,y-,y+,z-", convective={"z+": 0.0}).solve_steady()
    s = h3d.HeatSolver((9, 9, 9), 10, 1e-5, backend=CPU)
    for tol in (0.0, -1e-8, float("nan")):
        with pytest.raises(Exception, match="tolerance"):
            s.solve_steady(tol)


def test_cli(heat3d_bin, tmp_path):
    out = tmp_path / "r.json"
    p = run_cli([33, 33, 33, 1000, "1e-10", "--steady-solve", "--backend", "cpu", "--json-out", out], tmp_path)
    assert p.returncode == 0, p.stderr
    assert "Steady solve (conjugate gradients) has converged in 123 iterations" in p.stdout, p.stdout
    assert "heat3d: steady solve: status=converged restarts=0" in p.stdout
    j = json.loads(out.read_text())["steady_solve"]
    assert j["converged"] is True and j["iterations"] == 123 and j["true_residual"] <= 1e-10
    for key in ("residual", "r0_norm", "seconds", "restarts", "status"):
        assert key in j
    assert "--steady-solve" in run_cli(["--help"], tmp_path).stdout
    for bad in (["--dtype", "fp32"], ["--compat"], ["--insulated", "all"]):
        q = run_cli([9, 9, 9, 10, "1e-8", "--steady-solve", "--backend", "cpu"] + bad, tmp_path)
        assert q.returncode != 0 and "--steady-solve" in q.stderr, (bad, q.stderr)
    q = run_cli([9, 9, 9, 10, "0", "--steady-solve", "--backend", "cpu"], tmp_path)
    assert q.returncode != 0
