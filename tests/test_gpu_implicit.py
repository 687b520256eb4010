"""Implicit time steps on gfx950: the shifted operator and the two helper
operations of csrc/kernels/steady_cg.hip against the CPU definitions, through
ops, and the solver-level checks of tests/test_implicit_cpu.py on the HIP
backend.  Bounds: tests/_implicit_checks.py."""
import json

import numpy as np
import pytest
import torch.multiprocessing as mp

import _implicit_checks as ic
import _steady_cases as sc
from conftest import free_port
from _implicit_workers import implicit_gpu_worker

pytestmark = pytest.mark.gpu


def _both(h3d, gpu, N, arr):
    return sc.padded(h3d, N, arr, "cpu"), sc.padded(h3d, N, arr, gpu)


def _bits(f):
    return f.flat.cpu().numpy().view(np.int64)


@pytest.mark.parametrize("box", ["whole", "sub"])
@pytest.mark.parametrize("cap", [False, True])
@pytest.mark.parametrize("form", list(sc.FORMS))
@pytest.mark.parametrize("N", sc.SHAPES)
def test_shifted_apply_bitwise_and_dots(h3d, gpu, N, form, cap, box):
    """q = (R + mu A) p is bitwise the CPU's (67 crosses a 64-lane z tile, 21 is no
    multiple of the 4-row tile, 5 is the thin box), on the whole block and on a
    sub-box with walls on some sides only; p . q is within 2^-52 fsum|terms| of
    fsum and the same bits twice."""
    from heat3d_amd import ops

    n = [v - 2 for v in N]
    D = sc.physics_D(h3d, N)
    mu = 37.5
    (a,) = sc.random_fields(N, 11, 1)
    sv = np.random.default_rng(13).uniform(2.0 ** -10, 1.0, N)
    bx = None if box == "whole" else sc.sub_box(n)
    kc, kg = sc.form_fields(h3d, N, form, "cpu"), sc.form_fields(h3d, N, form, gpu)
    if cap:
        kc["cap"], kg["cap"] = _both(h3d, gpu, N, sv)
    if box == "sub":  # an inner side: the block's high z side is not a wall
        wall = [0, n[0] - 1, 0, n[1] - 1, 0, h3d.native().NO_WALL]
        kc["wall"], kg["wall"] = wall, wall
    pc, pg = _both(h3d, gpu, N, a)
    qc, qg = _both(h3d, gpu, N, 0 * a)
    dc = ops.steady_apply(pc, qc, D, box=bx, shift=mu, **kc)
    dg = ops.steady_apply(pg, qg, D, box=bx, shift=mu, **kg)
    assert np.array_equal(_bits(qc), _bits(qg))
    assert dg == ops.steady_apply(pg, qg, D, box=bx, shift=mu, **kg)
    ref, sabs = sc.fsum_bound(sc.owned_np(pc, bx), sc.owned_np(qc, bx))
    print(f"{N} {form} cap {cap} {box}: gpu {dg[0] + dg[1]!r} cpu {dc[0] + dc[1]!r} fsum {ref!r} bound {sc.EPS * sabs:.3e}")
    assert abs(dg[0] + dg[1] - ref) <= sc.EPS * sabs
    assert abs(dc[0] + dc[1] - ref) <= sc.EPS * sabs


@pytest.mark.parametrize("box", ["whole", "sub"])
@pytest.mark.parametrize("N", sc.SHAPES)
def test_helper_operations_bitwise(h3d, gpu, N, box):
    """r -= q with r . r and T' = fma(m, d, T): the CPU's bits, the fsum bound, the same pair twice."""
    from heat3d_amd import ops

    n = [v - 2 for v in N]
    bx = None if box == "whole" else sc.sub_box(n)
    fields = sc.random_fields(N, 31, 4)
    (rc, rg), (qc, qg), (Tc, Tg), (dc, dg) = (_both(h3d, gpu, N, f) for f in fields)
    pc = ops.steady_update(None, None, rc, qc, 1.0, box=bx)
    pg = ops.steady_update(None, None, rg, qg, 1.0, box=bx)
    assert np.array_equal(_bits(rc), _bits(rg)) and np.array_equal(_bits(qc), _bits(qg))
    ref, sabs = sc.fsum_bound(sc.owned_np(rg, bx), sc.owned_np(rg, bx))
    assert abs(pg[0] + pg[1] - ref) <= sc.EPS * sabs and abs(pc[0] + pc[1] - ref) <= sc.EPS * sabs
    r2, q2 = sc.padded(h3d, N, fields[0], gpu), sc.padded(h3d, N, fields[1], gpu)
    assert pg == ops.steady_update(None, None, r2, q2, 1.0, box=bx)
    m = 0.3721e3
    ops.steady_update(Tc, dc, None, None, m, box=bx)
    ops.steady_update(Tg, dg, None, None, m, box=bx)
    assert np.array_equal(_bits(Tc), _bits(Tg)) and np.array_equal(_bits(dc), _bits(dg))


@pytest.mark.parametrize("name,cap", [("reference33", True), ("reference17x33x65", False), ("open_form", True)])
def test_defect_of_a_step(h3d, gpu, name, cap):
    """The defect check of tests/test_implicit_cpu.py on the HIP backend, every m
    and theta; against the CPU backend from the same field the iteration counts
    are within 2 and the fields agree to the tolerance; the same call twice
    returns the same bits."""
    cpu, hip = ic.make_case(h3d, name, "cpu", cap=cap), ic.make_case(h3d, name, "hip", cap=cap)
    assert hip.s.backend == "hip"
    T0 = cpu.s.gather()
    assert np.array_equal(T0, hip.s.gather())
    print(f"{name} cap {cap}")
    for m in ic.MS:
        for theta in ic.THETAS:
            rc, _, Tc = ic.check_defect(cpu, m, theta, T0)
            rg, _, Tg = ic.check_defect(hip, m, theta, T0)
            assert abs(rg["iterations"] - rc["iterations"]) <= 2
            ic.fields_agree(Tg, Tc, m, rc["r0_norm"], "hip against cpu")
            hip.s.set_field(T0)
            r2 = hip.s.step_implicit(1, m, theta, tol=ic.TOL)
            assert ic.report(r2) == ic.report(rg) and np.array_equal(hip.s.gather(), Tg)


@pytest.mark.parametrize("m,theta", [(1.0, 0.5), (64.0, 1.0), (4096.0, 0.5)])
def test_exact_mode_factor(h3d, gpu, m, theta):
    rg, Tg = ic.check_mode_factor(h3d, "hip", m, theta)
    rc, Tc = ic.check_mode_factor(h3d, "cpu", m, theta)
    assert abs(rg["iterations"] - rc["iterations"]) <= 2
    ic.fields_agree(Tg, Tc, m, rc["r0_norm"], "hip against cpu")


@pytest.mark.parametrize("theta", ic.THETAS)
@pytest.mark.parametrize("N", [(33, 33, 33), (17, 33, 65)])
def test_heat_balance_identity(h3d, gpu, N, theta):
    """A source, a conductivity, mixed walls and a layered capacity: the balance
    identity on the HIP backend, step by step; against the CPU backend after the
    first step the iteration counts are within 2 and the fields agree to
    10 m tol r0_norm."""
    m = 16.0
    hip, cpu = ic.balance_case(h3d, "hip", N), ic.balance_case(h3d, "cpu", N)
    assert hip.s.backend == "hip"
    (dheat, bound, rg), = ic.check_balance_identity(hip, m, theta)
    assert abs(dheat) > 100 * bound
    (_, _, rc), = ic.check_balance_identity(cpu, m, theta)
    assert abs(rg["iterations"] - rc["iterations"]) <= 2
    ic.fields_agree(hip.s.gather(), cpu.s.gather(), m, rc["r0_norm"], "hip against cpu")
    ic.check_balance_identity(hip, m, theta)


def test_every_face_insulated_conserves_the_weighted_heat(h3d, gpu):
    N = (33, 33, 33)
    s = h3d.HeatSolver(N, 100, 1e-5, backend="hip", device=0, dtype="fp64", insulated="all")
    s.initialize()
    s.set_field(np.random.default_rng(4).uniform(0.0, 1.0, N))
    rc = s.model.layered_capacity(1.0, 8.0)
    s.set_capacity(rc)
    got = ic.check_balance_identity(ic.Case(h3d, s, N, dict(insulated="all"), rc=rc), 16.0, 1.0, steps=5)
    assert all(abs(dheat) <= bound for dheat, bound, _ in got)


def _run(h3d, m, theta, **extra):
    case = ic.make_case(h3d, "open_form", "hip", cap=True, **extra)
    r = case.s.step_implicit(1, m, theta, tol=ic.TOL)
    return r, case.s.gather()


@pytest.mark.parametrize("ranks", [2, 8])
def test_decompositions(h3d, gpu, ranks):
    m, theta = 256.0, 0.5
    decomp = (2, 1, 1) if ranks == 2 else (2, 2, 2)
    one, To = _run(h3d, m, theta)
    r, T = _run(h3d, m, theta, virtual_ranks=ranks, decomp=decomp)
    assert r["converged"] and abs(r["iterations"] - one["iterations"]) <= 2
    ic.fields_agree(T, To, m, one["r0_norm"], f"{ranks} virtual ranks")
    r2, T2 = _run(h3d, m, theta, virtual_ranks=ranks, decomp=decomp)
    assert ic.report(r2) == ic.report(r) and np.array_equal(T, T2)


def test_two_processes_one_gpu(h3d, gpu, tmp_path):
    m, theta = 256.0, 0.5
    mp.start_processes(implicit_gpu_worker, args=(2, free_port(), str(tmp_path), "open_form", (2, 1, 1), m, theta),
                       nprocs=2, join=True, start_method="spawn")
    got = [json.loads((tmp_path / f"implicit{r}.json").read_text()) for r in range(2)]
    assert got[0] == got[1] and got[0]["converged"]
    one, To = _run(h3d, m, theta)
    assert abs(got[0]["iterations"] - one["iterations"]) <= 2
    ic.fields_agree(np.load(tmp_path / "field.npy"), To, m, one["r0_norm"], "two processes")


def test_state_breakdown_and_steady_field(h3d, gpu):
    case = ic.make_case(h3d, "reference33", "hip")
    s = case.s
    s.set_field(case.exact)
    T = s.gather()
    r = s.step_implicit(2, 100.0, 0.5, tol=ic.TOL)
    assert r["converged"] and r["iterations"] == 0 and r["steps_done"] == 2 and s.state()["iter"] == 0
    assert np.array_equal(s.gather().view(np.int64), T.view(np.int64))
    s.set_field(np.random.default_rng(1).uniform(0.0, 1.0, case.N))
    s.native.inject(0, 4, 5, 6, float("nan"))
    T = s.gather()
    r = s.step_implicit(3, 8.0, 1.0, tol=ic.TOL)
    assert r["status"] == "breakdown" and not r["converged"] and r["steps_done"] == 0
    assert np.array_equal(s.gather().view(np.int64), T.view(np.int64))
    s.set_field(np.random.default_rng(1).uniform(0.0, 1.0, case.N))
    r = s.step_implicit(2, 32.0, 1.0, tol=ic.TOL)
    assert r["converged"] and s.state()["iter"] == 0
    s.step(2)
    s.synchronize()
    assert s.state()["iter"] == 2
    with pytest.raises(Exception, match="fp64"):
        h3d.HeatSolver((9, 9, 9), 10, 1e-5, backend="hip", device=0, dtype="fp32").step_implicit(1, 2.0)
    with pytest.raises(Exception, match="theta"):
        s.step_implicit(1, 2.0, 0.25)
