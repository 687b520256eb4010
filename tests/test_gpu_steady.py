"""The direct steady-state solve on gfx950 (csrc/kernels/steady_cg.hip) against
the CPU definitions, through ops, and the solver-level cases of
tests/test_steady_cpu.py on the HIP backend.  Bounds: tests/_steady_cases.py."""
import json
import math

import numpy as np
import pytest
import torch.multiprocessing as mp

import _steady_cases as sc
from conftest import free_port
from _steady_workers import steady_gpu_worker

pytestmark = pytest.mark.gpu


def _both(h3d, gpu, N, arr):
    return sc.padded(h3d, N, arr, "cpu"), sc.padded(h3d, N, arr, gpu)


def _bits(f):
    return f.flat.cpu().numpy().view(np.int64)


@pytest.mark.parametrize("box", ["whole", "sub"])
@pytest.mark.parametrize("form", list(sc.FORMS))
@pytest.mark.parametrize("N", sc.SHAPES)
def test_apply_bitwise_and_dots(h3d, gpu, N, form, box):
    """q = A p on random p (random wall vertices too) is bitwise the CPU's, on the
    whole block and on a sub-box with walls on some sides only; p . q is within
    2^-52 fsum|terms| of fsum and the same bits twice; p . A q == q . A p."""
    from heat3d_amd import ops

    n = [v - 2 for v in N]
    D = sc.physics_D(h3d, N)
    a, b = sc.random_fields(N, 11, 2)
    bx = None if box == "whole" else sc.sub_box(n)
    kc, kg = sc.form_fields(h3d, N, form, "cpu"), sc.form_fields(h3d, N, form, gpu)
    if box == "sub":  # an inner side: the block's high z side is not a wall
        wall = [0, n[0] - 1, 0, n[1] - 1, 0, h3d.native().NO_WALL]
        kc["wall"], kg["wall"] = wall, wall
    pc, pg = _both(h3d, gpu, N, a)
    qc, qg = _both(h3d, gpu, N, 0 * a)
    dc = ops.steady_apply(pc, qc, D, box=bx, **kc)
    dg = ops.steady_apply(pg, qg, D, box=bx, **kg)
    assert np.array_equal(_bits(qc), _bits(qg))
    assert dg == ops.steady_apply(pg, qg, D, box=bx, **kg)
    ref, sabs = sc.fsum_bound(sc.owned_np(pc, bx), sc.owned_np(qc, bx))
    print(f"{N} {form} {box}: gpu {dg[0] + dg[1]!r} cpu {dc[0] + dc[1]!r} fsum {ref!r} bound {sc.EPS * sabs:.3e}")
    assert abs(dg[0] + dg[1] - ref) <= sc.EPS * sabs
    assert abs(dc[0] + dc[1] - ref) <= sc.EPS * sabs
    if box == "whole":
        sg, tg = sc.padded(h3d, N, b, gpu), sc.padded(h3d, N, 0 * b, gpu)
        ops.steady_apply(sg, tg, D, **kg)
        l, sl = sc.fsum_bound(sc.owned_np(pg), sc.owned_np(tg))
        r, sr = sc.fsum_bound(sc.owned_np(sg), sc.owned_np(qg))
        print(f"  p.Aq {l!r} q.Ap {r!r} diff {abs(l - r):.3e} bound {4 * sc.EPS * max(sl, sr):.3e}")
        assert abs(l - r) <= 4 * sc.EPS * max(sl, sr)


@pytest.mark.parametrize("form", ["uniform", "conductivity_walls"])
@pytest.mark.parametrize("N", sc.SHAPES)
def test_residual_form_with_source_bitwise(h3d, gpu, N, form):
    """r = b - A T with a source, the stored Dirichlet values and the ambient
    temperature is bitwise the CPU's; r . r holds the fsum bound."""
    from heat3d_amd import ops

    D = sc.physics_D(h3d, N)
    a, q = sc.random_fields(N, 17, 2)
    kc, kg = sc.form_fields(h3d, N, form, "cpu"), sc.form_fields(h3d, N, form, gpu)
    Tc, Tg = _both(h3d, gpu, N, a)
    Sc, Sg = _both(h3d, gpu, N, 1e-3 * q)
    rc, rg = _both(h3d, gpu, N, 0 * a)
    ops.steady_apply(Tc, rc, D, residual=True, source=Sc, ambient=0.25, **kc)
    dg = ops.steady_apply(Tg, rg, D, residual=True, source=Sg, ambient=0.25, **kg)
    assert np.array_equal(_bits(rc), _bits(rg))
    ref, sabs = sc.fsum_bound(sc.owned_np(rg), sc.owned_np(rg))
    assert abs(dg[0] + dg[1] - ref) <= sc.EPS * sabs


@pytest.mark.parametrize("box", ["whole", "sub"])
@pytest.mark.parametrize("N", sc.SHAPES)
def test_update_and_direction_bitwise(h3d, gpu, N, box):
    from heat3d_amd import ops

    n = [v - 2 for v in N]
    bx = None if box == "whole" else sc.sub_box(n)
    fields = sc.random_fields(N, 23, 4)
    c, g = zip(*[_both(h3d, gpu, N, f) for f in fields])
    alpha, beta = 0.3721, 0.8125
    dc = ops.steady_update(c[0], c[1], c[2], c[3], alpha, box=bx)
    dg = ops.steady_update(g[0], g[1], g[2], g[3], alpha, box=bx)
    for fc, fg in zip(c, g):
        assert np.array_equal(_bits(fc), _bits(fg))
    ref, sabs = sc.fsum_bound(sc.owned_np(g[2], bx), sc.owned_np(g[2], bx))
    assert abs(dg[0] + dg[1] - ref) <= sc.EPS * sabs and abs(dc[0] + dc[1] - ref) <= sc.EPS * sabs
    again = [sc.padded(h3d, N, f, gpu) for f in fields]
    assert dg == ops.steady_update(*again, alpha, box=bx)
    ops.steady_direction(c[1], c[2], beta, box=bx)
    ops.steady_direction(g[1], g[2], beta, box=bx)
    assert np.array_equal(_bits(c[1]), _bits(g[1]))


@pytest.mark.parametrize("name", ["reference33", "reference17x33x65", "sine_source", "layered", "convective_slab",
                                  "open_form"])
def test_solve_reaches_the_steady_state(h3d, gpu, name):
    s, r, T = sc.solve_and_check(h3d, name, "hip")
    assert s.backend == "hip"
    # the CPU oracle takes the same road
    _, rc, Tc = sc.solve_and_check(h3d, name, "cpu")
    assert abs(r["iterations"] - rc["iterations"]) <= 2
    _, r2, T2 = sc.solve_and_check(h3d, name, "hip")
    assert np.array_equal(T, T2) and r2["iterations"] == r["iterations"] and r2["residual"] == r["residual"]


@pytest.mark.parametrize("ranks", [2, 8])
def test_decompositions(h3d, gpu, ranks):
    decomp = (2, 1, 1) if ranks == 2 else (2, 2, 2)
    _, single, _ = sc.solve_and_check(h3d, "sine_source", "hip")
    _, r, T = sc.solve_and_check(h3d, "sine_source", "hip", virtual_ranks=ranks, decomp=decomp)
    assert abs(r["iterations"] - single["iterations"]) <= 2
    _, r2, T2 = sc.solve_and_check(h3d, "sine_source", "hip", virtual_ranks=ranks, decomp=decomp)
    assert np.array_equal(T, T2) and r2["iterations"] == r["iterations"]


def test_two_processes_one_gpu(h3d, gpu, tmp_path):
    mp.start_processes(steady_gpu_worker, args=(2, free_port(), str(tmp_path), "sine_source", (2, 1, 1)), nprocs=2,
                       join=True, start_method="spawn")
    got = [json.loads((tmp_path / f"steady{r}.json").read_text()) for r in range(2)]
    assert got[0] == got[1] and got[0]["converged"]


def test_state_after_a_solve(h3d, gpu, tmp_path):
    s, exact, _ = sc.make_solver(h3d, "convective_slab", "hip")
    r = s.solve_steady(sc.TOL, sc.CAP)
    assert r["converged"] and s.state()["iter"] == 0
    b = s.heat_balance()
    assert math.isfinite(b["imbalance"]) and b["nonfinite"] == 0
    G = s.gather()
    assert np.array_equal(G[0, 1:-1, 1:-1], G[1, 1:-1, 1:-1])
    s.save_checkpoint(str(tmp_path / "ck"))
    s3, _, _ = sc.make_solver(h3d, "convective_slab", "hip")
    s3.load_checkpoint(str(tmp_path / "ck"))
    assert np.array_equal(s3.gather(), G)
    out = s.run()
    assert not out["fault"]
    assert s.state()["last_residual"] <= sc.TOL * r["r0_norm"] + 4 * sc.EPS


def test_usage_errors(h3d, gpu):
    with pytest.raises(Exception, match="fp64"):
        h3d.HeatSolver((9, 9, 9), 10, 1e-5, backend="hip", device=0, dtype="fp32").solve_steady()
    with pytest.raises(Exception, match="singular"):
        h3d.HeatSolver((9, 9, 9), 10, 1e-5, backend="hip", device=0, insulated="all").solve_steady()
    with pytest.raises(Exception, match="tolerance"):
        h3d.HeatSolver((9, 9, 9), 10, 1e-5, backend="hip", device=0).solve_steady(0.0)
