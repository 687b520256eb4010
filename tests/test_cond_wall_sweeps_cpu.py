"""A conductivity behind insulated or convective walls, CPU side: the row
kernels that take walls and a conductivity together (the definition of the wall
forms of the tv sweeps) against a single step on refreshed wall planes, the
K-step sweeps (--conductivity-sweeps) against the single-step schedule, the exact
steady state of the layered slab cooled through one face, the heat balance of
the insulated cube, checkpoints, and the form queries."""
import math

import numpy as np
import pytest
import torch

D = (0.06, 0.05, 0.04)
TORCH = {"fp64": torch.float64, "fp32": torch.float32}
EPS = {"fp64": float(np.finfo(np.float64).eps), "fp32": float(np.finfo(np.float32).eps)}
# all six faces walled: insulated only, and insulated and convective mixed
INSULATED = dict(insulated="all", convective=None, ambient=0.0)
MIXED = dict(insulated="x-,y-,z+", convective={"x+": 0.25, "y+": 0.5, "z-": 0.75}, ambient=0.375)
FACE_SETS = {"insulated": INSULATED, "mixed": MIXED}


def _rand(ops, n, td, gen, lo=0.0, hi=1.0):
    f = ops.PaddedField(n, dtype=td)
    v = f.ghosted()
    v.copy_((lo + (hi - lo) * torch.rand(v.shape, generator=gen, dtype=torch.float64)).to(td))
    return f


def _refresh(ops, T, fs):
    """The wall planes of the ghosted block T as a single step sees them: a
    convective wall shows convective_ghost of its inward neighbour, an insulated
    one a copy (convective faces first, then the copies, axis order x, y, z, as
    ftcs_reference does; the planes are disjoint from their sources)."""
    from heat3d_amd.utils.fma import fma

    mask = ops.insulated_mask(fs["insulated"])
    beta = ops.convective_faces(fs["convective"])
    tinf = torch.tensor(float(fs["ambient"]), dtype=T.dtype)
    for a in range(3):
        for e in range(2):
            f = 2 * a + e
            src = T.select(a, T.shape[a] - 2 if e else 1).clone()
            dst = T.select(a, T.shape[a] - 1 if e else 0)
            if beta[f] >= 0:
                dst.copy_(fma(beta[f], tinf - src, src))
            elif (mask >> f) & 1:
                dst.copy_(src)


def _setup(ops, n, dtype, faces, with_source, seed):
    fs, td = FACE_SETS[faces], TORCH[dtype]
    mask = ops.insulated_mask(fs["insulated"]) | ops.convective_mask(fs["convective"])
    assert mask == 63
    walls = ops.wall_coords(mask, n)
    conv = ops.convective_faces(fs["convective"]) if fs["convective"] else None
    gen = torch.Generator().manual_seed(seed)
    T = _rand(ops, n, td, gen)
    C = _rand(ops, n, td, gen, 0.025, 0.5)  # Ch = 0.5 c, c in [0.05, 1]
    S = _rand(ops, n, td, gen, -5.0, 5.0) if with_source else None
    return fs, td, walls, conv, T, C, S


@pytest.mark.parametrize("with_source", [False, True])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("faces", sorted(FACE_SETS))
def test_step_is_a_step_on_refreshed_wall_planes(h3d, dtype, faces, with_source):
    """cpu::stencil with StencilParams::wall and cond together: bit for bit,
    field and residual, the conductivity step without `walls` on wall planes
    refreshed first, 3 steps on (7, 6, 9) with all six faces walled.  (Before the
    wall forms of the conductivity row existed this call raised.)"""
    ops = h3d.ops
    n = (7, 6, 9)
    fs, td, walls, conv, a, C, S = _setup(ops, n, dtype, faces, with_source, 5)
    b = ops.PaddedField(n, dtype=td)
    b.flat.copy_(a.flat)
    for _ in range(3):
        st = ops.new_state("cpu")
        ops.ftcs_step(a, b, D, state=st, source=S, conductivity=C, walls=walls, conv=conv, ambient=fs["ambient"])
        r = ops.PaddedField(n, dtype=td)
        r.flat.copy_(a.flat)
        _refresh(ops, r.ghosted(), fs)
        want = ops.PaddedField(n, dtype=td)
        sw = ops.new_state("cpu")
        ops.ftcs_step(r, want, D, state=sw, source=S, conductivity=C)
        assert torch.equal(b.owned(), want.owned())
        assert ops.residual_from_state(st) == ops.residual_from_state(sw)
        # ... and the torch oracle of the same arithmetic
        new, res = ops.ftcs_reference(a.ghosted().clone(), D, src=S.owned() if S is not None else None, cond=C.ghosted(),
                                      insulated=fs["insulated"], convective=fs["convective"], ambient=fs["ambient"])
        assert torch.equal(b.owned(), new) and ops.residual_from_state(st) == res
        # the walls matter
        plain = ops.PaddedField(n, dtype=td)
        ops.ftcs_step(a, plain, D, source=S, conductivity=C)
        assert not torch.equal(plain.owned(), b.owned())
        a, b = b, a


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("with_source", [False, True])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("faces", sorted(FACE_SETS))
def test_sweep_is_k_such_steps(h3d, dtype, faces, with_source, K):
    """cpu::stencil_multi with walls and a conductivity: K single steps with both."""
    ops = h3d.ops
    n = (7, 6, 9)
    fs, td, walls, conv, src, C, S = _setup(ops, n, dtype, faces, with_source, 8)
    got = ops.PaddedField(n, dtype=td)
    st = ops.new_state("cpu")
    ops.sweep3(src, got, D, (0, n[0], 0, n[1], 0, n[2]), (0, -1, 0, -1, 0, -1), kernel=f"tv{K}", state=st, source=S,
               conductivity=C, walls=walls, conv=conv, ambient=fs["ambient"])
    a, b = ops.PaddedField(n, dtype=td), ops.PaddedField(n, dtype=td)
    a.flat.copy_(src.flat)
    b.flat.copy_(src.flat)
    for s in range(K):
        st1 = ops.new_state("cpu")
        ops.ftcs_step(a, b, D, state=st1, source=S, conductivity=C, walls=walls, conv=conv, ambient=fs["ambient"])
        assert ops.residual_from_state(st1) == ops.residual_from_state(st, s)
        a, b = b, a
    assert torch.equal(got.owned(), a.owned())


def _solver(h3d, N, fs, flag, vr=1, dec=None, temporal=3, dtype="fp64", iters=1000, eps=0.0, extra=()):
    return h3d.HeatSolver(N, iters, eps, dtype=dtype, backend="cpu", virtual_ranks=vr, decomp=dec,
                          conductivity_sweeps=flag, extra_args=["--temporal", str(temporal), *extra], **fs)


def _inputs(N, seed=2):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, N), rng.uniform(0.05, 1.0, N), rng.uniform(-5.0, 5.0, N)


def _run(s, N, with_source, steps, seed=2):
    T0, c, q = _inputs(N, seed)
    s.set_conductivity(c)
    if with_source:
        s.set_source(q)
    s.set_field(T0)
    s.step(steps)
    s.synchronize()
    return s.gather(), s.native.residual_history(), s.state()["conv_iter"]


GRIDS = {(13, 12, 11): 14, (17, 17, 17): 11}
SOLVER_FACES = {"insulated": dict(insulated="x-,y+,z-", convective=None, ambient=0.0),
                "mixed": dict(insulated="x-,z+", convective={"y+": 0.5, "z-": 0.75}, ambient=0.375)}


@pytest.fixture(scope="module")
def flag_off(h3d):
    """The single-step runs (flag off), per grid, face set and source."""
    out = {}
    for N, steps in GRIDS.items():
        for name, fs in SOLVER_FACES.items():
            for with_source in (False, True):
                s = _solver(h3d, N, fs, False)
                out[N, name, with_source] = _run(s, N, with_source, steps)
                assert not s.native.sweeps_active
    return out


@pytest.mark.parametrize("with_source", [False, True])
@pytest.mark.parametrize("faces", sorted(SOLVER_FACES))
@pytest.mark.parametrize("vr,dec", [(1, None), (2, None), (4, (1, 2, 2))])
@pytest.mark.parametrize("temporal", [2, 3])
@pytest.mark.parametrize("N", sorted(GRIDS))
def test_sweeps_equal_single_steps(h3d, flag_off, N, temporal, vr, dec, faces, with_source):
    """--conductivity-sweeps behind walls: sweeps of depth 2 and 3 on 1, 2 and
    1x2x2 virtual ranks, bitwise the flag-off run: field, residual history and
    conv_iter.  The step counts (14, 11) end in a partial sweep or a single step."""
    s = _solver(h3d, N, SOLVER_FACES[faces], True, vr, dec, temporal)
    got = _run(s, N, with_source, GRIDS[N])
    assert s.native.sweeps_active and s.kernel.startswith(f"tv{temporal}:"), s.kernel
    assert s.state()["iter"] == GRIDS[N]
    want = flag_off[N, faces, with_source]
    assert got[1] == want[1] and got[2] == want[2]
    assert np.array_equal(got[0], want[0])


def test_convergence_iteration(h3d):
    """A run to convergence: the same conv_iter, last residual and field with
    and without the flag (the rollback inside a sweep)."""
    res = []
    for flag in (False, True):
        s = _solver(h3d, (13, 12, 11), SOLVER_FACES["mixed"], flag, iters=20000, eps=1e-3)
        T0, c, _ = _inputs((13, 12, 11))
        s.set_conductivity(c)
        s.set_field(T0)
        r = s.run()
        assert r["converged"] and s.native.sweeps_active == flag
        res.append((r["conv_iter"], r["last_residual"], s.gather()))
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    assert np.array_equal(res[0][2], res[1][2])


def test_clear_and_set_conductivity_switch_the_kernels(h3d):
    """clear_conductivity() returns the run to the lean wall forms,
    set_conductivity() to the tv sweeps; the fields are those of fresh runs."""
    N = (13, 12, 11)
    T0, c, _ = _inputs(N)
    s = _solver(h3d, N, SOLVER_FACES["mixed"], True)
    T7, _, _ = _run(s, N, False, 7)
    assert s.native.sweeps_active and s.kernel.startswith("tv3")
    s.clear_conductivity()
    assert s.native.sweeps_active and s.kernel.startswith("tl3"), s.kernel
    s.step(6)
    s.synchronize()
    t = _solver(h3d, N, SOLVER_FACES["mixed"], False)  # (no conductivity: the lean wall forms either way)
    t.set_field(T7)
    t.step(6)
    t.synchronize()
    assert t.native.sweeps_active and np.array_equal(s.gather(), t.gather())
    T13 = s.gather()
    s.set_conductivity(c)
    assert s.native.sweeps_active and s.kernel.startswith("tv3"), s.kernel
    s.step(5)
    s.synchronize()
    u = _solver(h3d, N, SOLVER_FACES["mixed"], False)
    u.set_conductivity(c)
    u.set_field(T13)
    assert not u.native.sweeps_active
    u.step(5)
    u.synchronize()
    assert np.array_equal(s.gather(), u.gather())


SLAB = dict(insulated="x-,x+,z-,z+", convective={"y-": 0.5}, ambient=0.25)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_layered_slab_steady_state_is_a_fixed_point(h3d, dtype):
    """layered_convective_slab_steady is a fixed point of the sweeps on
    (5, 33, 5): max |T - p| <= 8 u * 20 after 20 steps, u the dtype's machine
    epsilon, the tolerance of test_conductivity_cpu for layered_steady (the wall
    needs no more: the flag-off path moves the field by 0 in fp64 and by
    2.8e-8 in fp32 here, measured on the CPU, the flag-on path by the same).
    Without the conductivity, or with an insulated y- face, the field moves by
    orders of magnitude more."""
    N = (5, 33, 5)
    tol = 8 * EPS[dtype] * 20
    moved = {}
    for flag in (False, True):
        s = _solver(h3d, N, SLAB, flag, dtype=dtype)
        c = s.model.layered_conductivity(0.25, 1.0)
        p = s.model.layered_convective_slab_steady(c, 0.5, 0.25)
        s.set_conductivity(c)
        s.set_field(p)
        assert s.native.sweeps_active == flag
        s.step(20)
        s.synchronize()
        moved[flag] = np.abs(s.gather() - p).max()
    print(f"layered slab {dtype}: moved {moved}, tolerance {tol:.3e}")
    assert moved[False] <= tol and moved[True] <= tol
    # the defining relations (float64): a constant flux through every y face
    v, cy = p[2, :, 2], c[2, :, 2]
    w = 0.5 * (cy[:-1] + cy[1:])
    F = w * np.diff(v)
    assert v[-1] == 1.0 and v[0] == v[1] + 0.5 * (0.25 - v[1])
    assert np.abs(F[1:] - F[1]).max() < 1e-14 and abs(0.5 * w[0] * (v[1] - 0.25) - F[1]) < 1e-14
    assert np.all(np.diff(v[1:]) > 0) and v[1] > 0.25
    # not a fixed point of the uniform material, nor with the y- face insulated
    t = _solver(h3d, N, SLAB, True, dtype=dtype)
    t.set_field(p)
    t.step(20)
    t.synchronize()
    assert np.abs(t.gather() - p)[1:-1, 1:-1, 1:-1].max() > 1e2 * tol
    t = _solver(h3d, N, dict(insulated="x-,x+,y-,z-,z+"), True, dtype=dtype)
    t.set_conductivity(c)
    t.set_field(p)
    t.step(20)
    t.synchronize()
    assert np.abs(t.gather() - p)[1:-1, 1:-1, 1:-1].max() > 1e2 * tol


def test_relaxation_towards_the_layered_slab_steady_state(h3d):
    """From a zero interior the sweeps converge to the steady state: closer at
    the smaller eps, and the same run as without the flag."""
    N = (5, 33, 5)
    errs = []
    for eps in (1e-4, 1e-6):
        out = []
        for flag in (False, True):
            s = _solver(h3d, N, SLAB, flag, iters=400000, eps=eps)
            c = s.model.layered_conductivity(0.25, 1.0)
            p = s.model.layered_convective_slab_steady(c, 0.5, 0.25)
            T0 = p.copy()
            T0[1:-1, 1:-1, 1:-1] = 0.0
            s.set_conductivity(c)
            s.set_field(T0)
            r = s.run()
            assert r["converged"], r
            out.append((r["conv_iter"], s.gather()))
        assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])
        errs.append(np.abs(out[1][1] - p).max())
    print("relaxation: max |T - p| at eps 1e-4, 1e-6:", errs)
    assert errs[1] < errs[0] and errs[1] < 1e-2


def test_heat_balance(h3d):
    """All six faces insulated, a random conductivity, no source: the
    conservative form telescopes (both cells of a face add the same weight and
    opposite differences; behind a wall the flux is w (c - c) = +0), so the
    interior sum moves by rounding only.  One update rounds 15 times, per axis two
    differences, one product and one fused multiply-add, then the three outer
    fused multiply-adds, each result of magnitude at most 2 for a field in
    [0, 1] and weights <= 1, so each error is at most 2^-53: the drift after n
    steps is at most 15 n M_points 2^-53 (test_walls_cpu bounds the uniform
    update's 9 roundings by 10).  With one face left Dirichlet the sum moves by
    orders of magnitude more (the bound discriminates)."""
    N, n = (18, 14, 22), 30
    rng = np.random.default_rng(9)
    T0 = rng.uniform(0.0, 1.0, N)
    c = rng.uniform(0.05, 1.0, N)
    points = (N[0] - 2) * (N[1] - 2) * (N[2] - 2)
    bound = 15 * n * points * 2.0 ** -53
    drift = {}
    for faces in ("all", "x-,x+,y-,z-,z+"):
        s = _solver(h3d, N, dict(insulated=faces), True)
        s.set_conductivity(c)
        s.set_field(T0)
        assert s.native.sweeps_active
        s.step(n)
        s.synchronize()
        drift[faces] = abs(math.fsum(s.gather()[1:-1, 1:-1, 1:-1].ravel()) - math.fsum(T0[1:-1, 1:-1, 1:-1].ravel()))
    print(f"heat drift {drift}, bound {bound:.3e}")
    assert drift["all"] <= bound
    assert drift["x-,x+,y-,z-,z+"] > 1e3 * bound


def test_checkpoint_restart(h3d, tmp_path):
    """A restart mid-way (after 8 of 20 steps, inside the sweep schedule) gives
    the uninterrupted run, bitwise."""
    N = (13, 12, 11)
    T0, c, q = _inputs(N)
    s = _solver(h3d, N, SOLVER_FACES["mixed"], True)
    want, _, _ = _run(s, N, True, 20)
    a = _solver(h3d, N, SOLVER_FACES["mixed"], True)
    _run(a, N, True, 8)
    a.save_checkpoint(str(tmp_path / "ck"))
    b = _solver(h3d, N, SOLVER_FACES["mixed"], True)
    b.set_conductivity(c)
    b.set_source(q)
    b.load_checkpoint(str(tmp_path / "ck"))
    assert b.native.sweeps_active and b.state()["iter"] == 8
    b.step(12)
    b.synchronize()
    assert np.array_equal(b.gather(), want)


def test_form_queries(h3d):
    """Every wall form of tv2 and tv3 is built in both dtypes; the query names
    the tile that runs it; today's call signatures keep working."""
    ext = h3d.native()
    plain = {("fp64", 2): (2, 16), ("fp64", 3): (2, 12), ("fp32", 2): (5, 16), ("fp32", 3): (4, 12)}
    for dt in ("fp64", "fp32"):
        for K in (2, 3):
            assert ext.cond_sweep_supported(dt, f"tv{K}") and ext.cond_sweep_supported(dt, f"tv{K}", True)
            assert ext.cond_sweep_shape(dt, f"tv{K}") == plain[dt, K]
            for wall in (1, 2):
                for src in (False, True):
                    assert ext.cond_sweep_supported(dt, f"tv{K}", src, wall)
                    R, WY = ext.cond_sweep_shape(dt, f"tv{K}", src, wall)
                    # a shape of at least 8 waves whose tile is deeper than its halo rows
                    assert WY >= 8 and R * WY > 2 * K
                    if not src:
                        assert (R, WY) == plain[dt, K]
                assert ext.cond_sweep_max_depth(dt, src, wall) == 3
        assert ext.cond_sweep_shape(dt, "tv4", False, 1) is None and not ext.cond_sweep_supported(dt, "tv4", False, 2)
    assert ext.cond_sweep_shape("fp64", "tl3") is None
    with pytest.raises(RuntimeError, match="wall is 0"):
        ext.cond_sweep_supported("fp64", "tv2", False, 3)
    # the dispatch checks come before any device work: host fields do
    ops = h3d.ops
    n = (8, 40, 70)
    T, C, out = ops.PaddedField(n), ops.PaddedField(n), ops.PaddedField(n)
    C.flat.fill_(0.25)
    args = ("fp64", T.data_ptr(), out.data_ptr(), list(n), [1, 1, 1], [0, n[0], 0, n[1], 0, n[2]], [0, -1, 0, -1, 0, -1],
            list(D), 0, 0)
    walls = ops.wall_coords(63, n)
    with pytest.raises(RuntimeError, match="tv kernels need a conductivity field"):
        ext.hip.stencil_sweep3(*args, "tv2", 0, 0, 0, walls)
    assert torch.count_nonzero(out.flat) == 0
