"""Spatially varying conductivity (T_t = div(alpha c grad T) + q, 0 < c <= 1),
CPU backend: the arithmetic definition ftcs_update_var against the PyTorch
oracle, its conservative structure, the discrete steady state of a layered
body, the uniform limit, decomposition invariance, set / clear, the usage
errors, the CLI flag and checkpoints."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import run_cli

D = (0.06, 0.05, 0.04)
DT = {"fp64": torch.float64, "fp32": torch.float32}
EPS = {"fp64": float(np.finfo(np.float64).eps), "fp32": float(np.finfo(np.float32).eps)}
USAGE = "bin/HeatEquation3D NUM_CELLS_X NUM_CELLS_Y NUM_CELLS_Z ITER_MAX EPS"


def _rand_field(ops, n, dtype, seed, lo=0.0, hi=1.0, scale=1.0):
    """Random values in [lo, hi) times `scale` (in double, rounded once) on every ghost layer."""
    g = torch.Generator().manual_seed(seed)
    f = ops.PaddedField(n, dtype=dtype)
    v = f.ghosted()
    v.copy_((scale * (lo + (hi - lo) * torch.rand(v.shape, generator=g, dtype=torch.float64))).to(dtype))
    return f


def _rand_cond(ops, n, dtype, seed):
    """Ch = dtype(0.5 * c), c random in [0.05, 1]."""
    return _rand_field(ops, n, dtype, seed, 0.05, 1.0, 0.5)


def _rand_source(ops, n, dtype, seed):
    return _rand_field(ops, n, dtype, seed, -1e-3, 1e-3)


@pytest.mark.parametrize("with_source", [False, True])
@pytest.mark.parametrize("n", [(9, 13, 130), (5, 3, 64)])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_oracle_matches_cpu_stencil(h3d, dtype, n, with_source):
    ops = h3d.ops
    T = _rand_field(ops, n, dtype, 1)
    C = _rand_cond(ops, n, dtype, 2)
    S = _rand_source(ops, n, dtype, 3) if with_source else None
    want, res = ops.ftcs_reference(T.ghosted(), D, src=S.owned() if S else None, cond=C.ghosted())
    out = ops.PaddedField(n, dtype=dtype)
    st = ops.new_state("cpu")
    ops.ftcs_step(T, out, D, state=st, source=S, conductivity=C)
    assert torch.equal(out.owned(), want)
    assert ops.residual_from_state(st, 0) == res
    # the conductivity matters, and the default keeps the plain update
    plain, _ = ops.ftcs_reference(T.ghosted(), D, src=S.owned() if S else None)
    assert not torch.equal(plain, want)
    out2 = ops.PaddedField(n, dtype=dtype)
    ops.ftcs_step(T, out2, D, source=S)
    assert torch.equal(out2.owned(), plain)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_cpu_sweep_is_k_single_steps(h3d, dtype):
    """cpu::stencil_multi passes the conductivity on: K single steps stay the definition."""
    ops = h3d.ops
    n, K = (9, 13, 130), 3
    T = _rand_field(ops, n, dtype, 4)
    C = _rand_cond(ops, n, dtype, 5)
    a = T
    for s in range(K):
        b = ops.PaddedField(n, dtype=dtype)
        b.flat.copy_(a.flat)
        ops.ftcs_step(a, b, D, conductivity=C)
        a = b
    out = ops.PaddedField(n, dtype=dtype)
    out.flat.copy_(T.flat)
    ops.sweep(T, out, D, [0, n[0], 0, n[1], 0, n[2]], kernel=f"tl{K}", conductivity=C)
    assert torch.equal(out.owned(), a.owned())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_face_weights_and_fluxes_are_symmetric(h3d, dtype):
    """The structure behind exact conservation: the weight of a face has the
    same bits seen from either of its two cells (the add commutes), and the
    flux w (T_q - T_p) that leaves p is exactly minus the one that enters q."""
    from heat3d_amd.utils import fma

    g = torch.Generator().manual_seed(6)
    hp = (0.5 * (0.05 + 0.95 * torch.rand(4096, generator=g, dtype=torch.float64))).to(dtype)
    hq = (0.5 * (0.05 + 0.95 * torch.rand(4096, generator=g, dtype=torch.float64))).to(dtype)
    Tp = torch.rand(4096, generator=g, dtype=torch.float64).to(dtype)
    Tq = torch.rand(4096, generator=g, dtype=torch.float64).to(dtype)
    ity = torch.int64 if dtype == torch.float64 else torch.int32
    w_pq, w_qp = fma.face_weight(hp, hq), fma.face_weight(hq, hp)
    assert w_pq.dtype == dtype
    assert torch.equal(w_pq.view(ity), w_qp.view(ity))
    assert torch.equal((w_pq * (Tq - Tp)).view(ity), (-(w_qp * (Tp - Tq))).view(ity))
    # ... and the update uses exactly these weights: two neighbouring cells in
    # a line along z, everything else equal, exchange what the face carries
    one = lambda v: v[:1]
    up = fma.ftcs_update_var(one(Tp), one(Tp), one(Tp), one(Tp), one(Tp), one(Tp), one(Tq), one(hp), one(hp), one(hp),
                             one(hp), one(hp), one(hp), one(hq), (0.0, 0.0, 1.0))
    uq = fma.ftcs_update_var(one(Tq), one(Tq), one(Tq), one(Tq), one(Tq), one(Tp), one(Tq), one(hq), one(hq), one(hq),
                             one(hq), one(hq), one(hp), one(hq), (0.0, 0.0, 1.0))
    # with Dz = 1 and no other flux: T' = T + f exactly rounded once, f = +-w (Tq - Tp)
    f = one(w_pq) * (one(Tq) - one(Tp))
    assert torch.equal(up, one(Tp) + f) and torch.equal(uq, one(Tq) - f)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_layered_steady_state_is_a_fixed_point(h3d, dtype):
    """The exact steady state of the discrete scheme for a two-layer body stays
    put: max |T - p| <= 8 u * 20 after 20 steps, u the dtype's machine epsilon.

    Derived, not measured: p varies in y only, so fx and fz are exactly 0; the
    two y fluxes of a point cancel up to a few roundings of terms of size
    <= D w |dp| < 0.1, plus one rounding of the result (values <= 1); the
    update is a max-norm contraction, so the drift adds at most linearly.
    A non-conservative form (c at the vertex times the plain Laplacian) is not
    stationary here at all: at the material interface p has a kink, its plain
    second difference is O(|dp|) ~ 1e-1, and that form moves T by ~D c |dp|
    ~ 1e-3 per step, orders of magnitude beyond this bound."""
    n = (17, 17, 17)
    s = h3d.HeatSolver(n, 1000, 0.0, backend="cpu", dtype=dtype)
    c = s.model.layered_conductivity(0.25, 1.0)
    p = s.model.layered_steady(c)
    assert p[0, 0, 0] == 0.0 and p[0, -1, 0] == 1.0 and np.all(np.diff(p[0, :, 0]) > 0)
    s.set_conductivity(c)
    s.set_field(p)
    s.step(20)
    s.synchronize()
    err = np.abs(s.gather() - p).max()
    print("layered fixed point", dtype, "max |T - p| =", err, "bound", 8 * EPS[dtype] * 20)
    assert err <= 8 * EPS[dtype] * 20
    # the plain solver is not stationary on this field (the kink at the interface)
    t = h3d.HeatSolver(n, 1000, 0.0, backend="cpu", dtype=dtype)
    t.set_field(p)
    t.step(20)
    t.synchronize()
    assert np.abs(t.gather() - p).max() > 1e-3


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_uniform_conductivity_is_the_plain_solver_up_to_rounding(h3d, dtype):
    """c == 1: the same scheme in another association.  A per-step difference of
    a few ulps of max|T|, accumulated under the contraction for 50 steps."""
    n = (33, 29, 37)
    a = h3d.HeatSolver(n, 1000, 0.0, backend="cpu", dtype=dtype)
    a.step(50)
    a.synchronize()
    b = h3d.HeatSolver(n, 1000, 0.0, backend="cpu", dtype=dtype)
    b.set_conductivity(np.ones(n))
    b.step(50)
    b.synchronize()
    Ta, Tb = a.gather(), b.gather()
    diff = np.abs(Ta - Tb).max()
    print("uniform c == 1 against plain", dtype, "max |diff| =", diff)
    assert diff <= 50 * 8 * EPS[dtype] * np.abs(Ta).max()


def test_relaxation_towards_the_layered_steady_state(h3d):
    n = (17, 17, 17)
    errs = []
    for eps in (1e-4, 1e-6):
        s = h3d.HeatSolver(n, 200000, eps, backend="cpu")
        c = s.model.layered_conductivity(0.25, 1.0)
        p = s.model.layered_steady(c)
        T0 = p.copy()
        T0[1:-1, 1:-1, 1:-1] = 0.0
        s.set_conductivity(c)
        s.set_field(T0)
        r = s.run()
        assert r["converged"], r
        errs.append(np.abs(s.gather() - p).max())
    print("relaxation: max |T - p| at eps 1e-4, 1e-6:", errs)
    assert errs[1] < errs[0]


def test_decomposition_invariance(h3d):
    n = (21, 19, 23)
    rng = np.random.default_rng(7)
    c = rng.uniform(0.05, 1.0, n)
    q = rng.uniform(-50.0, 50.0, n)
    fields = []
    for vr, dec in ((1, None), (8, (2, 2, 2)), (8, (8, 1, 1))):
        s = h3d.HeatSolver(n, 1000, 0.0, backend="cpu", virtual_ranks=vr, decomp=dec)
        s.set_conductivity(c)
        s.set_source(q)
        s.step(50)
        s.synchronize()
        fields.append(s.gather())
    assert np.array_equal(fields[0], fields[1])
    assert np.array_equal(fields[0], fields[2])
    # ... and the conductivity is really in there
    s = h3d.HeatSolver(n, 1000, 0.0, backend="cpu")
    s.set_source(q)
    s.step(50)
    s.synchronize()
    assert not np.array_equal(fields[0], s.gather())


@pytest.mark.parametrize("temporal", [(), ("--temporal", "3")])
def test_set_and_clear(h3d, temporal):
    n = (17, 15, 19)
    c = np.random.default_rng(8).uniform(0.05, 1.0, n)
    fresh = h3d.HeatSolver(n, 1000, 0.0, backend="cpu", extra_args=list(temporal))
    fresh.step(50)
    fresh.synchronize()
    s = h3d.HeatSolver(n, 1000, 0.0, backend="cpu", extra_args=list(temporal))
    s.set_conductivity(c)
    assert s.native.has_conductivity
    s.step(10)
    s.synchronize()
    assert s.state()["iter"] == 10
    s.clear_conductivity()
    assert not s.native.has_conductivity
    s.initialize()
    s.step(50)
    s.synchronize()
    assert np.array_equal(s.gather(), fresh.gather())


@pytest.mark.parametrize("bad", [0.0, 1.5, float("nan")])
def test_bad_values_are_usage_errors(h3d, heat3d_bin, tmp_path, bad):
    n = (17, 17, 17)
    c = np.full(n, 0.5)
    c[2, 2, 2] = bad  # read by the first subdomain of 2x2x2 only (ghosts included)
    for vr, dec in ((1, None), (8, (2, 2, 2))):
        s = h3d.HeatSolver(n, 10, 0.0, backend="cpu", virtual_ranks=vr, decomp=dec)
        with pytest.raises(h3d.native().UsageError, match=r"conductivity.*\(0, 1\]"):
            s.set_conductivity(c)
        assert not s.native.has_conductivity
        s.step(2)  # the solver goes on without one
        s.synchronize()
    c.tofile(tmp_path / "c.raw")
    for extra in ((), ("--virtual-ranks", "8", "--decomp", "2x2x2")):
        r = run_cli([*n, 10, "1e-4", "--backend", "cpu", "--conductivity", "c.raw", "--output", "none", *extra],
                    tmp_path)
        assert r.returncode != 0
        assert USAGE in r.stdout
        assert "conductivity" in r.stderr and "(0, 1]" in r.stderr


def test_python_argument_checks(h3d):
    s = h3d.HeatSolver((9, 9, 9), 10, 0.0, backend="cpu")
    with pytest.raises(ValueError):
        s.set_conductivity(np.ones((9, 9, 8)))
    ops = h3d.ops
    T = ops.PaddedField((5, 5, 40))
    with pytest.raises(ValueError):
        ops.ftcs_step(T, ops.PaddedField((5, 5, 40)), D, conductivity=ops.PaddedField((5, 5, 41)))
    with pytest.raises(ValueError):
        s.model.layered_steady(np.random.default_rng(0).uniform(0.1, 1.0, (9, 9, 9)))


def test_cli_wrong_file_size_and_compat_are_usage_errors(heat3d_bin, tmp_path):
    np.ones(100).tofile(tmp_path / "short.raw")
    r = run_cli(["15", "13", "17", "10", "1e-4", "--backend", "cpu", "--conductivity", "short.raw"], tmp_path)
    assert r.returncode != 0
    assert USAGE in r.stdout
    assert "--conductivity" in r.stderr and "bytes" in r.stderr
    np.ones((15, 13, 17)).tofile(tmp_path / "c.raw")
    r = run_cli(["15", "13", "17", "10", "1e-4", "--backend", "cpu", "--compat", "--conductivity", "c.raw"], tmp_path)
    assert r.returncode != 0
    assert USAGE in r.stdout
    assert "--compat" in r.stderr and "--conductivity" in r.stderr


def test_cli_conductivity_and_initial(h3d, heat3d_bin, tmp_path):
    n = (15, 13, 17)
    rng = np.random.default_rng(11)
    c = rng.uniform(0.05, 1.0, n)
    s = h3d.HeatSolver(n, 100000, 1e-4, backend="cpu")
    T0 = s.model.initial_field() + 0.0
    T0[1:-1, 1:-1, 1:-1] = rng.uniform(0.0, 1.0, (n[0] - 2, n[1] - 2, n[2] - 2))
    s.set_conductivity(c)
    s.set_field(T0)
    r = s.run()
    assert r["converged"]
    s.write_tecplot(str(tmp_path / "py.dat"))
    c.tofile(tmp_path / "c.raw")
    T0.tofile(tmp_path / "t0.raw")
    x = run_cli([*n, 100000, "1e-4", "--backend", "cpu", "--conductivity", "c.raw", "--initial", "t0.raw",
                 "--output", "cli.dat", "--json-out", "run.json"], tmp_path)
    assert x.returncode == 0, x.stderr
    j = json.loads((tmp_path / "run.json").read_text())
    assert j["conv_iter"] == r["conv_iter"] and j["converged"]
    assert (tmp_path / "cli.dat").read_bytes() == (tmp_path / "py.dat").read_bytes()
    # virtual ranks read their own boxes: same result
    x2 = run_cli([*n, 100000, "1e-4", "--backend", "cpu", "--virtual-ranks", "4", "--decomp", "2x2x1",
                  "--conductivity", "c.raw", "--initial", "t0.raw", "--output", "none", "--json-out", "run2.json"],
                 tmp_path)
    assert x2.returncode == 0, x2.stderr
    assert json.loads((tmp_path / "run2.json").read_text())["conv_iter"] == r["conv_iter"]
    assert "--conductivity FILE" in h3d.native().usage()


def test_checkpoint_with_conductivity(h3d, tmp_path):
    n = (15, 13, 17)
    c = np.random.default_rng(3).uniform(0.05, 1.0, n)
    a = h3d.HeatSolver(n, 1000, 0.0, backend="cpu")
    a.set_conductivity(c)
    a.step(30)
    a.synchronize()
    ck = str(tmp_path / "ck")
    a.save_checkpoint(ck)
    assert json.loads(open(os.path.join(ck, "meta.json")).read())["has_conductivity"] is True
    a.step(30)
    a.synchronize()
    b = h3d.HeatSolver(n, 1000, 0.0, backend="cpu")
    b.set_conductivity(c)
    b.load_checkpoint(ck)
    b.step(30)
    b.synchronize()
    assert np.array_equal(a.gather(), b.gather())
    assert b.state()["iter"] == a.state()["iter"] == 60
    d = h3d.HeatSolver(n, 1000, 0.0, backend="cpu")
    d.initialize()
    with pytest.raises(RuntimeError, match="conductivity"):
        d.load_checkpoint(ck)
    # a checkpoint without one records that, and loads as before
    d.step(10)
    d.synchronize()
    ck2 = str(tmp_path / "ck2")
    d.save_checkpoint(ck2)
    assert json.loads(open(os.path.join(ck2, "meta.json")).read())["has_conductivity"] is False
    d.load_checkpoint(ck2)
