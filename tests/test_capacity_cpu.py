"""A spatially varying heat capacity, CPU side: rc T_t = div(alpha c grad T) + q
with the stored field s = dtype(1 / rc) and the step T' = fma(s, u, T) on the
increment u of the step (kernels.hpp cap_update).

1. rc == 2 against an existing operator: T + 0.5 * (-A T), bit for bit.
2. The decay of a Dirichlet eigenmode under a uniform capacity.
3. Conservation of the weighted heat in an insulated cube, and the per-step
   identity of the heat balance.
4. The steady state does not move: the convective slab, run() and solve_steady.
5. A layered transient against a NumPy/torch transcription of the definition.
   (2 to 5 live in tests/_capacity_checks.py, which the GPU tests run as well.)
6. Refusals: bad values, file size, --compat, sweeps with a capacity, restart."""
import json

import numpy as np
import pytest
import torch

import _capacity_checks as cc
from conftest import run_cli

TORCH = {"fp64": torch.float64, "fp32": torch.float32}
EPS = {"fp64": 2.0 ** -52, "fp32": 2.0 ** -23}


def _solver(h3d, N, dtype="fp64", iters=1000, eps=0.0, **kw):
    return h3d.HeatSolver(N, iters, eps, dtype=dtype, backend="cpu", **kw)


# ---- 1. a power-of-two capacity against steady_apply -------------------------------------

@pytest.mark.parametrize("layered", [False, True], ids=["uniform", "layered"])
def test_power_of_two_capacity_is_half_the_increment(h3d, layered):
    """s = 0.5 is exact and 0.5 * u is exact, so fma(0.5, u, T) and the plain
    T + 0.5 * u round once to the same value; u = -(A T) of ops.steady_apply,
    whose field is the same fused chain started from zero."""
    ops = h3d.ops
    N = (21, 19, 23)
    n = tuple(v - 2 for v in N)
    m = h3d.HeatEquation3D(N)
    rng = np.random.default_rng(11)
    T0 = rng.uniform(-1.0, 1.0, N)
    for a in range(3):
        T0[(slice(None),) * a + (0,)] = 0.0
        T0[(slice(None),) * a + (-1,)] = 0.0
    c = m.layered_conductivity(0.25, 1.0) if layered else None
    s = _solver(h3d, N, extra_args=["--temporal", "1"])
    s.set_field(T0)
    if layered:
        s.set_conductivity(c)
    s.set_capacity(np.full(N, 2.0))
    s.step(1)
    s.synchronize()
    got = s.gather()
    f, out = ops.PaddedField(n), ops.PaddedField(n)
    f.ghosted().copy_(torch.from_numpy(T0))
    ch = None
    if layered:
        ch = ops.PaddedField(n)
        ch.ghosted().copy_(torch.from_numpy(0.5 * c))
    ops.steady_apply(f, out, m.D, cond=ch)
    want = T0[1:-1, 1:-1, 1:-1] + 0.5 * (-out.owned().numpy())
    assert np.array_equal(got[1:-1, 1:-1, 1:-1], want)
    # the capacity is seen: the same step without it gives another field
    s.clear_capacity()
    s.set_field(T0)
    s.step(1)
    s.synchronize()
    assert not np.array_equal(s.gather()[1:-1, 1:-1, 1:-1], want)


# ---- 2. eigenmode decay -------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("rc", [4.0, 1.0])
def test_eigenmode_decay(h3d, dtype, rc):
    cc.eigenmode_decay(h3d, "cpu", dtype, rc)


# ---- 3. conservation ----------------------------------------------------------------------

def test_weighted_heat_is_conserved(h3d):
    cc.weighted_heat_is_conserved(h3d, "cpu")


def test_heat_balance_weights_with_the_capacity(h3d):
    """heat = hx hy hz sum T / s against math.fsum; the other quantities are
    those of the run without a capacity."""
    import math

    N = (9, 8, 12)
    for dtype in ("fp64", "fp32"):
        s = _solver(h3d, N, dtype)
        rng = np.random.default_rng(5)
        T0 = rng.uniform(-1.0, 1.0, N)
        rc = rng.uniform(1.0, 9.0, N)
        s.set_field(T0)
        plain = s.heat_balance()
        assert "capacity" not in plain
        s.set_capacity(rc)
        got = s.heat_balance()
        np_t = np.float64 if dtype == "fp64" else np.float32
        T = T0.astype(np_t).astype(np.float64)[1:-1, 1:-1, 1:-1]
        sv = (1.0 / rc).astype(np_t).astype(np.float64)[1:-1, 1:-1, 1:-1]
        m = s.model
        ref = m.h[0] * m.h[1] * m.h[2] * math.fsum((T / sv).ravel())
        assert abs(got["heat"] - ref) <= 4 * math.ulp(ref)
        for key in ("t_min", "t_max", "nonfinite", "source_power", "flow", "imbalance"):
            assert got[key] == plain[key], key


# ---- 4. the steady state does not move ----------------------------------------------------

def test_steady_state_does_not_depend_on_the_capacity(h3d):
    cc.steady_state_does_not_depend_on_the_capacity(h3d, "cpu")


def test_solve_steady_ignores_the_capacity(h3d):
    cc.solve_steady_ignores_the_capacity(h3d, "cpu")


# ---- 5. the definition, transcribed -------------------------------------------------------

def test_layered_transient_matches_the_definition(h3d):
    cc.layered_transient_matches_the_definition(h3d, "cpu")


def test_sweep_definition_is_k_single_steps(h3d):
    """cpu::stencil_multi with cap (the definition of a later sweep kernel) is K
    single steps: the sweep entry on CPU tensors against ftcs_step, with a
    conductivity, a source and insulated walls."""
    ops = h3d.ops
    n, D = (6, 7, 9), (0.06, 0.05, 0.04)
    for dtype in (torch.float64, torch.float32):
        gen = torch.Generator().manual_seed(2)

        def rand(lo, hi):
            f = ops.PaddedField(n, dtype=dtype)
            v = f.ghosted()
            v.copy_((lo + (hi - lo) * torch.rand(v.shape, generator=gen, dtype=torch.float64)).to(dtype))
            return f

        T, C, S = rand(-1, 1), rand(0.025, 0.5), rand(-1e-3, 1e-3)
        K = ops.PaddedField(n, dtype=dtype)
        K.ghosted().copy_((1.0 / (1.0 + 7.0 * torch.rand(K.ghosted().shape, generator=gen, dtype=torch.float64))).to(dtype))
        walls = ops.wall_coords(63, n)
        box = [0, n[0], 0, n[1], 0, n[2]]
        a, b = ops.PaddedField(n, dtype=dtype), ops.PaddedField(n, dtype=dtype)
        a.flat.copy_(T.flat)
        for _ in range(3):
            b.flat.copy_(a.flat)
            ops.ftcs_step(a, b, D, source=S, conductivity=C, walls=walls, cap=K)
            a, b = b, a
        out = ops.PaddedField(n, dtype=dtype)
        out.flat.copy_(T.flat)
        ops.sweep3(T, out, D, box, (0, -1, 0, -1, 0, -1), kernel="tv3", source=S, conductivity=C, walls=walls, cap=K)
        assert torch.equal(out.owned(), a.owned())
        plain = ops.PaddedField(n, dtype=dtype)
        ops.sweep3(T, plain, D, box, (0, -1, 0, -1, 0, -1), kernel="tv3", source=S, conductivity=C, walls=walls)
        assert not torch.equal(plain.owned(), a.owned())


def test_decomposition_invariance(h3d):
    """1 rank against 2x2x2 virtual ranks: fields and residual histories, with
    walls, a conductivity and a source; clear_capacity() returns the bits of a
    run that never had a capacity."""
    N = (17, 17, 17)
    rng = np.random.default_rng(6)
    T0, rc, q = rng.uniform(0.0, 1.0, N), rng.uniform(1.0, 9.0, N), rng.uniform(-50.0, 50.0, N)
    out = []
    for vr, dec in ((1, None), (8, (2, 2, 2))):
        s = _solver(h3d, N, insulated="x-,z+", convective={"y-": 0.5}, ambient=0.25, virtual_ranks=vr, decomp=dec,
                    extra_args=["--temporal", "3"])
        c = s.model.layered_conductivity(0.25, 1.0)
        s.set_field(T0)
        s.set_conductivity(c)
        s.set_source(q)
        s.set_capacity(rc)
        assert s.native.has_capacity and not s.native.sweeps_active
        s.step(14)
        s.synchronize()
        out.append((s.gather(), s.native.residual_history(), s.heat_balance()["heat"]))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    assert abs(out[0][2] - out[1][2]) <= 4 * np.spacing(abs(out[0][2]))
    fresh = _solver(h3d, N, extra_args=["--temporal", "3"])
    fresh.step(14)
    fresh.synchronize()
    assert fresh.native.sweeps_active
    s = _solver(h3d, N, extra_args=["--temporal", "3"])
    s.set_capacity(rc)
    s.step(3)
    s.synchronize()
    assert not s.native.sweeps_active
    s.clear_capacity()
    assert s.native.sweeps_active and not s.native.has_capacity
    s.initialize()
    s.step(14)
    s.synchronize()
    assert np.array_equal(s.gather(), fresh.gather())
    assert s.native.residual_history() == fresh.native.residual_history()


# ---- 6. refusals ----------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [0.5, float("nan"), float("inf")])
def test_bad_values_are_a_usage_error(h3d, bad):
    N = (7, 8, 9)
    s = _solver(h3d, N, virtual_ranks=2)
    rc = np.full(N, 2.0)
    rc[3, 4, 5] = bad
    rc[5, 1, 1] = bad
    with pytest.raises(RuntimeError, match=r"capacity.*first at index \(3, 4, 5\)"):
        s.set_capacity(rc)
    assert not s.native.has_capacity
    s.step(2)  # the run goes on without one
    s.synchronize()


def test_cli_flag(h3d, heat3d_bin, tmp_path):
    N = (9, 8, 7)
    rc = np.full(N, 3.0)
    rc.tofile(tmp_path / "rc.bin")
    np.full(N, 3.0)[:-1].tofile(tmp_path / "short.bin")
    low = rc.copy()
    low[2, 3, 4] = 0.5
    low.tofile(tmp_path / "low.bin")
    base = [str(v) for v in N] + ["50", "0", "--backend", "cpu", "--output", "none", "--quiet"]
    ok = run_cli(base + ["--capacity", "rc.bin", "--json-out", "r.json", "--heat-balance"], tmp_path)
    assert ok.returncode == 0, ok.stderr
    rep = json.loads((tmp_path / "r.json").read_text())
    assert rep["has_capacity"] is True and rep["heat_balance"]["capacity"] is True
    plain = run_cli(base + ["--json-out", "p.json"], tmp_path)
    assert plain.returncode == 0 and json.loads((tmp_path / "p.json").read_text())["has_capacity"] is False
    for args, msg in ((["--capacity", "short.bin"], "--capacity file"), (["--capacity", "low.bin"], "capacity"),
                      (["--capacity", "rc.bin", "--compat"], "--capacity is not part of --compat")):
        r = run_cli(base + args, tmp_path)
        assert r.returncode != 0 and msg in r.stderr, (args, r.stderr)
    assert "--capacity FILE" in run_cli(["--help"], tmp_path).stdout


@pytest.mark.parametrize("kernel", ["tl3", "tl3:2", "tl4:1:4:1:12:0:3:66:0:3", "tv3"])
def test_gfx950_sweep_entries_refuse_a_capacity(h3d, ext, kernel):
    """The lean, pair, edge-role and tv entries check their parameters on the
    host before anything is launched: with a capacity they raise (no GPU needed,
    nothing is dereferenced)."""
    ops = h3d.ops
    n = (8, 40, 70)
    f = [ops.PaddedField(n) for _ in range(4)]
    box = [0, n[0], 0, n[1], 0, n[2]]
    with pytest.raises(RuntimeError, match="no heat-capacity form"):
        ext.hip.stencil_sweep("fp64", f[0].data_ptr(), f[1].data_ptr(), list(n), 1, box, [0, -1], [0.06, 0.05, 0.04], 0, 0,
                              kernel, 0, 0, f[2].data_ptr() if kernel.startswith("tv") else 0, f[3].data_ptr())


@pytest.mark.parametrize("flags", [["--compat"], ["--scheme", "reference"]], ids=["compat", "scheme-reference"])
def test_compat_solver_refuses(h3d, flags):
    s = h3d.HeatSolver((7, 7, 7), 10, 0.0, backend="cpu", extra_args=flags)
    with pytest.raises(RuntimeError, match="not part of --compat / --scheme reference"):
        s.set_capacity(np.full((7, 7, 7), 2.0))
    assert not s.native.has_capacity


def test_checkpoint_needs_the_capacity_again(h3d, tmp_path):
    N = (9, 9, 9)
    rc = h3d.HeatEquation3D(N).layered_capacity(1.0, 4.0)
    a = _solver(h3d, N)
    a.set_capacity(rc)
    a.step(7)
    a.synchronize()
    a.save_checkpoint(str(tmp_path / "ck"))
    assert json.loads((tmp_path / "ck" / "meta.json").read_text())["has_capacity"] is True
    a.step(5)
    a.synchronize()
    b = _solver(h3d, N)
    b.initialize()
    with pytest.raises(RuntimeError, match="heat capacity"):
        b.load_checkpoint(str(tmp_path / "ck"))
    b.set_capacity(rc)
    b.load_checkpoint(str(tmp_path / "ck"))
    b.step(5)
    b.synchronize()
    assert np.array_equal(a.gather(), b.gather())
    # a checkpoint of a run without a capacity has the key and loads as before
    p = _solver(h3d, N)
    p.step(3)
    p.synchronize()
    p.save_checkpoint(str(tmp_path / "plain"))
    assert json.loads((tmp_path / "plain" / "meta.json").read_text())["has_capacity"] is False
    _solver(h3d, N).initialize().load_checkpoint(str(tmp_path / "plain"))
    # ... and one from before the key existed
    meta = json.loads((tmp_path / "plain" / "meta.json").read_text())
    del meta["has_capacity"]
    (tmp_path / "plain" / "meta.json").write_text(json.dumps(meta))
    _solver(h3d, N).initialize().load_checkpoint(str(tmp_path / "plain"))
