"""Volumetric heat source (T_t = alpha lap(T) + q) and user-supplied initial
fields, CPU backend: the arithmetic definition T' = ftcs_update(...) + S with
S = dtype(dt * q) against the PyTorch oracle, the K-step sweep definition, the
solver (zero source == no source, decomposition invariance, a manufactured
steady state, set_field), the CLI flags and checkpoints."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import run_cli

D = (0.06, 0.05, 0.04)


def _rand_field(ops, n, dtype, seed, gx=1, view="ghosted"):
    g = torch.Generator().manual_seed(seed)
    f = ops.PaddedField(n, dtype=dtype, gx=gx)
    v = getattr(f, view)()
    v.copy_(torch.rand(v.shape, generator=g, dtype=torch.float64).to(dtype))
    return f


def _rand_source(ops, n, dtype, seed, gx=1, view="ghosted"):
    """S of the size of a real dt * q (~1e-3 of the field), either sign."""
    g = torch.Generator().manual_seed(seed)
    f = ops.PaddedField(n, dtype=dtype, gx=gx)
    v = getattr(f, view)()
    v.copy_(((torch.rand(v.shape, generator=g, dtype=torch.float64) - 0.5) * 2e-3).to(dtype))
    return f


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_oracle_matches_cpu_stencil(h3d, dtype):
    ops = h3d.ops
    n = (9, 13, 130)
    T = _rand_field(ops, n, dtype, 1)
    S = _rand_source(ops, n, dtype, 2)
    want, res = ops.ftcs_reference(T.ghosted(), D, src=S.owned())
    out = ops.PaddedField(n, dtype=dtype)
    st = ops.new_state("cpu")
    ops.ftcs_step(T, out, D, state=st, source=S)
    assert torch.equal(out.owned(), want)
    assert ops.residual_from_state(st, 0) == res
    # the source matters, and the default keeps today's result
    plain, _ = ops.ftcs_reference(T.ghosted(), D)
    assert not torch.equal(plain, want)
    out2 = ops.PaddedField(n, dtype=dtype)
    ops.ftcs_step(T, out2, D)
    assert torch.equal(out2.owned(), plain)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_sweep_is_k_single_steps(h3d, K, dtype):
    ops = h3d.ops
    n = (9, 13, 130)
    T = _rand_field(ops, n, dtype, 3)
    S = _rand_source(ops, n, dtype, 4)
    a, b = T, None
    st1 = ops.new_state("cpu")
    for s in range(K):
        b = ops.PaddedField(n, dtype=dtype)
        b.flat.copy_(a.flat)
        ops.ftcs_step(a, b, D, state=st1, slot=s, source=S)
        a = b
    out = ops.PaddedField(n, dtype=dtype)
    out.flat.copy_(T.flat)
    stk = ops.new_state("cpu")
    ops.sweep(T, out, D, [0, n[0], 0, n[1], 0, n[2]], kernel=f"tl{K}", state=stk, source=S)
    assert torch.equal(out.owned(), a.owned())
    for s in range(K):
        assert ops.residual_from_state(stk, s) == ops.residual_from_state(st1, s), s


def test_zero_source_equals_no_source(h3d):
    n = (17, 17, 17)
    a = h3d.HeatSolver(n, 100000, 1e-4, backend="cpu")
    ra = a.run()
    Ta = a.gather()
    b = h3d.HeatSolver(n, 100000, 1e-4, backend="cpu")
    b.set_source(np.zeros(n))
    assert b.native.has_source
    rb = b.run()
    assert ra["converged"] and rb["converged"]
    assert rb["conv_iter"] == ra["conv_iter"] and rb["last_residual"] == ra["last_residual"]
    assert np.array_equal(b.gather(), Ta)
    b.clear_source()
    assert not b.native.has_source
    b.initialize()
    rc = b.run()
    assert rc["conv_iter"] == ra["conv_iter"] and rc["last_residual"] == ra["last_residual"]
    assert np.array_equal(b.gather(), Ta)


@pytest.mark.parametrize("temporal", [(), ("--temporal", "1"), ("--temporal", "3")])
def test_decomposition_invariance(h3d, temporal):
    n = (21, 19, 23)
    q = np.random.default_rng(7).uniform(-50.0, 50.0, n)
    fields = []
    for vr, dec in ((1, None), (3, (3, 1, 1)), (8, (2, 2, 2))):
        s = h3d.HeatSolver(n, 1000, 0.0, backend="cpu", virtual_ranks=vr, decomp=dec, extra_args=list(temporal))
        s.set_source(q)
        s.step(60)
        s.synchronize()
        fields.append(s.gather())
    assert np.array_equal(fields[0], fields[1])
    assert np.array_equal(fields[0], fields[2])
    # ... and the source is really in there
    s = h3d.HeatSolver(n, 1000, 0.0, backend="cpu", extra_args=list(temporal))
    s.step(60)
    s.synchronize()
    assert not np.array_equal(fields[0], s.gather())


def test_manufactured_steady_state(h3d):
    """The discrete steady state of sine_source(A) is exactly y + A sin sin sin.
    A NumPy model of this run reaches 9.2e-15 at 6000 steps (1.5e-8 at 3000);
    the bound is about 100x that floor."""
    n = (17, 15, 19)
    s = h3d.HeatSolver(n, 10000, 0.0, backend="cpu")
    m = s.model
    A = 0.25
    s.set_source(m.sine_source(A))
    s.step(6000)
    s.synchronize()
    x, y, z = (np.arange(k) * h for k, h in zip(n, m.h))
    exact = y[None, :, None] + A * np.sin(np.pi * x)[:, None, None] * np.sin(np.pi * y)[None, :, None] * \
        np.sin(np.pi * z)[None, None, :]
    err = np.abs(s.gather() - exact).max()
    print("manufactured steady state: max error", err)
    assert err <= 1e-12


def test_set_field_default_problem(h3d):
    n = (13, 13, 13)
    a = h3d.HeatSolver(n, 1000, 0.0, backend="cpu")
    a.step(50)
    a.synchronize()
    b = h3d.HeatSolver(n, 1000, 0.0, backend="cpu")
    b.set_field(b.model.initial_field())
    b.step(50)
    b.synchronize()
    assert np.array_equal(a.gather(), b.gather())


@pytest.mark.parametrize("vr,dec", [(1, None), (8, (2, 2, 2))])
def test_set_field_linear_in_x(h3d, vr, dec):
    n = (13, 13, 13)
    s = h3d.HeatSolver(n, 1000, 0.0, backend="cpu", virtual_ranks=vr, decomp=dec)
    T0 = np.broadcast_to((np.arange(n[0]) * s.model.h[0])[:, None, None], n).copy()
    s.set_field(T0)
    s.step(50)
    s.synchronize()
    T = s.gather()
    assert np.abs(T - T0).max() <= 1e-13
    for sl in ((0,), (-1,), (slice(None), 0), (slice(None), -1), (slice(None), slice(None), 0),
               (slice(None), slice(None), -1)):
        assert np.array_equal(T[sl], T0[sl])


def test_python_argument_checks(h3d):
    s = h3d.HeatSolver((9, 9, 9), 10, 0.0, backend="cpu")
    with pytest.raises(ValueError):
        s.set_source(np.zeros((9, 9, 8)))
    bad = np.zeros((9, 9, 9))
    bad[4, 4, 4] = np.nan
    with pytest.raises(ValueError):
        s.set_source(bad)
    with pytest.raises(ValueError):
        s.set_field(bad)
    with pytest.raises(ValueError):
        s.set_field(np.zeros((3, 3)))


def test_cli_source_and_initial(h3d, heat3d_bin, tmp_path):
    n = (15, 13, 17)
    rng = np.random.default_rng(11)
    q = rng.uniform(-30.0, 30.0, n)
    s = h3d.HeatSolver(n, 100000, 1e-4, backend="cpu")
    T0 = s.model.initial_field() + 0.0
    T0[1:-1, 1:-1, 1:-1] = rng.uniform(0.0, 1.0, (n[0] - 2, n[1] - 2, n[2] - 2))
    s.set_source(q)
    s.set_field(T0)
    r = s.run()
    assert r["converged"]
    s.write_tecplot(str(tmp_path / "py.dat"))
    q.tofile(tmp_path / "q.raw")
    T0.tofile(tmp_path / "t0.raw")
    c = run_cli([*n, 100000, "1e-4", "--backend", "cpu", "--source", "q.raw", "--initial", "t0.raw",
                 "--output", "cli.dat", "--json-out", "run.json"], tmp_path)
    assert c.returncode == 0, c.stderr
    j = json.loads((tmp_path / "run.json").read_text())
    assert j["conv_iter"] == r["conv_iter"] and j["converged"]
    assert (tmp_path / "cli.dat").read_bytes() == (tmp_path / "py.dat").read_bytes()
    # virtual ranks read their own boxes: same result
    c2 = run_cli([*n, 100000, "1e-4", "--backend", "cpu", "--virtual-ranks", "4", "--decomp", "2x2x1", "--source",
                  "q.raw", "--initial", "t0.raw", "--output", "none", "--json-out", "run2.json"], tmp_path)
    assert c2.returncode == 0, c2.stderr
    assert json.loads((tmp_path / "run2.json").read_text())["conv_iter"] == r["conv_iter"]
    # --help lists the flags
    assert "--source FILE" in h3d.native().usage() and "--initial FILE" in h3d.native().usage()


@pytest.mark.parametrize("flag", ["--source", "--initial"])
def test_cli_wrong_file_size_is_usage_error(heat3d_bin, tmp_path, flag):
    np.zeros(100).tofile(tmp_path / "short.raw")
    c = run_cli(["15", "13", "17", "10", "1e-4", "--backend", "cpu", flag, "short.raw"], tmp_path)
    assert c.returncode != 0
    assert "bin/HeatEquation3D NUM_CELLS_X NUM_CELLS_Y NUM_CELLS_Z ITER_MAX EPS" in c.stdout
    assert flag in c.stderr and "bytes" in c.stderr


def test_checkpoint_with_source(h3d, tmp_path):
    n = (15, 13, 17)
    q = np.random.default_rng(3).uniform(-40.0, 40.0, n)
    a = h3d.HeatSolver(n, 1000, 0.0, backend="cpu")
    a.set_source(q)
    a.step(30)
    a.synchronize()
    ck = str(tmp_path / "ck")
    a.save_checkpoint(ck)
    assert json.loads(open(os.path.join(ck, "meta.json")).read())["has_source"] is True
    a.step(30)
    a.synchronize()
    b = h3d.HeatSolver(n, 1000, 0.0, backend="cpu")
    b.set_source(q)
    b.load_checkpoint(ck)
    b.step(30)
    b.synchronize()
    assert np.array_equal(a.gather(), b.gather())
    assert b.state()["iter"] == a.state()["iter"] == 60
    c = h3d.HeatSolver(n, 1000, 0.0, backend="cpu")
    c.initialize()
    with pytest.raises(RuntimeError, match="heat source"):
        c.load_checkpoint(ck)
    # a checkpoint without a source records that, and loads as before
    d = h3d.HeatSolver(n, 1000, 0.0, backend="cpu")
    d.step(10)
    d.synchronize()
    ck2 = str(tmp_path / "ck2")
    d.save_checkpoint(ck2)
    assert json.loads(open(os.path.join(ck2, "meta.json")).read())["has_source"] is False
    c.load_checkpoint(ck2)
