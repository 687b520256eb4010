"""K-step sweeps with a conductivity field (--conductivity-sweeps), CPU backend:
the sweep schedule (whole sweeps, partial sweeps, single-step remainders, x slabs
and block decompositions, rollback to the convergence iteration) gives bit for
bit the fields of the single-step run; the flag alone changes nothing; the CLI
flag; the tv kernel specs."""
import numpy as np
import pytest
import torch

from conftest import run_cli

N = (33, 29, 37)
USAGE = "bin/HeatEquation3D NUM_CELLS_X NUM_CELLS_Y NUM_CELLS_Z ITER_MAX EPS"


def _cq():
    # the seeded c and q of test_gpu_conductivity._cq
    rng = np.random.default_rng(5)
    return rng.uniform(0.05, 1.0, N), rng.uniform(-50.0, 50.0, N)


def _solver(h3d, sweeps, vr=1, dec=None, temporal=3, dtype="fp64"):
    s = h3d.HeatSolver(N, 1000, 0.0, dtype=dtype, backend="cpu", virtual_ranks=vr, decomp=dec,
                       conductivity_sweeps=sweeps, extra_args=["--temporal", str(temporal)])
    c, q = _cq()
    s.set_conductivity(c)
    s.set_source(q)
    return s


@pytest.fixture(scope="module")
def single_step_fields(h3d):
    """Flag-off fields after 1, 2, 7 and 50 steps (one subdomain; the result does
    not depend on the decomposition: tests/test_conductivity_cpu.py)."""
    out = {}
    for m in (1, 2, 7, 50):
        s = _solver(h3d, False)
        assert not s.native.sweeps_active
        s.step(m)
        s.synchronize()
        out[m] = s.gather()
    return out


@pytest.mark.parametrize("temporal", [2, 3])
@pytest.mark.parametrize("vr,dec", [(1, None), (3, None), (8, (2, 2, 2))])
def test_sweeps_equal_single_steps(h3d, single_step_fields, vr, dec, temporal):
    for m in (1, 2, 7, 50):
        s = _solver(h3d, True, vr, dec, temporal)
        assert s.native.sweeps_active and s.kernel.startswith(f"tv{temporal}:"), s.kernel
        s.step(m)
        s.synchronize()
        assert s.state()["iter"] == m
        assert np.array_equal(s.gather(), single_step_fields[m]), (vr, dec, temporal, m)


def test_sweeps_equal_single_steps_fp32(h3d):
    a, b = _solver(h3d, True, dtype="fp32"), _solver(h3d, False, dtype="fp32")
    for s in (a, b):
        s.step(20)
        s.synchronize()
    assert a.native.sweeps_active and not b.native.sweeps_active
    assert np.array_equal(a.gather(), b.gather())


def test_layered_convergence(h3d):
    """Rollback to the exact convergence iteration inside a sweep."""
    res = []
    for sweeps in (False, True):
        s = h3d.HeatSolver((33, 33, 33), 200000, 1e-4, backend="cpu", conductivity_sweeps=sweeps,
                           extra_args=["--temporal", "3"])
        c = s.model.layered_conductivity(0.25, 1.0)
        T0 = s.model.layered_steady(c).copy()
        T0[1:-1, 1:-1, 1:-1] = 0.0
        s.set_conductivity(c)
        s.set_field(T0)
        assert s.native.sweeps_active == sweeps
        r = s.run()
        assert r["converged"]
        res.append((r["conv_iter"], r["last_residual"], s.gather()))
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    assert np.array_equal(res[0][2], res[1][2])


def test_clear_returns_to_lean_sweeps(h3d):
    fresh = h3d.HeatSolver(N, 1000, 0.0, backend="cpu", extra_args=["--temporal", "3"])
    fresh.step(20)
    fresh.synchronize()
    s = h3d.HeatSolver(N, 1000, 0.0, backend="cpu", conductivity_sweeps=True, extra_args=["--temporal", "3"])
    s.set_conductivity(_cq()[0])
    s.step(10)
    s.synchronize()
    assert s.native.sweeps_active and s.kernel.startswith("tv3")
    s.clear_conductivity()
    assert s.state()["iter"] == 0
    assert s.native.sweeps_active and s.kernel.startswith("tl3"), s.kernel
    s.initialize()
    s.step(20)
    s.synchronize()
    assert np.array_equal(s.gather(), fresh.gather())


def test_flag_without_conductivity_changes_nothing(h3d):
    a = h3d.HeatSolver(N, 1000, 0.0, backend="cpu", conductivity_sweeps=True, extra_args=["--temporal", "3"])
    b = h3d.HeatSolver(N, 1000, 0.0, backend="cpu", extra_args=["--temporal", "3"])
    assert "--conductivity-sweeps" in a.args and "--conductivity-sweeps" not in b.args
    for s in (a, b):
        s.step(20)
        s.synchronize()
    assert a.kernel == b.kernel and a.kernel.startswith("tl3")
    assert a.native.sweeps_active and b.native.sweeps_active
    assert np.array_equal(a.gather(), b.gather())
    # no temporal blocking: the flag has nothing to switch
    c = h3d.HeatSolver(N, 1000, 0.0, backend="cpu", conductivity_sweeps=True, extra_args=["--temporal", "1"])
    c.set_conductivity(_cq()[0])
    assert not c.native.sweeps_active


def test_cli_flag(h3d, heat3d_bin, tmp_path):
    assert "--conductivity-sweeps" in h3d.native().usage()
    np.ones((15, 13, 17)).tofile(tmp_path / "c.raw")
    r = run_cli(["15", "13", "17", "10", "1e-4", "--backend", "cpu", "--compat", "--conductivity-sweeps"], tmp_path)
    assert r.returncode != 0
    assert USAGE in r.stdout
    assert "--compat" in r.stderr and "--conductivity-sweeps" in r.stderr
    import json

    outs = []
    for extra in ((), ("--conductivity-sweeps",)):
        x = run_cli(["15", "13", "17", "40", "0", "--backend", "cpu", "--temporal", "3", "--conductivity", "c.raw",
                     "--output", f"o{len(extra)}.dat", "--json-out", "run.json", *extra], tmp_path)
        assert x.returncode == 0, x.stderr
        j = json.loads((tmp_path / "run.json").read_text())
        assert j["conductivity_sweeps"] == bool(extra)
        assert j["kernel"].startswith("tv3") == bool(extra), j["kernel"]
        outs.append((tmp_path / f"o{len(extra)}.dat").read_bytes())
    assert outs[0] == outs[1]


def test_kernel_specs(h3d):
    ext, ops = h3d.native(), h3d.ops
    for spec in ("tv2", "tv3"):
        full = ext.kernel_spec_resolved(spec, "fp64")
        assert full.startswith(spec + ":")
        assert ext.kernel_spec_resolved(full, "fp64") == full
        for dt in ("fp64", "fp32"):
            assert ext.cond_sweep_supported(dt, spec) and ext.cond_sweep_supported(dt, spec, True)
    assert not ext.cond_sweep_supported("fp64", "tl3")
    with pytest.raises(RuntimeError, match="unknown kernel"):
        ext.kernel_spec_resolved("tv7", "fp64")
    # the dispatch checks come before any device work: host fields do
    n = (8, 40, 70)
    T, C, out = ops.PaddedField(n), ops.PaddedField(n), ops.PaddedField(n)
    C.flat.fill_(0.25)
    args = ("fp64", T.data_ptr(), out.data_ptr(), list(n), 1, [0, n[0], 0, n[1], 0, n[2]], [0, -1],
            [0.06, 0.05, 0.04], 0, 0)
    with pytest.raises(RuntimeError, match="no conductivity form"):
        ext.hip.stencil_sweep(*args, "tl3", 0, 0, C.data_ptr())
    with pytest.raises(RuntimeError, match="tv kernels need a conductivity field"):
        ext.hip.stencil_sweep(*args, "tv2", 0, 0, 0)
    assert torch.count_nonzero(out.flat) == 0
