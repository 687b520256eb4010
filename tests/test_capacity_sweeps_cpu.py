"""K-step sweeps with a heat capacity and a conductivity (--capacity-sweeps),
CPU backend: the sweep schedule (whole sweeps of depth 3 and 2, partial sweeps,
single-step remainders, x slabs and a 2x2x2 block decomposition, rollback to the
convergence iteration) gives bit for bit the field, the residual history and the
iteration count of the single-step run, without walls and behind an insulated x-
and a convective y- wall; the flag without a conductivity does nothing; the flag
with --compat is a usage error; clear_capacity() returns to the earlier bits; the
tc kernel specs and the CLI flag."""
import numpy as np
import pytest
import torch

from conftest import run_cli

N = (17, 19, 33)
STEPS = 40  # 13 sweeps of 3 and a single step; 20 sweeps of 2
USAGE = "bin/HeatEquation3D NUM_CELLS_X NUM_CELLS_Y NUM_CELLS_Z ITER_MAX EPS"
WALLS = dict(insulated="x-", convective={"y-": 0.5}, ambient=0.25)
D = (0.06, 0.05, 0.04)


def _inputs():
    rng = np.random.default_rng(5)
    return (rng.uniform(0.0, 1.0, N), rng.uniform(0.05, 1.0, N), rng.uniform(1.0, 9.0, N),
            rng.uniform(-50.0, 50.0, N))


def _solver(h3d, flag, walls=False, vr=1, dec=None, temporal=3, eps=0.0, iters=100000, cond=True, **kw):
    s = h3d.HeatSolver(N, iters, eps, backend="cpu", virtual_ranks=vr, decomp=dec, capacity_sweeps=flag,
                       extra_args=["--temporal", str(temporal)], **(WALLS if walls else {}), **kw)
    T0, c, rc, q = _inputs()
    s.set_field(T0)
    if cond:
        s.set_conductivity(c)
    s.set_source(q)
    s.set_capacity(rc)
    return s


def _steps(s, steps=STEPS):
    s.step(steps)
    s.synchronize()
    return s.gather(), s.native.residual_history(), s.state()["iter"]


def history_upto(s, conv_iter):
    """{iteration: residual} of the kept history (the last 1024 checks, the last
    of them iteration state()["iter"] - 1) up to the convergence iteration: what
    follows it are the checks of iterations issued after convergence, no-ops
    whose number depends on the schedule's polling."""
    hist = s.native.residual_history()
    first = s.state()["iter"] - len(hist)
    return {first + i: r for i, r in enumerate(hist) if first + i <= conv_iter}


@pytest.fixture(scope="module")
def flag_off(h3d):
    """The single-step runs (flag off), with and without walls."""
    out = {}
    for walls in (False, True):
        s = _solver(h3d, False, walls)
        assert s.native.has_capacity and not s.native.sweeps_active
        out[walls] = _steps(s)
        assert "tc" not in s.kernel
    return out


@pytest.mark.parametrize("walls", [False, True], ids=["dirichlet", "walls"])
@pytest.mark.parametrize("vr,dec", [(1, None), (8, (2, 2, 2)), (2, (2, 1, 1))], ids=["one", "2x2x2", "2x1x1"])
@pytest.mark.parametrize("temporal", [3, 2])
def test_sweeps_equal_single_steps(h3d, flag_off, temporal, vr, dec, walls):
    s = _solver(h3d, True, walls, vr, dec, temporal)
    assert s.native.has_capacity and s.native.sweeps_active and s.kernel.startswith(f"tc{temporal}:"), s.kernel
    T, hist, it = _steps(s)
    wT, whist, wit = flag_off[walls]
    assert it == wit == STEPS
    assert hist == whist
    assert np.array_equal(T, wT)


@pytest.mark.parametrize("walls", [False, True], ids=["dirichlet", "walls"])
def test_convergence_iteration(h3d, walls):
    """run() to eps 1e-3: the same conv_iter and the same history up to it (what
    follows are the checks of iterations issued after convergence), the same
    field: the rollback inside a sweep."""
    res = []
    for flag in (False, True):
        s = _solver(h3d, flag, walls, eps=1e-3)
        r = s.run()
        assert r["converged"] and s.native.sweeps_active == flag
        res.append((r["conv_iter"], history_upto(s, r["conv_iter"]), s.gather()))
    assert res[0][0] == res[1][0] > 3
    both = sorted(res[0][1].keys() & res[1][1].keys())
    assert len(both) >= 64 and both[-1] == res[0][0]
    assert [res[0][1][t] for t in both] == [res[1][1][t] for t in both]
    assert np.array_equal(res[0][2], res[1][2])


def test_flag_without_a_conductivity_does_nothing(h3d, flag_off):
    s = _solver(h3d, True, cond=False)
    assert s.native.has_capacity and not s.native.sweeps_active and "tc" not in s.kernel
    T, hist, it = _steps(s)
    t = _solver(h3d, False, cond=False)
    wT, whist, wit = _steps(t)
    assert it == wit and hist == whist and np.array_equal(T, wT)
    # (and the conductivity is what made the other runs differ)
    assert not np.array_equal(T, flag_off[False][0])


def test_other_sweep_flags_mean_nothing_with_a_capacity(h3d, flag_off):
    """While a capacity is set capacity_sweeps alone decides."""
    s = _solver(h3d, False, True, conductivity_sweeps=True, wall_source_sweeps=True)
    assert not s.native.sweeps_active
    T, hist, it = _steps(s)
    assert hist == flag_off[True][1] and np.array_equal(T, flag_off[True][0])


def test_flag_with_compat_is_a_usage_error(h3d, heat3d_bin, tmp_path):
    assert "--capacity-sweeps" in h3d.native().usage()
    r = run_cli(["15", "13", "17", "10", "1e-4", "--backend", "cpu", "--compat", "--capacity-sweeps"], tmp_path)
    assert r.returncode != 0
    assert USAGE in r.stdout
    assert "--compat" in r.stderr and "--capacity-sweeps" in r.stderr
    with pytest.raises(RuntimeError, match="--capacity-sweeps"):
        h3d.HeatSolver((15, 13, 17), 10, 1e-4, backend="cpu", capacity_sweeps=True, extra_args=["--compat"])


def test_cli_flag(h3d, heat3d_bin, tmp_path):
    """--capacity / --conductivity from files: the same output file with and without the flag."""
    import json

    n = (15, 13, 17)
    rng = np.random.default_rng(3)
    rng.uniform(0.05, 1.0, n).tofile(tmp_path / "c.raw")
    rng.uniform(1.0, 9.0, n).tofile(tmp_path / "rc.raw")
    outs = []
    for extra in ((), ("--capacity-sweeps",)):
        x = run_cli([*map(str, n), "40", "0", "--backend", "cpu", "--temporal", "3", "--conductivity", "c.raw",
                     "--capacity", "rc.raw", "--output", f"o{len(extra)}.dat", "--json-out", "run.json", *extra],
                    tmp_path)
        assert x.returncode == 0, x.stderr
        j = json.loads((tmp_path / "run.json").read_text())
        assert j["capacity_sweeps"] == bool(extra) and j["has_capacity"]
        assert j["kernel"].startswith("tc3") == bool(extra), j["kernel"]
        outs.append((tmp_path / f"o{len(extra)}.dat").read_bytes())
    assert outs[0] == outs[1]


def test_clear_returns_to_the_earlier_bits(h3d):
    """clear_capacity() puts a flag-on run back on the tv sweeps
    (conductivity_sweeps) or the single steps it ran before, clear_conductivity()
    on the capacity's single steps; the fields are those of fresh runs."""
    T0, c, rc, q = _inputs()
    fresh = h3d.HeatSolver(N, 1000, 0.0, backend="cpu", conductivity_sweeps=True, extra_args=["--temporal", "3"])
    fresh.set_field(T0)
    fresh.set_conductivity(c)
    fresh.set_source(q)
    assert fresh.native.sweeps_active and fresh.kernel.startswith("tv3")
    want = _steps(fresh, 20)
    s = _solver(h3d, True, conductivity_sweeps=True)
    assert s.kernel.startswith("tc3")
    _steps(s, 7)
    s.clear_capacity()
    assert not s.native.has_capacity and s.native.sweeps_active and s.kernel.startswith("tv3"), s.kernel
    s.set_field(T0)
    got = _steps(s, 20)
    assert got[1] == want[1] and np.array_equal(got[0], want[0])
    # ... and back, then without the conductivity: the capacity's single steps
    s.set_capacity(rc)
    assert s.native.sweeps_active and s.kernel.startswith("tc3")
    s.clear_conductivity()
    assert s.native.has_capacity and not s.native.sweeps_active and "tc" not in s.kernel
    s.set_field(T0)
    got = _steps(s, 20)
    t = _solver(h3d, False, cond=False)
    want = _steps(t, 20)
    assert got[1] == want[1] and np.array_equal(got[0], want[0])


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_tc_spec_runs_the_definition(h3d, dtype, K):
    """ops.sweep with a tc spec on host fields: K single steps with cond and cap."""
    ops = h3d.ops
    n = (7, 6, 9)
    gen = torch.Generator().manual_seed(4)

    def rand(lo, hi):
        f = ops.PaddedField(n, dtype=dtype)
        f.ghosted().copy_((lo + (hi - lo) * torch.rand(f.ghosted().shape, generator=gen, dtype=torch.float64)).to(dtype))
        return f

    T, C, S, A = rand(0.0, 1.0), rand(0.025, 0.5), rand(-1e-3, 1e-3), rand(1.0, 9.0)
    A.ghosted().copy_((1.0 / A.ghosted().double()).to(dtype))
    got = ops.PaddedField(n, dtype=dtype)
    st = ops.new_state("cpu")
    ops.sweep(T, got, D, (0, n[0], 0, n[1], 0, n[2]), kernel=f"tc{K}", state=st, source=S, conductivity=C, cap=A)
    a, b = ops.PaddedField(n, dtype=dtype), ops.PaddedField(n, dtype=dtype)
    a.flat.copy_(T.flat)
    b.flat.copy_(T.flat)
    for s in range(K):
        st1 = ops.new_state("cpu")
        ops.ftcs_step(a, b, D, state=st1, source=S, conductivity=C, cap=A)
        assert ops.residual_from_state(st1) == ops.residual_from_state(st, s)
        a, b = b, a
    assert torch.equal(got.owned(), a.owned())


def test_form_queries(h3d):
    """tc2 is built in every form of both dtypes (the solver never falls back to
    single steps for want of a kernel); each built form runs on at least 8
    waves; the dispatch checks come before any device work."""
    ext = h3d.native()
    for dt in ("fp64", "fp32"):
        for wall in (0, 1, 2):
            for src in (False, True):
                deepest = ext.cap_sweep_max_depth(dt, src, wall)
                assert 2 <= deepest <= 3
                for K in (2, 3):
                    shape = ext.cap_sweep_shape(dt, f"tc{K}", src, wall)
                    assert (shape is not None) == ext.cap_sweep_supported(dt, f"tc{K}", src, wall) == (K <= deepest)
                    if shape:
                        R, WY = shape
                        assert WY >= 8 and R * WY > 2 * K
                assert ext.cap_sweep_shape(dt, "tc4", src, wall) is None
        assert not ext.cap_sweep_supported(dt, "tv3") and not ext.cond_sweep_supported(dt, "tc3")
    with pytest.raises(RuntimeError, match="wall is 0"):
        ext.cap_sweep_supported("fp64", "tc2", False, 3)
    ops = h3d.ops
    n = (8, 40, 70)
    T, C, A, out = ops.PaddedField(n), ops.PaddedField(n), ops.PaddedField(n), ops.PaddedField(n)
    C.flat.fill_(0.25)
    A.flat.fill_(0.5)
    args = ("fp64", T.data_ptr(), out.data_ptr(), list(n), [1, 1, 1], [0, n[0], 0, n[1], 0, n[2]], [0, -1, 0, -1, 0, -1],
            list(D), 0, 0)
    none = [ext.NO_WALL] * 6
    with pytest.raises(RuntimeError, match="tc kernels need a heat-capacity field.*tv2 / tv3"):
        ext.hip.stencil_sweep3(*args, "tc2", 0, 0, C.data_ptr(), none, [-1.0] * 6, 0.0, 0)
    with pytest.raises(RuntimeError, match="tc kernels need a conductivity field.*single steps"):
        ext.hip.stencil_sweep3(*args, "tc2", 0, 0, 0, none, [-1.0] * 6, 0.0, A.data_ptr())
    with pytest.raises(RuntimeError, match="no heat-capacity form.*tc2 / tc3"):
        ext.hip.stencil_sweep3(*args, "tv3", 0, 0, C.data_ptr(), none, [-1.0] * 6, 0.0, A.data_ptr())
    assert torch.count_nonzero(out.flat) == 0
