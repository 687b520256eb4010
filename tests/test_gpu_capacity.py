"""A spatially varying heat capacity on the GPU: the single-step kernels of
stencil_cap.hip ({uniform, conductivity} x {source, none} x {fp64, fp32}) against
the CPU definition bit for bit (field, residual, nothing written outside the
box) at the smallest shapes that reach each kernel path, the power-of-two
capacity against steady_apply, the solver across decompositions and backends,
clear_capacity(), the value domain, and the heat balance."""
import numpy as np
import pytest
import torch

import _capacity_checks as cc
import _value_fields as vf

pytestmark = pytest.mark.gpu

D = (0.06, 0.05, 0.04)
SENTINEL = -7.0
TORCH = {"fp64": torch.float64, "fp32": torch.float32}
FORMS = [pytest.param(c, s, dt, id=f"{'cond' if c else 'uniform'}{'-src' if s else ''}-{dt}")
         for c in (False, True) for s in (False, True) for dt in ("fp64", "fp32")]

# box lo = (1, 1, 1): an odd lo[2], so the tile's first column starts below the
# box; y extent 19 is no multiple of the 16 rows of a tile, z extent 70 (fp32:
# 133) no multiple of the vector width, and more than one tile along z in fp32
PATHS = {
    # id: (kernel, z extent or None for the ragged default, y extent, ghost depth)
    "tile-ragged": ("tile", None, 19, 1),
    "two-x-segments": ("tile:0:0:0:0:16", None, 19, 1),
    "nontemporal": ("tile:0:0:0:0:16:1", None, 19, 1),
    "naive-thin": ("tile", 31, 19, 1),
    "naive-one-row": ("tile", None, 1, 1),
    "naive-by-name": ("naive", None, 19, 1),
    "sub-box-ghost-3": ("tile", None, 19, 3),
}


def _rand(ops, n, dtype, seed, lo, hi, g=1):
    gen = torch.Generator().manual_seed(seed)
    f = ops.PaddedField(n, dtype=dtype, gx=g, gy=g, gz=g)
    v = f.deep3()
    v.copy_((lo + (hi - lo) * torch.rand(v.shape, generator=gen, dtype=torch.float64)).to(dtype))
    return f


def _to(ops, f, dev):
    if f is None:
        return None
    d = ops.PaddedField(f.n, dtype=f.dtype, device=dev, gx=f.gx, gy=f.gy, gz=f.gz)
    d.flat.copy_(f.flat)
    return d


def _fields(ops, n, dtype, cond, src, g=1, seed=1):
    T = _rand(ops, n, dtype, seed, -1.0, 1.0, g)
    C = _rand(ops, n, dtype, seed + 1, 0.025, 0.5, g) if cond else None
    S = _rand(ops, n, dtype, seed + 2, -1e-3, 1e-3, g) if src else None
    K = _rand(ops, n, dtype, seed + 3, 1.0, 9.0, g)
    K.deep3().copy_((1.0 / K.deep3().double()).to(dtype))  # s = dtype(1 / rc)
    return T, C, S, K


def _step(ops, dev, T, C, S, K, box, kernel):
    """One step on `dev` into a sentinel-filled field; returns (flat buffer, residual)."""
    out = ops.PaddedField(T.n, dtype=T.dtype, device=dev, gx=T.gx, gy=T.gy, gz=T.gz)
    out.flat.fill_(SENTINEL)
    st = ops.new_state(dev)
    ops.ftcs_step(_to(ops, T, dev), out, D, box=box, kernel=kernel, state=st, source=_to(ops, S, dev),
                  conductivity=_to(ops, C, dev), cap=_to(ops, K, dev))
    if dev != "cpu":
        torch.cuda.synchronize()
    return out.flat.cpu(), ops.residual_from_state(st, 0)


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("cond,src,dt", FORMS)
def test_kernel_paths_match_the_definition(h3d, gpu, path, cond, src, dt):
    ops = h3d.ops
    kernel, ez, ey, g = PATHS[path]
    ez = ez or (133 if dt == "fp32" else 70)
    box = [1, 38, 1, 1 + ey, 1, 1 + ez]
    n = (39, ey + 2, ez + 2)
    T, C, S, K = _fields(ops, n, TORCH[dt], cond, src, g)
    want, rw = _step(ops, "cpu", T, C, S, K, box, "auto")
    got, rg = _step(ops, gpu, T, C, S, K, box, kernel)
    assert vf.same_bits(got, want)
    assert rg == rw and rw > 0.0
    # something was written, and only inside the box
    assert (want != SENTINEL).sum().item() == 37 * ey * ez
    # the capacity is seen: the same launch without it gives another field
    if path == "tile-ragged":
        out = ops.PaddedField(n, dtype=TORCH[dt], device=gpu)
        out.flat.fill_(SENTINEL)
        ops.ftcs_step(_to(ops, T, gpu), out, D, box=box, kernel=kernel, source=_to(ops, S, gpu),
                      conductivity=_to(ops, C, gpu))
        torch.cuda.synchronize()
        assert not torch.equal(out.flat.cpu(), want)


@pytest.mark.parametrize("layered", [False, True], ids=["uniform", "layered"])
def test_power_of_two_capacity_is_half_the_increment(h3d, gpu, layered):
    """rc == 2: one step equals T + 0.5 * (-steady_apply(T)) bit for bit (0.5 u is
    exact, so the fused and the plain form round once to the same value)."""
    ops = h3d.ops
    N = (21, 19, 23)
    n = tuple(v - 2 for v in N)
    m = h3d.HeatEquation3D(N)
    rng = np.random.default_rng(11)
    T0 = rng.uniform(-1.0, 1.0, N)
    for a in range(3):
        T0[(slice(None),) * a + (0,)] = 0.0
        T0[(slice(None),) * a + (-1,)] = 0.0
    f = ops.PaddedField(n)
    f.ghosted().copy_(torch.from_numpy(T0))
    ch = None
    if layered:
        ch = ops.PaddedField(n)
        ch.ghosted().copy_(torch.from_numpy(0.5 * m.layered_conductivity(0.25, 1.0)))
    half = ops.PaddedField(n)
    half.flat.fill_(0.5)
    out, au = ops.PaddedField(n, device=gpu), ops.PaddedField(n, device=gpu)
    ops.ftcs_step(_to(ops, f, gpu), out, m.D, conductivity=_to(ops, ch, gpu), cap=_to(ops, half, gpu))
    ops.steady_apply(_to(ops, f, gpu), au, m.D, cond=_to(ops, ch, gpu))
    torch.cuda.synchronize()
    want = f.owned() + 0.5 * (-au.owned().cpu())
    assert torch.equal(out.owned().cpu(), want)


# the implementation-independent checks of tests/test_capacity_cpu.py on the gfx950 backend

@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("rc", [4.0, 1.0])
def test_eigenmode_decay(h3d, gpu, dtype, rc):
    cc.eigenmode_decay(h3d, "hip", dtype, rc)


def test_weighted_heat_is_conserved(h3d, gpu):
    cc.weighted_heat_is_conserved(h3d, "hip")


def test_steady_state_does_not_depend_on_the_capacity(h3d, gpu):
    cc.steady_state_does_not_depend_on_the_capacity(h3d, "hip")


def test_solve_steady_ignores_the_capacity(h3d, gpu):
    cc.solve_steady_ignores_the_capacity(h3d, "hip")


def test_layered_transient_matches_the_definition(h3d, gpu):
    cc.layered_transient_matches_the_definition(h3d, "hip")


@pytest.mark.parametrize("kind", ["nan", "+inf", "subnormal"])
@pytest.mark.parametrize("cond,src,dt", FORMS)
def test_value_domain(h3d, gpu, kind, cond, src, dt):
    """One NaN, one Inf, a subnormal field: the CPU's bits, at the masked box of
    tests/test_gpu_value_domain.py."""
    ops = h3d.ops
    n = (9, 50, 130)
    dtype = TORCH[dt]
    _, C, S, K = _fields(ops, n, dtype, cond, src)
    if kind == "subnormal":
        T = vf.field(ops, "subnormal", n, dtype, 9)
        S = vf.source(ops, "subnormal", n, dtype, 10) if src else None
    else:
        T = vf.spike(ops, kind, (4, 17, 64), n, dtype, 9)
    box = [0, n[0], 0, n[1], 0, n[2]]
    want, rw = _step(ops, "cpu", T, C, S, K, box, "auto")
    got, rg = _step(ops, gpu, T, C, S, K, box, "tile")
    assert vf.same_bits(got, want)
    assert (rg == rw) or (rg != rg and rw != rw)
    if kind != "subnormal":
        assert rg != rg  # NaN - NaN and Inf - Inf: the residual says so


N_SOLVER = (33, 33, 33)
WALLS = dict(insulated="x-,z+", convective={"y-": 0.5}, ambient=0.25)


def _inputs():
    rng = np.random.default_rng(5)
    return (rng.uniform(0.0, 1.0, N_SOLVER), rng.uniform(1.0, 9.0, N_SOLVER), rng.uniform(0.05, 1.0, N_SOLVER),
            rng.uniform(-50.0, 50.0, N_SOLVER))


def _run(h3d, backend, dt, walls, vr=1, dec=None, eps=0.0, steps=40, full=True):
    """full: with a conductivity and a source; else the uniform material with the capacity alone."""
    s = h3d.HeatSolver(N_SOLVER, 100000, eps, dtype=dt, backend=backend, virtual_ranks=vr, decomp=dec,
                       **(WALLS if walls else {}))
    T0, rc, c, q = _inputs()
    s.set_field(T0)
    if full:
        s.set_conductivity(c)
        s.set_source(q)
    s.set_capacity(rc)
    assert s.native.has_capacity and not s.native.sweeps_active
    if eps > 0:
        r = s.run()
        return r["converged"], r["conv_iter"], s.native.residual_history(), s.gather()
    s.step(steps)
    s.synchronize()
    return s.state()["iter"], s.native.residual_history(), s.gather()


@pytest.fixture(scope="module")
def cpu_runs(h3d):
    return {(dt, w, f): _run(h3d, "cpu", dt, w, full=f) for dt in ("fp64", "fp32") for w in (False, True)
            for f in (False, True)}


@pytest.mark.parametrize("full", [False, True], ids=["uniform", "cond-src"])
@pytest.mark.parametrize("walls", [False, True], ids=["dirichlet", "walls"])
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
@pytest.mark.parametrize("vr,dec", [(1, None), (8, (2, 2, 2))])
def test_solver_gpu_equals_cpu(h3d, gpu, cpu_runs, dt, walls, vr, dec, full):
    it, hist, field = _run(h3d, "hip", dt, walls, vr, dec, full=full)
    want = cpu_runs[(dt, walls, full)]
    assert it == want[0] == 40
    assert hist == want[1]
    assert np.array_equal(field, want[2])


@pytest.mark.parametrize("walls", [False, True], ids=["dirichlet", "walls"])
def test_solver_convergence_equals_cpu(h3d, gpu, walls):
    a = _run(h3d, "cpu", "fp64", walls, eps=1e-3)
    b = _run(h3d, "hip", "fp64", walls, eps=1e-3)
    c = _run(h3d, "hip", "fp64", walls, 8, (2, 2, 2), eps=1e-3)
    assert a[0] and a[1] > 10
    assert a[:2] == b[:2] == c[:2]
    # the residuals of iterations 0 .. conv_iter (what follows them in the history are the checks of
    # iterations issued after convergence, no-ops whose number depends on the backend's polling)
    k = a[1] + 1
    print(f"history lengths {len(a[2])} {len(b[2])} {len(c[2])}, conv_iter {a[1]}")
    assert len(a[2]) >= k and a[2][:k] == b[2][:k] == c[2][:k]
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[3], c[3])


def test_clear_returns_to_the_sweeps(h3d, gpu):
    fresh = h3d.HeatSolver(N_SOLVER, 1000, 0.0, backend="hip")
    fresh.step(50)
    fresh.synchronize()
    assert fresh.native.sweeps_active
    s = h3d.HeatSolver(N_SOLVER, 1000, 0.0, backend="hip")
    s.set_capacity(_inputs()[1])
    s.step(10)
    s.synchronize()
    assert not s.native.sweeps_active and "tl" not in s.kernel
    s.clear_capacity()
    assert s.native.sweeps_active and "tl" in s.kernel and not s.native.has_capacity
    s.initialize()
    s.step(50)
    s.synchronize()
    assert np.array_equal(s.gather(), fresh.gather())
    assert s.native.residual_history() == fresh.native.residual_history()


def test_a_nan_is_a_fault_not_convergence(h3d, gpu):
    out = []
    for backend in ("cpu", "hip"):
        s = h3d.HeatSolver(N_SOLVER, 500, 1e-12, backend=backend)
        s.set_capacity(_inputs()[1])
        s.native.inject(0, 16, 16, 16, float("nan"))
        r = s.run()
        st = s.state()
        assert not r["converged"] and st["fault"] == 1
        out.append((st["conv_iter"], st["iter"]))
    assert out[0] == out[1]


def test_sweep_with_a_capacity_is_an_error(h3d, gpu):
    ops = h3d.ops
    n = (8, 40, 70)
    T, C, _, K = _fields(ops, n, torch.float64, True, False)
    out = ops.PaddedField(n, device=gpu)
    box = [0, n[0], 0, n[1], 0, n[2]]
    for kernel, c in (("tl3", None), ("tl3:2", None), ("tv3", C)):
        with pytest.raises(RuntimeError, match="no heat-capacity form"):
            ops.sweep(_to(ops, T, gpu), out, D, box, kernel=kernel, conductivity=_to(ops, c, gpu), cap=_to(ops, K, gpu))


@pytest.mark.parametrize("dt", ["fp64", "fp32"])
def test_heat_balance_matches_the_definition(h3d, gpu, dt):
    """heat = hx hy hz sum T / s: the kernel against the CPU definition to the
    last rounding of two double-double sums of different shapes; the per-step
    identity on the GPU backend."""
    import math

    ops = h3d.ops
    n = (9, 12, 133)
    T, C, S, K = _fields(ops, n, TORCH[dt], True, True)
    m = h3d.HeatEquation3D(tuple(v + 2 for v in n))
    want = ops.heat_balance(T, m, source=S, cond=C, cap=K)
    got = ops.heat_balance(_to(ops, T, gpu), m, source=_to(ops, S, gpu), cond=_to(ops, C, gpu), cap=_to(ops, K, gpu))
    assert got["capacity"] is True
    assert abs(got["heat"] - want["heat"]) <= math.ulp(want["heat"])
    plain = ops.heat_balance(_to(ops, T, gpu), m, source=_to(ops, S, gpu), cond=_to(ops, C, gpu))
    assert plain["heat"] != got["heat"]
    for key in ("t_min", "t_max", "nonfinite", "source_power", "flow", "imbalance"):
        assert got[key] == plain[key], key
    s = h3d.HeatSolver(N_SOLVER, 100, 0.0, dtype=dt, backend="hip", **WALLS)
    T0, rc, c, q = _inputs()
    s.set_field(T0)
    s.set_conductivity(c)
    s.set_source(q)
    s.set_capacity(rc)
    U = (N_SOLVER[0] - 2) ** 3
    vol = s.model.h[0] * s.model.h[1] * s.model.h[2]
    eps = 2.0 ** -52 if dt == "fp64" else 2.0 ** -23
    b = s.heat_balance()
    for k in range(3):
        s.step(1)
        nb = s.heat_balance()
        tmax = max(abs(b["t_min"]), abs(b["t_max"]), abs(nb["t_min"]), abs(nb["t_max"]))
        bound = 8 * eps * tmax * U * vol
        defect = abs(nb["heat"] - b["heat"] - s.model.dt * b["imbalance"])
        print(f"{dt} step {k}: defect {defect:.3e} bound {bound:.3e}")
        assert defect <= bound
        b = nb
