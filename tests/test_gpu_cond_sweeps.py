"""The tv kernels (stencil_tbv.hip: K-step sweeps with a conductivity field) on
the GPU against the CPU K-single-steps definition bit for bit (field and all K
residual slots; with and without a heat source; tiles with masked tails, several
y tiles, fewer rows than a wave holds, boxes narrower than a tile's halo, a
single row; deep x / y / z halos with update ranges; the sub-box store mask; the
done flag; NaN faults), and the solver with --conductivity-sweeps: GPU == CPU
backend across decompositions and graph modes, and the convergence iteration."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D = (0.06, 0.05, 0.04)
DTYPES = [torch.float64, torch.float32]
KERNELS = ["tv2", "tv3"]  # every built depth


def _field(ops, n, dtype, seed, g=(1, 1, 1), lo=0.0, hi=1.0, scale=1.0):
    """Random values in [lo, hi) times `scale` on every ghost layer (host field)."""
    gen = torch.Generator().manual_seed(seed)
    f = ops.PaddedField(n, dtype=dtype, gx=g[0], gy=g[1], gz=g[2])
    v = f.deep3()
    v.copy_((scale * (lo + (hi - lo) * torch.rand(v.shape, generator=gen, dtype=torch.float64))).to(dtype))
    return f


def _cond(ops, n, dtype, seed, g=(1, 1, 1)):
    # Ch = dtype(0.5 * c), c in [0.05, 1], ghosts included
    return _field(ops, n, dtype, seed, g, 0.05, 1.0, 0.5)


def _source(ops, n, dtype, seed, g=(1, 1, 1)):
    return _field(ops, n, dtype, seed, g, -1e-3, 1e-3)


def _to(ops, f, gpu):
    d = ops.PaddedField(f.n, dtype=f.dtype, device=gpu, gx=f.gx, gy=f.gy, gz=f.gz)
    d.flat.copy_(f.flat)
    return d


def _both(ops, gpu, call, T, C, S, fill=-5.0):
    """Runs call(src, dst, state, source, conductivity) on host and on GPU
    fields; returns (want, got, residuals_cpu, residuals_gpu), fields as host
    flat tensors."""
    want = ops.PaddedField(T.n, dtype=T.dtype, gx=T.gx, gy=T.gy, gz=T.gz)
    want.flat.fill_(fill)
    st_c = ops.new_state("cpu")
    call(T, want, st_c, S, C)
    got = _to(ops, want, gpu)
    got.flat.fill_(fill)
    st_g = ops.new_state(gpu)
    call(_to(ops, T, gpu), got, st_g, _to(ops, S, gpu) if S else None, _to(ops, C, gpu))
    torch.cuda.synchronize()
    res = lambda st: [ops.residual_from_state(st, s) for s in range(4)]
    return want.flat, got.flat.cpu(), res(st_c), res(st_g)


@pytest.mark.parametrize("with_source", [False, True])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [(9, 13, 130), (6, 100, 70), (5, 3, 64), (3, 30, 7), (33, 1, 513)])
def test_sweep_matches_cpu(h3d, gpu, n, dtype, kernel, with_source):
    """(9, 13, 130): three z tiles with a masked tail; (6, 100, 70): at least two
    y tiles for any tile height up to 96 rows, and a z seam; (5, 3, 64): fewer
    rows than one wave holds; (3, 30, 7): narrower than a tile's halo;
    (33, 1, 513): a single row."""
    ops = h3d.ops
    T, C = _field(ops, n, dtype, 1), _cond(ops, n, dtype, 2)
    S = _source(ops, n, dtype, 3) if with_source else None
    box = [0, n[0], 0, n[1], 0, n[2]]

    def call(src, dst, st, q, c):
        ops.sweep(src, dst, D, box, kernel=kernel, state=st, source=q, conductivity=c)

    want, got, rc, rg = _both(ops, gpu, call, T, C, S)
    assert torch.equal(got, want), f"max diff {(got - want).abs().max().item()}"
    assert rc == rg, (rc, rg)
    K = int(kernel[2])
    assert all(r > 1e-300 for r in rg[:K])  # every stage recorded its residual


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n0,box_x,side", [(4, (0, 4), "both"), (9, (0, 9), "hi"), (12, (4, 8), "both")])
def test_sweep_deep_halo_matches_cpu(h3d, gpu, kernel, dtype, n0, box_x, side):
    """The slab path (the cases of test_gpu_temporal._deep_halo_case): K-plane
    ghost layers, the x update range widened into them."""
    ops = h3d.ops
    K = int(kernel[2])
    n = (n0, 37, 133)
    ux = (-(K - 1) if side in ("lo", "both") else 0, n0 + (K - 1 if side in ("hi", "both") else 0))
    box = (box_x[0], box_x[1], 0, n[1], 0, n[2])
    g = (K, 1, 1)
    T, C, S = _field(ops, n, dtype, 7, g), _cond(ops, n, dtype, 8, g), _source(ops, n, dtype, 9, g)

    def call(src, dst, st, q, c):
        ops.sweep(src, dst, D, box, ux, kernel=kernel, state=st, source=q, conductivity=c)

    want, got, rc, rg = _both(ops, gpu, call, T, C, S)
    assert torch.equal(got, want), f"max diff {(got - want).abs().max().item()}"
    assert rc == rg, (rc, rg)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep3_update_ranges_match_cpu(h3d, gpu, kernel, dtype):
    """Deep ghosts and update ranges on every axis (block decompositions)."""
    ops = h3d.ops
    K = int(kernel[2])
    n, box = (12, 50, 140), (0, 12, 0, 50, 0, 140)
    u = []
    for a in range(3):
        u += [-(K - 1), n[a] + K - 1]
    g = (K, K, K)
    T, C = _field(ops, n, dtype, 11, g), _cond(ops, n, dtype, 12, g)

    def call(src, dst, st, q, c):
        ops.sweep3(src, dst, D, box, u, kernel=kernel, state=st, source=q, conductivity=c)

    want, got, rc, rg = _both(ops, gpu, call, T, C, None)
    assert torch.equal(got, want), f"max diff {(got - want).abs().max().item()}"
    assert rc == rg, (rc, rg)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_sub_box_writes_nothing_outside(h3d, gpu, kernel, dtype):
    ops = h3d.ops
    n, box = (12, 14, 200), [3, 7, 2, 9, 5, 133]
    T, C = _field(ops, n, dtype, 4), _cond(ops, n, dtype, 5)

    def call(src, dst, st, q, c):
        ops.sweep(src, dst, D, box, kernel=kernel, state=st, conductivity=c)

    want, got, rc, rg = _both(ops, gpu, call, T, C, None, fill=-7.0)
    assert torch.equal(got, want) and rc == rg
    x0, x1, y0, y1, z0, z1 = box
    ref = ops.PaddedField(n, dtype=dtype)
    ref.flat.copy_(got)
    assert (ref.owned()[x0:x1, y0:y1, z0:z1] != -7.0).all()
    ref.owned()[x0:x1, y0:y1, z0:z1] = -7.0
    assert (ref.flat == -7.0).all()


@pytest.mark.parametrize("kernel", KERNELS)
def test_done_flag_writes_nothing(h3d, gpu, kernel):
    ops, ext = h3d.ops, h3d.native()
    n, dtype = (9, 13, 130), torch.float64
    T, C = _to(ops, _field(ops, n, dtype, 1), gpu), _to(ops, _cond(ops, n, dtype, 2), gpu)
    out = ops.PaddedField(n, dtype=dtype, device=gpu)
    out.flat.fill_(-7.0)
    st = ops.new_state(gpu)
    st.view(torch.int32)[ext.STATE_DONE_OFFSET // 4] = 1
    before = st.clone()
    ops.sweep(T, out, D, [0, n[0], 0, n[1], 0, n[2]], kernel=kernel, state=st, conductivity=C)
    torch.cuda.synchronize()
    assert (out.flat == -7.0).all() and torch.equal(st, before)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_uniform_lean_sweep_differs(h3d, gpu, kernel, dtype):
    """The conductivity is seen: the tl sweep of the same depth without it
    gives another field."""
    ops = h3d.ops
    n = (9, 13, 130)
    box = [0, n[0], 0, n[1], 0, n[2]]
    T, C = _to(ops, _field(ops, n, dtype, 1), gpu), _to(ops, _cond(ops, n, dtype, 2), gpu)
    a, b = ops.PaddedField(n, dtype=dtype, device=gpu), ops.PaddedField(n, dtype=dtype, device=gpu)
    ops.sweep(T, a, D, box, kernel=kernel, conductivity=C)
    ops.sweep(T, b, D, box, kernel="tl" + kernel[2])
    torch.cuda.synchronize()
    assert not torch.equal(a.owned().cpu(), b.owned().cpu())


N_SOLVER = (33, 29, 37)


def _cq():
    rng = np.random.default_rng(5)
    return rng.uniform(0.05, 1.0, N_SOLVER), rng.uniform(-50.0, 50.0, N_SOLVER)


def test_sweep_nan_faults(h3d, gpu):
    """A NaN in the field reaches the convergence check as a fault."""
    s = h3d.HeatSolver((41, 37, 45), 10 ** 6, 1e-5, backend="hip", conductivity_sweeps=True)
    s.set_conductivity(np.random.default_rng(2).uniform(0.05, 1.0, (41, 37, 45)))
    assert s.native.sweeps_active
    s.step(12)
    s.synchronize()
    s.native.inject(0, 20, 18, 22, float("nan"))
    r = s.run()
    assert r["fault"] and not r["converged"], r


@pytest.fixture(scope="module")
def cpu_fields(h3d):
    """CPU-backend single-step fields after 50 steps with the seeded conductivity and source, per dtype."""
    out = {}
    c, q = _cq()
    for dt in ("fp64", "fp32"):
        s = h3d.HeatSolver(N_SOLVER, 1000, 0.0, dtype=dt, backend="cpu")
        s.set_conductivity(c)
        s.set_source(q)
        s.step(50)
        s.synchronize()
        out[dt] = s.gather()
    return out


@pytest.mark.parametrize("dt", ["fp64", "fp32"])
@pytest.mark.parametrize("vr,dec,graph", [(1, None, True), (3, None, True), (8, (2, 2, 2), True), (1, None, False)])
def test_solver_gpu_equals_cpu(h3d, gpu, cpu_fields, dt, vr, dec, graph):
    s = h3d.HeatSolver(N_SOLVER, 1000, 0.0, dtype=dt, backend="hip", virtual_ranks=vr, decomp=dec, graph=graph,
                       conductivity_sweeps=True)
    c, q = _cq()
    s.set_conductivity(c)
    s.set_source(q)
    assert s.native.temporal_blocking and s.native.sweeps_active and s.kernel.startswith("tv3"), s.kernel
    s.step(50)
    s.synchronize()
    assert s.state()["iter"] == 50
    assert np.array_equal(s.gather(), cpu_fields[dt])
    if graph and vr == 1:
        assert s.native.graph_launches > 0


def test_solver_convergence_equals_cpu(h3d, gpu):
    n = (33, 33, 33)
    res = []
    for backend in ("cpu", "hip"):
        s = h3d.HeatSolver(n, 200000, 1e-4, backend=backend, conductivity_sweeps=backend == "hip")
        c = s.model.layered_conductivity(0.25, 1.0)
        T0 = s.model.layered_steady(c).copy()
        T0[1:-1, 1:-1, 1:-1] = 0.0
        s.set_conductivity(c)
        s.set_field(T0)
        assert s.native.sweeps_active == (backend == "hip")
        r = s.run()
        assert r["converged"]
        res.append((r["conv_iter"], r["last_residual"], s.gather()))
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    assert np.array_equal(res[0][2], res[1][2])
