"""Spatially varying conductivity on the GPU: the single-step kernels of
stencil_var.hip (tile, naive; with and without a heat source) against the
PyTorch oracle bit for bit (field and residual), the sub-box store mask, the
refused K-step sweep, and the solver with a conductivity field: GPU == CPU
backend across decompositions and graph modes, the convergence iteration, and
the return to K-step sweeps after clear_conductivity()."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D = (0.06, 0.05, 0.04)
DTYPES = [torch.float64, torch.float32]


def _rand(ops, n, dtype, seed, lo=0.0, hi=1.0, scale=1.0):
    """Random values in [lo, hi) times `scale` on the whole ghost shell (host field)."""
    gen = torch.Generator().manual_seed(seed)
    f = ops.PaddedField(n, dtype=dtype)
    v = f.ghosted()
    v.copy_((scale * (lo + (hi - lo) * torch.rand(v.shape, generator=gen, dtype=torch.float64))).to(dtype))
    return f


def _cond(ops, n, dtype, seed):
    # Ch = dtype(0.5 * c), c in [0.05, 1], ghosts included
    return _rand(ops, n, dtype, seed, 0.05, 1.0, 0.5)


def _source(ops, n, dtype, seed):
    return _rand(ops, n, dtype, seed, -1e-3, 1e-3)


def _to(ops, f, gpu):
    d = ops.PaddedField(f.n, dtype=f.dtype, device=gpu)
    d.flat.copy_(f.flat)
    return d


@pytest.mark.parametrize("with_source", [False, True])
@pytest.mark.parametrize("kernel", ["tile", "naive"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [(9, 13, 130), (5, 3, 64)])
def test_single_step_matches_oracle(h3d, gpu, kernel, dtype, n, with_source):
    """(9, 13, 130): several waves of a tile in y, two tiles in z with a masked
    tail, partial rows; (5, 3, 64): fewer rows than a wave's R."""
    ops = h3d.ops
    T, C = _rand(ops, n, dtype, 1), _cond(ops, n, dtype, 2)
    S = _source(ops, n, dtype, 3) if with_source else None
    want, res = ops.ftcs_reference(T.ghosted(), D, src=S.owned() if S else None, cond=C.ghosted())
    out = ops.PaddedField(n, dtype=dtype, device=gpu)
    st = ops.new_state(gpu)
    ops.ftcs_step(_to(ops, T, gpu), out, D, kernel=kernel, state=st, source=_to(ops, S, gpu) if S else None,
                  conductivity=_to(ops, C, gpu))
    torch.cuda.synchronize()
    got = out.owned().cpu()
    assert torch.equal(got, want), f"max diff {(got - want).abs().max().item()}"
    assert ops.residual_from_state(st, 0) == res
    # the conductivity is seen: the same launch without it gives another field
    out2 = ops.PaddedField(n, dtype=dtype, device=gpu)
    ops.ftcs_step(_to(ops, T, gpu), out2, D, kernel=kernel, source=_to(ops, S, gpu) if S else None)
    torch.cuda.synchronize()
    assert not torch.equal(out2.owned().cpu(), want)


@pytest.mark.parametrize("with_source", [False, True])
@pytest.mark.parametrize("kernel", ["tile", "naive"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_sub_box_writes_nothing_outside(h3d, gpu, kernel, dtype, with_source):
    """The masked tail, with the first z point of the box unaligned."""
    ops = h3d.ops
    n, box = (12, 14, 200), [3, 7, 2, 9, 5, 133]
    T, C = _rand(ops, n, dtype, 4), _cond(ops, n, dtype, 5)
    S = _source(ops, n, dtype, 6) if with_source else None
    want, _ = ops.ftcs_reference(T.ghosted(), D, src=S.owned() if S else None, cond=C.ghosted())
    out = ops.PaddedField(n, dtype=dtype, device=gpu)
    out.flat.fill_(-7.0)
    ops.ftcs_step(_to(ops, T, gpu), out, D, box=box, kernel=kernel, source=_to(ops, S, gpu) if S else None,
                  conductivity=_to(ops, C, gpu))
    torch.cuda.synchronize()
    ref = ops.PaddedField(n, dtype=dtype)
    ref.flat.fill_(-7.0)
    x0, x1, y0, y1, z0, z1 = box
    ref.owned()[x0:x1, y0:y1, z0:z1] = want[x0:x1, y0:y1, z0:z1]
    assert torch.equal(out.flat.cpu(), ref.flat)


def test_sweep_with_conductivity_is_an_error(h3d, gpu):
    ops = h3d.ops
    n, dtype = (8, 40, 70), torch.float64
    T, C = _rand(ops, n, dtype, 7), _cond(ops, n, dtype, 8)
    out = ops.PaddedField(n, dtype=dtype, device=gpu)
    with pytest.raises(RuntimeError, match="no conductivity form"):
        ops.sweep(_to(ops, T, gpu), out, D, [0, n[0], 0, n[1], 0, n[2]], kernel="tl3", conductivity=_to(ops, C, gpu))


N_SOLVER = (33, 29, 37)


def _cq():
    rng = np.random.default_rng(5)
    return rng.uniform(0.05, 1.0, N_SOLVER), rng.uniform(-50.0, 50.0, N_SOLVER)


@pytest.fixture(scope="module")
def cpu_fields(h3d):
    """CPU-backend fields after 50 steps with the seeded conductivity and source, per dtype."""
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
@pytest.mark.parametrize("vr,dec,graph", [(1, None, True), (8, (2, 2, 2), True), (1, None, False)])
def test_solver_gpu_equals_cpu(h3d, gpu, cpu_fields, dt, vr, dec, graph):
    s = h3d.HeatSolver(N_SOLVER, 1000, 0.0, dtype=dt, backend="hip", virtual_ranks=vr, decomp=dec, graph=graph)
    c, q = _cq()
    s.set_conductivity(c)
    s.set_source(q)
    # deep ghosts stay, the iterations run as single steps
    assert s.native.temporal_blocking and not s.native.sweeps_active
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
        s = h3d.HeatSolver(n, 200000, 1e-4, backend=backend)
        c = s.model.layered_conductivity(0.25, 1.0)
        p = s.model.layered_steady(c)
        T0 = p.copy()
        T0[1:-1, 1:-1, 1:-1] = 0.0
        s.set_conductivity(c)
        s.set_field(T0)
        r = s.run()
        assert r["converged"]
        res.append((r["conv_iter"], r["last_residual"], s.gather()))
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    assert np.array_equal(res[0][2], res[1][2])


def test_solver_clear_returns_to_sweeps(h3d, gpu):
    fresh = h3d.HeatSolver(N_SOLVER, 1000, 0.0, backend="hip")
    fresh.step(50)
    fresh.synchronize()
    assert fresh.native.sweeps_active
    s = h3d.HeatSolver(N_SOLVER, 1000, 0.0, backend="hip")
    s.set_conductivity(_cq()[0])
    s.step(10)
    s.synchronize()
    assert not s.native.sweeps_active and "tl" not in s.kernel
    s.clear_conductivity()
    assert s.native.sweeps_active and "tl" in s.kernel
    s.initialize()
    s.step(50)
    s.synchronize()
    assert np.array_equal(s.gather(), fresh.gather())
