"""Volumetric heat source on the GPU: the single-step kernels (tile, naive) and
the K-step lean sweep kernel in their source forms against the PyTorch oracle
and the CPU K-single-steps definition, bit for bit (field and every residual
slot), and the solver with a source: GPU == CPU backend, decomposition and
graph invariance, and the exact convergence iteration through the rollback."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D = (0.06, 0.05, 0.04)
DTYPES = [torch.float64, torch.float32]


def _rand(ops, n, dtype, seed, g=(1, 1, 1), scale=1.0, shift=0.0):
    """Random values on every ghost layer of every axis (host field)."""
    gen = torch.Generator().manual_seed(seed)
    f = ops.PaddedField(n, dtype=dtype, gx=g[0], gy=g[1], gz=g[2])
    v = f.deep3()
    v.copy_(((torch.rand(v.shape, generator=gen, dtype=torch.float64) - shift) * scale).to(dtype))
    return f


def _source(ops, n, dtype, seed, g=(1, 1, 1)):
    # S of the size of a real dt * q, either sign, non-zero on the ghosts too
    return _rand(ops, n, dtype, seed, g, scale=2e-3, shift=0.5)


def _to(ops, f, gpu):
    d = ops.PaddedField(f.n, dtype=f.dtype, device=gpu, gx=f.gx, gy=f.gy, gz=f.gz)
    d.flat.copy_(f.flat)
    return d


def _oracle_steps(ops, T, S, K):
    """K oracle steps with fixed ghosts: (owned field, residuals)."""
    T = T.ghosted().clone()
    res = []
    for _ in range(K):
        u, r = ops.ftcs_reference(T, D, src=S.owned())
        T = T.clone()
        T[1:-1, 1:-1, 1:-1] = u
        res.append(r)
    return T[1:-1, 1:-1, 1:-1], res


@pytest.mark.parametrize("kernel", ["tile", "naive"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [(9, 13, 130), (5, 3, 64)])
def test_single_step_matches_oracle(h3d, gpu, kernel, dtype, n):
    ops = h3d.ops
    T, S = _rand(ops, n, dtype, 1), _source(ops, n, dtype, 2)
    want, res = _oracle_steps(ops, T, S, 1)
    out = ops.PaddedField(n, dtype=dtype, device=gpu)
    st = ops.new_state(gpu)
    ops.ftcs_step(_to(ops, T, gpu), out, D, kernel=kernel, state=st, source=_to(ops, S, gpu))
    torch.cuda.synchronize()
    assert torch.equal(out.owned().cpu(), want)
    assert ops.residual_from_state(st, 0) == res[0]


@pytest.mark.parametrize("kernel", ["tile", "naive"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_single_step_sub_box_writes_nothing_outside(h3d, gpu, kernel, dtype):
    ops = h3d.ops
    n, box = (12, 14, 200), [3, 7, 2, 9, 5, 133]
    T, S = _rand(ops, n, dtype, 3), _source(ops, n, dtype, 4)
    want, _ = _oracle_steps(ops, T, S, 1)
    out = ops.PaddedField(n, dtype=dtype, device=gpu)
    out.flat.fill_(-7.0)
    ops.ftcs_step(_to(ops, T, gpu), out, D, box=box, kernel=kernel, source=_to(ops, S, gpu))
    torch.cuda.synchronize()
    exp = torch.full_like(out.flat, -7.0).cpu()
    ref = ops.PaddedField(n, dtype=dtype)
    ref.flat.copy_(exp)
    x0, x1, y0, y1, z0, z1 = box
    ref.owned()[x0:x1, y0:y1, z0:z1] = want[x0:x1, y0:y1, z0:z1]
    assert torch.equal(out.flat.cpu(), ref.flat)


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [(7, 50, 70), (40, 45, 130)])
def test_lean_sweep_matches_oracle(h3d, gpu, K, dtype, n):
    """(7, 50, 70): two tiles in y and z, every step fill / drain / masked;
    (40, 45, 130): the mask-free fast path runs."""
    ops = h3d.ops
    T, S = _rand(ops, n, dtype, 5), _source(ops, n, dtype, 6)
    want, res = _oracle_steps(ops, T, S, K)
    out = ops.PaddedField(n, dtype=dtype, device=gpu)
    out.flat.fill_(-3.0)
    st = ops.new_state(gpu)
    ops.sweep(_to(ops, T, gpu), out, D, [0, n[0], 0, n[1], 0, n[2]], kernel=f"tl{K}", state=st,
              source=_to(ops, S, gpu))
    torch.cuda.synchronize()
    got = out.owned().cpu()
    assert torch.equal(got, want), f"max diff {(got - want).abs().max().item()}"
    assert [ops.residual_from_state(st, s) for s in range(K)] == res


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("box", [(0, 12, 0, 50, 0, 140), (3, 9, 4, 46, 5, 135)])
def test_sweep3_deep_halos_match_cpu(h3d, gpu, K, dtype, box):
    """Deep ghosts (K, K, K), update ranges widened into them, random non-zero
    source ghosts: a wrong source plane, row or column changes the result."""
    ops = h3d.ops
    n, g = (12, 50, 140), (K, K, K)
    u = []
    for a in range(3):
        u += [-(K - 1), n[a] + K - 1]
    T, S = _rand(ops, n, dtype, 7, g), _source(ops, n, dtype, 8, g)
    want = ops.PaddedField(n, dtype=dtype, gx=K, gy=K, gz=K)
    want.flat.fill_(-5.0)
    st_c = ops.new_state("cpu")
    ops.sweep3(T, want, D, box, u, kernel=f"tl{K}", state=st_c, source=S)
    got = ops.PaddedField(n, dtype=dtype, device=gpu, gx=K, gy=K, gz=K)
    got.flat.fill_(-5.0)
    st_g = ops.new_state(gpu)
    ops.sweep3(_to(ops, T, gpu), got, D, box, u, kernel=f"tl{K}", state=st_g, source=_to(ops, S, gpu))
    torch.cuda.synchronize()
    assert torch.equal(got.flat.cpu(), want.flat)
    assert [ops.residual_from_state(st_g, s) for s in range(K)] == \
        [ops.residual_from_state(st_c, s) for s in range(K)]
    # the source is seen: without it the CPU definition gives another field
    plain = ops.PaddedField(n, dtype=dtype, gx=K, gy=K, gz=K)
    plain.flat.fill_(-5.0)
    ops.sweep3(T, plain, D, box, u, kernel=f"tl{K}")
    assert not torch.equal(plain.flat, want.flat)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,n,bx", [(3, (4, 60, 70), (0, 3)), (3, (4, 60, 70), (0, 4)), (3, (4, 70, 70), (0, 4)),
                                    (4, (4, 70, 70), (0, 4))])
def test_thin_slab_matches_cpu(h3d, gpu, dtype, K, n, bx):
    """Thin x slabs through ops.sweep with gx = K: 3 planes of 60 rows and 4 of
    70 take the y-marching tiles (3-wave, 5-wave; K = 4: 4-wave), 4 planes of
    60 rows the x-marching default."""
    ops = h3d.ops
    g = (K, 1, 1)
    ux = (-(K - 1), n[0] + K - 1)
    box = (bx[0], bx[1], 0, n[1], 0, n[2])
    T, S = _rand(ops, n, dtype, 9, g), _source(ops, n, dtype, 10, g)
    want = ops.PaddedField(n, dtype=dtype, gx=K)
    want.flat.fill_(-5.0)
    st_c = ops.new_state("cpu")
    ops.sweep(T, want, D, box, ux, kernel=f"tl{K}", state=st_c, source=S)
    got = ops.PaddedField(n, dtype=dtype, device=gpu, gx=K)
    got.flat.fill_(-5.0)
    st_g = ops.new_state(gpu)
    ops.sweep(_to(ops, T, gpu), got, D, box, ux, kernel=f"tl{K}", state=st_g, source=_to(ops, S, gpu))
    torch.cuda.synchronize()
    assert torch.equal(got.flat.cpu(), want.flat)
    assert [ops.residual_from_state(st_g, s) for s in range(K)] == \
        [ops.residual_from_state(st_c, s) for s in range(K)]


def test_residual_last_only_variant(h3d, gpu):
    ops = h3d.ops
    n, K, dtype = (20, 50, 70), 3, torch.float64
    T, S = _rand(ops, n, dtype, 11), _source(ops, n, dtype, 12)
    dT, dS = _to(ops, T, gpu), _to(ops, S, gpu)
    outs, last = [], []
    for spec in ("tl3:1:3:1:16:0:3:2", "tl3:1:3:1:16:0:3:66"):
        out = ops.PaddedField(n, dtype=dtype, device=gpu)
        st = ops.new_state(gpu)
        ops.sweep(dT, out, D, [0, n[0], 0, n[1], 0, n[2]], kernel=spec, state=st, source=dS)
        torch.cuda.synchronize()
        outs.append(out.owned().cpu())
        last.append(ops.residual_from_state(st, K - 1))
    want, res = _oracle_steps(ops, T, S, K)
    assert torch.equal(outs[0], want) and torch.equal(outs[1], want)
    assert last[0] == last[1] == res[K - 1]


def test_spec_without_source_form_is_an_error(h3d, gpu):
    ops = h3d.ops
    n, dtype = (8, 40, 70), torch.float64
    T, S = _rand(ops, n, dtype, 13), _source(ops, n, dtype, 14)
    out = ops.PaddedField(n, dtype=dtype, device=gpu)
    for spec in ("tl3:1:2:1:16:0:3", "tl3:2", "tl5"):
        with pytest.raises(RuntimeError, match="no heat-source form"):
            ops.sweep(_to(ops, T, gpu), out, D, [0, n[0], 0, n[1], 0, n[2]], kernel=spec, source=_to(ops, S, gpu))
    s = h3d.HeatSolver((33, 29, 37), 100, 0.0, backend="hip", extra_args=["--kernel2", "tl3:1:2:1:16:0:3"])
    with pytest.raises(RuntimeError, match="no heat-source form"):
        s.set_source(np.ones((33, 29, 37)))
        s.step(6)
        s.synchronize()


N_SOLVER = (33, 29, 37)


def _q():
    return np.random.default_rng(5).uniform(-50.0, 50.0, N_SOLVER)


@pytest.fixture(scope="module")
def cpu_fields(h3d):
    """CPU-backend fields after 50 steps with the seeded source, per dtype."""
    out = {}
    for dt in ("fp64", "fp32"):
        s = h3d.HeatSolver(N_SOLVER, 1000, 0.0, dtype=dt, backend="cpu")
        s.set_source(_q())
        s.step(50)
        s.synchronize()
        out[dt] = s.gather()
    return out


@pytest.mark.parametrize("dt", ["fp64", "fp32"])
@pytest.mark.parametrize("vr,dec,graph", [(1, None, True), (8, (2, 2, 2), True), (1, None, False)])
def test_solver_gpu_equals_cpu(h3d, gpu, cpu_fields, dt, vr, dec, graph):
    s = h3d.HeatSolver(N_SOLVER, 1000, 0.0, dtype=dt, backend="hip", virtual_ranks=vr, decomp=dec, graph=graph)
    s.set_source(_q())
    assert s.native.temporal_blocking
    # fp32 source runs compute every residual
    assert not (dt == "fp32" and s.native.monotone_check)
    s.step(50)
    s.synchronize()
    assert np.array_equal(s.gather(), cpu_fields[dt])


@pytest.mark.parametrize("vr,dec,extra", [(1, None, []), (8, (2, 2, 2), ["--long-sweeps", "off"])])
def test_exact_convergence_iteration(h3d, gpu, vr, dec, extra):
    """run() with a source: the default schedule (K-step sweeps, rollback
    through the single-step source kernel) == --temporal 1."""
    n = (33, 33, 33)
    res = []
    for e in (extra, extra + ["--temporal", "1"]):
        s = h3d.HeatSolver(n, 100000, 1e-4, backend="hip", virtual_ranks=vr, decomp=dec, extra_args=e)
        s.set_source(s.model.sine_source(0.25))
        r = s.run()
        assert r["converged"]
        res.append((r["conv_iter"], r["last_residual"], s.gather()))
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    assert np.array_equal(res[0][2], res[1][2])
