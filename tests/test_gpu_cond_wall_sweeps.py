"""The wall forms of the tv kernels (stencil_tbv_wall.hip, stencil_tbv_conv.hip:
K-step sweeps with a conductivity field behind insulated or convective walls) on
the GPU against the CPU K-single-steps definition bit for bit (field and all K
residual slots; every built form: insulated or convective, with and without a
heat source, tv2 and tv3, both dtypes; the tile edge cases of
test_gpu_cond_sweeps.py with all six faces walled, one face per axis, walls
inside deep halos; the sub-box store mask; the done flag; a depth without a
form), and the solver with --conductivity-sweeps behind walls: GPU == CPU
backend and flag on == flag off across decompositions and graph modes, the
convergence iteration, the steady state of the layered slab."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D = (0.06, 0.05, 0.04)
DTYPES = [torch.float64, torch.float32]
KERNELS = ["tv2", "tv3"]  # every built depth
EPS = {"fp64": float(np.finfo(np.float64).eps), "fp32": float(np.finfo(np.float32).eps)}
SENTINEL = -5.0


def _mixed(mask):
    """Convective coefficients for a face mask: every other walled face
    convective (0.25 .. 0.75), the others insulated; at least one convective."""
    betas = (0.25, -1.0, 0.5, -1.0, -1.0, 0.75)
    conv = [b if (mask >> f) & 1 else -1.0 for f, b in enumerate(betas)]
    if all(b < 0 for b in conv):  # the mask's first face
        f = next(f for f in range(6) if (mask >> f) & 1)
        conv[f] = 0.5
    return conv


FORMS = {"insulated": lambda mask: (None, 0.0), "convective": lambda mask: (_mixed(mask), 0.375)}


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


def _both(ops, gpu, call, T, C, S, fill=SENTINEL):
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
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [(9, 13, 130), (6, 100, 70), (5, 3, 64), (3, 30, 7), (33, 1, 513)])
def test_sweep_matches_cpu(h3d, gpu, n, dtype, kernel, form, with_source):
    """Every built form with all six faces walled.  (9, 13, 130): three z tiles
    with a masked tail; (6, 100, 70): at least two y tiles for any tile height up
    to 96 rows, and a z seam; (5, 3, 64): fewer rows than one wave holds;
    (3, 30, 7): narrower than a tile's halo; (33, 1, 513): a single row (both y
    walls on it)."""
    ops = h3d.ops
    T, C = _field(ops, n, dtype, 1), _cond(ops, n, dtype, 2)
    S = _source(ops, n, dtype, 3) if with_source else None
    box, u = [0, n[0], 0, n[1], 0, n[2]], (0, -1, 0, -1, 0, -1)
    walls = ops.wall_coords(63, n)
    conv, ambient = FORMS[form](63)

    def call(src, dst, st, q, c):
        ops.sweep3(src, dst, D, box, u, kernel=kernel, state=st, source=q, conductivity=c, walls=walls, conv=conv,
                   ambient=ambient)

    want, got, rc, rg = _both(ops, gpu, call, T, C, S)
    bad = (got != want).nonzero()
    assert not len(bad), f"{len(bad)} values differ, first flat index {int(bad[0])}"
    assert rc == rg, (rc, rg)
    K = int(kernel[2])
    assert all(r > 1e-300 for r in rg[:K])  # every stage recorded its residual
    # the walls matter on this box: the sweep without them gives another field
    plain = ops.PaddedField(n, dtype=dtype)
    ops.sweep3(T, plain, D, box, u, kernel=kernel, source=S, conductivity=C)
    ref = ops.PaddedField(n, dtype=dtype)
    ref.flat.copy_(want)
    assert not torch.equal(plain.owned(), ref.owned())


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mask", [0b010101, 0b101010], ids=["low", "high"])
def test_one_face_per_axis(h3d, gpu, mask, dtype, kernel, form):
    """Only the low, or only the high, face of each axis walled: both sides of
    every compare (plane, row bits, lane mask) on their own."""
    ops = h3d.ops
    n = (9, 13, 130)
    T, C, S = _field(ops, n, dtype, 21), _cond(ops, n, dtype, 22), _source(ops, n, dtype, 23)
    box, u = [0, n[0], 0, n[1], 0, n[2]], (0, -1, 0, -1, 0, -1)
    walls = ops.wall_coords(mask, n)
    conv, ambient = FORMS[form](mask)

    def call(src, dst, st, q, c):
        ops.sweep3(src, dst, D, box, u, kernel=kernel, state=st, source=q, conductivity=c, walls=walls, conv=conv,
                   ambient=ambient)

    want, got, rc, rg = _both(ops, gpu, call, T, C, S)
    assert torch.equal(got, want), f"max diff {(got - want).abs().max().item()}"
    assert rc == rg, (rc, rg)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_walls_inside_deep_halos(h3d, gpu, dtype, kernel, form):
    """Deep ghosts and update ranges on every axis (block decompositions): the
    block starts at global (2, 1, 1) of a grid that ends one vertex after its y
    and z extents, so the x- wall-adjacent plane (-1) and the y+ / z+
    wall-adjacent row and column (n) are computed inside the halos; x+, y- and z-
    have no wall (NO_WALL).  Nothing is updated beyond a wall-adjacent plane."""
    ops = h3d.ops
    K = int(kernel[2])
    n, box = (12, 50, 140), (0, 12, 0, 50, 0, 140)
    mask = 0b101001  # x-, y+, z+
    walls = ops.wall_coords(mask, n, gstart=(2, 1, 1), N=(n[0] + 100, n[1] + 3, n[2] + 3))
    none = h3d.native().NO_WALL
    assert walls == [-1, none, none, n[1], none, n[2]]
    u = [max(-(K - 1), -1), n[0] + K - 1, -(K - 1), min(n[1] + K - 1, n[1] + 1), -(K - 1), min(n[2] + K - 1, n[2] + 1)]
    g = (K, K, K)
    T, C, S = _field(ops, n, dtype, 11, g), _cond(ops, n, dtype, 12, g), _source(ops, n, dtype, 13, g)
    conv, ambient = FORMS[form](mask)

    def call(src, dst, st, q, c):
        ops.sweep3(src, dst, D, box, u, kernel=kernel, state=st, source=q, conductivity=c, walls=walls, conv=conv,
                   ambient=ambient)

    want, got, rc, rg = _both(ops, gpu, call, T, C, S)
    assert torch.equal(got, want), f"max diff {(got - want).abs().max().item()}"
    assert rc == rg, (rc, rg)
    # the halo walls are seen
    plain = ops.PaddedField(n, dtype=dtype, gx=K, gy=K, gz=K)
    ops.sweep3(T, plain, D, box, u, kernel=kernel, source=S, conductivity=C)
    ref = ops.PaddedField(n, dtype=dtype, gx=K, gy=K, gz=K)
    ref.flat.copy_(want)
    assert not torch.equal(plain.owned(), ref.owned())


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n0,box_x,side", [(4, (0, 4), "both"), (9, (0, 9), "hi"), (12, (4, 8), "both")])
def test_x_slab_deep_halo_with_yz_walls(h3d, gpu, kernel, dtype, form, n0, box_x, side):
    """The x-slab cases of test_gpu_cond_sweeps.test_sweep_deep_halo_matches_cpu
    (K-plane ghost layers, the x update range widened into them) with walls on
    the four y and z faces."""
    ops = h3d.ops
    K = int(kernel[2])
    n = (n0, 37, 133)
    u = (-(K - 1) if side in ("lo", "both") else 0, n0 + (K - 1 if side in ("hi", "both") else 0), 0, -1, 0, -1)
    box = (box_x[0], box_x[1], 0, n[1], 0, n[2])
    g = (K, 1, 1)
    mask = 0b111100
    walls = ops.wall_coords(mask, n)
    conv, ambient = FORMS[form](mask)
    T, C, S = _field(ops, n, dtype, 7, g), _cond(ops, n, dtype, 8, g), _source(ops, n, dtype, 9, g)

    def call(src, dst, st, q, c):
        ops.sweep3(src, dst, D, box, u, kernel=kernel, state=st, source=q, conductivity=c, walls=walls, conv=conv,
                   ambient=ambient)

    want, got, rc, rg = _both(ops, gpu, call, T, C, S)
    assert torch.equal(got, want), f"max diff {(got - want).abs().max().item()}"
    assert rc == rg, (rc, rg)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_sub_box_writes_nothing_outside(h3d, gpu, kernel, dtype, form):
    """A sub-box that touches the x-, y+ and z+ walls."""
    ops = h3d.ops
    n, box = (12, 14, 200), [0, 7, 2, 14, 5, 200]
    T, C = _field(ops, n, dtype, 4), _cond(ops, n, dtype, 5)
    walls = ops.wall_coords(63, n)
    conv, ambient = FORMS[form](63)

    def call(src, dst, st, q, c):
        ops.sweep3(src, dst, D, box, (0, -1, 0, -1, 0, -1), kernel=kernel, state=st, conductivity=c, walls=walls,
                   conv=conv, ambient=ambient)

    want, got, rc, rg = _both(ops, gpu, call, T, C, None, fill=-7.0)
    assert torch.equal(got, want) and rc == rg
    x0, x1, y0, y1, z0, z1 = box
    ref = ops.PaddedField(n, dtype=dtype)
    ref.flat.copy_(got)
    assert (ref.owned()[x0:x1, y0:y1, z0:z1] != -7.0).all()
    ref.owned()[x0:x1, y0:y1, z0:z1] = -7.0
    assert (ref.flat == -7.0).all()


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kernel", KERNELS)
def test_done_flag_writes_nothing(h3d, gpu, kernel, form):
    ops, ext = h3d.ops, h3d.native()
    n, dtype = (9, 13, 130), torch.float64
    T, C = _to(ops, _field(ops, n, dtype, 1), gpu), _to(ops, _cond(ops, n, dtype, 2), gpu)
    out = ops.PaddedField(n, dtype=dtype, device=gpu)
    out.flat.fill_(-7.0)
    st = ops.new_state(gpu)
    st.view(torch.int32)[ext.STATE_DONE_OFFSET // 4] = 1
    before = st.clone()
    conv, ambient = FORMS[form](63)
    ops.sweep3(T, out, D, [0, n[0], 0, n[1], 0, n[2]], (0, -1, 0, -1, 0, -1), kernel=kernel, state=st, conductivity=C,
               walls=ops.wall_coords(63, n), conv=conv, ambient=ambient)
    torch.cuda.synchronize()
    assert (out.flat == -7.0).all() and torch.equal(st, before)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_depth_without_a_form_raises_and_writes_nothing(h3d, gpu, form):
    """tv4 has no form at all, with or without walls; a tv spec without a
    conductivity keeps its own error."""
    ops = h3d.ops
    n, dtype = (9, 13, 130), torch.float64
    T, C = _to(ops, _field(ops, n, dtype, 1), gpu), _to(ops, _cond(ops, n, dtype, 2), gpu)
    out = ops.PaddedField(n, dtype=dtype, device=gpu)
    out.flat.fill_(-7.0)
    conv, ambient = FORMS[form](63)
    kw = dict(walls=ops.wall_coords(63, n), conv=conv, ambient=ambient)
    box, u = [0, n[0], 0, n[1], 0, n[2]], (0, -1, 0, -1, 0, -1)
    assert h3d.native().cond_sweep_shape("fp64", "tv4", False, 1 if conv is None else 2) is None
    with pytest.raises(RuntimeError, match="tv"):
        ops.sweep3(T, out, D, box, u, kernel="tv4", conductivity=C, **kw)
    with pytest.raises(RuntimeError, match="need a conductivity"):
        ops.sweep3(T, out, D, box, u, kernel="tv3", **kw)
    torch.cuda.synchronize()
    assert (out.flat == -7.0).all()


# ---- the solver

N33 = (33, 33, 33)
STEPS = 26  # eight sweeps of three steps and a partial sweep of two
FACE_SETS = {"insulated": dict(insulated="x-,y+,z-", convective=None, ambient=0.0),
             "mixed": dict(insulated="x-,z+", convective={"y+": 0.5, "z-": 0.75}, ambient=0.375)}


def _inputs():
    rng = np.random.default_rng(5)
    return rng.uniform(0.0, 1.0, N33), rng.uniform(0.05, 1.0, N33), rng.uniform(-50.0, 50.0, N33)


def _run(h3d, backend, dt, faces, with_source, flag, steps=STEPS, **kw):
    s = h3d.HeatSolver(N33, 1000, 0.0, dtype=dt, backend=backend, conductivity_sweeps=flag, **FACE_SETS[faces], **kw)
    T0, c, q = _inputs()
    s.set_conductivity(c)
    if with_source:
        s.set_source(q)
    s.set_field(T0)
    assert s.native.sweeps_active == flag
    s.step(steps)
    s.synchronize()
    assert s.state()["iter"] == steps
    return s, s.gather(), s.native.residual_history()


@pytest.fixture(scope="module")
def cpu_flag_on(h3d):
    """CPU backend, flag on (K = 3 sweeps of the definition), per dtype, face set and source."""
    out = {}
    for dt in ("fp64", "fp32"):
        for faces in FACE_SETS:
            for with_source in (False, True):
                out[dt, faces, with_source] = _run(h3d, "cpu", dt, faces, with_source, True,
                                                   extra_args=["--temporal", "3"])[1:]
    return out


@pytest.mark.parametrize("with_source", [False, True])
@pytest.mark.parametrize("faces", sorted(FACE_SETS))
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
@pytest.mark.parametrize("vr,dec,graph", [(1, None, True), (2, (2, 1, 1), True), (4, (1, 2, 2), True), (1, None, False)])
def test_solver_gpu_equals_cpu(h3d, gpu, cpu_flag_on, dt, faces, with_source, vr, dec, graph):
    s, T, hist = _run(h3d, "hip", dt, faces, with_source, True, virtual_ranks=vr, decomp=dec, graph=graph)
    assert s.native.temporal_blocking and s.kernel.startswith("tv3"), s.kernel
    want, whist = cpu_flag_on[dt, faces, with_source]
    assert hist == whist
    assert np.array_equal(T, want)
    if graph and vr == 1:
        assert s.native.graph_launches > 0


@pytest.mark.parametrize("with_source", [False, True])
@pytest.mark.parametrize("faces", sorted(FACE_SETS))
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
def test_solver_flag_on_equals_flag_off(h3d, gpu, cpu_flag_on, dt, faces, with_source):
    """The single-step path of the same build (flag off) on the GPU: the same bits."""
    s, T, hist = _run(h3d, "hip", dt, faces, with_source, False)
    assert not s.kernel.startswith("tv"), s.kernel
    want, whist = cpu_flag_on[dt, faces, with_source]
    assert hist == whist
    assert np.array_equal(T, want)


def test_solver_convergence_equals_cpu(h3d, gpu):
    """A run to convergence at a small eps: the same conv_iter, last residual and
    field on both backends (the rollback inside a sweep)."""
    res = []
    for backend in ("cpu", "hip"):
        s = h3d.HeatSolver(N33, 200000, 1e-4, backend=backend, conductivity_sweeps=True,
                           extra_args=["--temporal", "3"], **FACE_SETS["mixed"])
        T0, c, _ = _inputs()
        s.set_conductivity(c)
        s.set_field(T0)
        assert s.native.sweeps_active
        r = s.run()
        assert r["converged"]
        res.append((r["conv_iter"], r["last_residual"], s.gather()))
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    assert np.array_equal(res[0][2], res[1][2])


@pytest.mark.parametrize("dt", ["fp64", "fp32"])
def test_layered_slab_steady_state(h3d, gpu, dt):
    """layered_convective_slab_steady is a fixed point of the tv wall sweeps on
    (5, 33, 5): the tolerance of tests/test_cond_wall_sweeps_cpu.py, 8 u * 20
    after 20 steps."""
    N = (5, 33, 5)
    s = h3d.HeatSolver(N, 1000, 0.0, dtype=dt, backend="hip", conductivity_sweeps=True, insulated="x-,x+,z-,z+",
                       convective={"y-": 0.5}, ambient=0.25)
    c = s.model.layered_conductivity(0.25, 1.0)
    p = s.model.layered_convective_slab_steady(c, 0.5, 0.25)
    s.set_conductivity(c)
    s.set_field(p)
    assert s.native.sweeps_active and s.kernel.startswith("tv3"), s.kernel
    s.step(20)
    s.synchronize()
    moved = np.abs(s.gather() - p).max()
    print(f"layered slab {dt}: moved {moved:.3e}, tolerance {8 * EPS[dt] * 20:.3e}")
    assert moved <= 8 * EPS[dt] * 20
