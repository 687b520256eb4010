"""The tc kernels (stencil_tbc.hip, stencil_tbc_wall.hip, stencil_tbc_conv.hip:
K-step sweeps with a conductivity field and a heat capacity) on the GPU against
the CPU K-single-steps definition bit for bit (the whole flat field and all K
residual slots; both dtypes, tc2 and tc3, with and without a heat source; the
tile edge cases, deep halos, update ranges, store mask, done flag and NaN of
tests/test_gpu_cond_sweeps.py; the wall cases of
tests/test_gpu_cond_wall_sweeps.py), and the solver with --capacity-sweeps: the
GPU with the flag equals the CPU backend without it across decompositions and
graph modes, the convergence iteration, the heat balance."""
import numpy as np
import pytest
import torch

import _value_fields as vf

pytestmark = pytest.mark.gpu

D = (0.06, 0.05, 0.04)
DTYPES = [torch.float64, torch.float32]
DT = {torch.float64: "fp64", torch.float32: "fp32"}
KERNELS = ["tc2", "tc3"]
SENTINEL = -5.0
BOXES = [(9, 13, 130), (6, 100, 70), (5, 3, 64), (3, 30, 7), (33, 1, 513)]


def _mixed(mask):
    """Convective coefficients for a face mask (tests/test_gpu_cond_wall_sweeps.py):
    every other walled face convective, the others insulated; at least one convective."""
    betas = (0.25, -1.0, 0.5, -1.0, -1.0, 0.75)
    conv = [b if (mask >> f) & 1 else -1.0 for f, b in enumerate(betas)]
    if all(b < 0 for b in conv):
        f = next(f for f in range(6) if (mask >> f) & 1)
        conv[f] = 0.5
    return conv


FORMS = {"insulated": lambda mask: (None, 0.0), "convective": lambda mask: (_mixed(mask), 0.375)}
WALL = {"none": 0, "insulated": 1, "convective": 2}


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


def _cap(ops, n, dtype, seed, g=(1, 1, 1)):
    # s = dtype(1 / rc), rc in [1, 9), on every ghost layer
    f = _field(ops, n, dtype, seed, g, 1.0, 9.0)
    f.deep3().copy_((1.0 / f.deep3().double()).to(dtype))
    return f


def _to(ops, f, gpu):
    if f is None:
        return None
    d = ops.PaddedField(f.n, dtype=f.dtype, device=gpu, gx=f.gx, gy=f.gy, gz=f.gz)
    d.flat.copy_(f.flat)
    return d


def _need(h3d, dtype, kernel, with_source, form="none"):
    """Skips a depth only where the form is not built (tc2 always is:
    test_every_form_has_a_depth_2_kernel)."""
    if not h3d.native().cap_sweep_supported(DT[dtype], kernel, with_source, WALL[form]):
        assert kernel != "tc2"
        pytest.skip(f"{kernel} {DT[dtype]} source={with_source} walls={form}: not built, runs at depth 2")


def _both(ops, gpu, call, T, C, S, A, fill=SENTINEL):
    """Runs call(src, dst, state, source, conductivity, cap) on host and on GPU
    fields; returns (want, got, residuals_cpu, residuals_gpu), fields as host
    flat tensors."""
    want = ops.PaddedField(T.n, dtype=T.dtype, gx=T.gx, gy=T.gy, gz=T.gz)
    want.flat.fill_(fill)
    st_c = ops.new_state("cpu")
    call(T, want, st_c, S, C, A)
    got = _to(ops, want, gpu)
    got.flat.fill_(fill)
    st_g = ops.new_state(gpu)
    call(_to(ops, T, gpu), got, st_g, _to(ops, S, gpu), _to(ops, C, gpu), _to(ops, A, gpu))
    torch.cuda.synchronize()
    res = lambda st: [ops.residual_from_state(st, s) for s in range(4)]
    return want.flat, got.flat.cpu(), res(st_c), res(st_g)


def test_every_form_has_a_depth_2_kernel(h3d):
    ext = h3d.native()
    for dt in ("fp64", "fp32"):
        for src in (False, True):
            for wall in (0, 1, 2):
                assert ext.cap_sweep_max_depth(dt, src, wall) >= 2, (dt, src, wall)


@pytest.mark.parametrize("with_source", [False, True])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", BOXES)
def test_sweep_matches_cpu(h3d, gpu, n, dtype, kernel, with_source):
    """(9, 13, 130): three z tiles with a masked tail; (6, 100, 70): at least two
    y tiles for any tile height up to 96 rows, and a z seam; (5, 3, 64): fewer
    rows than one wave holds; (3, 30, 7): narrower than a tile's halo;
    (33, 1, 513): a single row."""
    _need(h3d, dtype, kernel, with_source)
    ops = h3d.ops
    T, C, A = _field(ops, n, dtype, 1), _cond(ops, n, dtype, 2), _cap(ops, n, dtype, 6)
    S = _source(ops, n, dtype, 3) if with_source else None
    box = [0, n[0], 0, n[1], 0, n[2]]

    def call(src, dst, st, q, c, a):
        ops.sweep(src, dst, D, box, kernel=kernel, state=st, source=q, conductivity=c, cap=a)

    want, got, rc, rg = _both(ops, gpu, call, T, C, S, A)
    assert vf.same_bits(got, want)
    assert rc == rg, (rc, rg)
    K = int(kernel[2])
    assert all(r > 1e-300 for r in rg[:K])  # every stage recorded its residual


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n0,box_x,side", [(4, (0, 4), "both"), (9, (0, 9), "hi"), (12, (4, 8), "both")])
def test_sweep_deep_halo_matches_cpu(h3d, gpu, kernel, dtype, n0, box_x, side):
    """The slab path: K-plane ghost layers, the x update range widened into
    them; s is read on the ghost planes a stage updates."""
    _need(h3d, dtype, kernel, True)
    ops = h3d.ops
    K = int(kernel[2])
    n = (n0, 37, 133)
    ux = (-(K - 1) if side in ("lo", "both") else 0, n0 + (K - 1 if side in ("hi", "both") else 0))
    box = (box_x[0], box_x[1], 0, n[1], 0, n[2])
    g = (K, 1, 1)
    T, C, S, A = _field(ops, n, dtype, 7, g), _cond(ops, n, dtype, 8, g), _source(ops, n, dtype, 9, g), _cap(ops, n, dtype, 10, g)

    def call(src, dst, st, q, c, a):
        ops.sweep(src, dst, D, box, ux, kernel=kernel, state=st, source=q, conductivity=c, cap=a)

    want, got, rc, rg = _both(ops, gpu, call, T, C, S, A)
    assert vf.same_bits(got, want)
    assert rc == rg, (rc, rg)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep3_update_ranges_match_cpu(h3d, gpu, kernel, dtype):
    """Deep ghosts and update ranges on every axis (block decompositions)."""
    _need(h3d, dtype, kernel, False)
    ops = h3d.ops
    K = int(kernel[2])
    n, box = (12, 50, 140), (0, 12, 0, 50, 0, 140)
    u = []
    for a in range(3):
        u += [-(K - 1), n[a] + K - 1]
    g = (K, K, K)
    T, C, A = _field(ops, n, dtype, 11, g), _cond(ops, n, dtype, 12, g), _cap(ops, n, dtype, 14, g)

    def call(src, dst, st, q, c, a):
        ops.sweep3(src, dst, D, box, u, kernel=kernel, state=st, source=q, conductivity=c, cap=a)

    want, got, rc, rg = _both(ops, gpu, call, T, C, None, A)
    assert vf.same_bits(got, want)
    assert rc == rg, (rc, rg)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_sub_box_writes_nothing_outside(h3d, gpu, kernel, dtype):
    _need(h3d, dtype, kernel, False)
    ops = h3d.ops
    n, box = (12, 14, 200), [3, 7, 2, 9, 5, 133]
    T, C, A = _field(ops, n, dtype, 4), _cond(ops, n, dtype, 5), _cap(ops, n, dtype, 6)

    def call(src, dst, st, q, c, a):
        ops.sweep(src, dst, D, box, kernel=kernel, state=st, conductivity=c, cap=a)

    want, got, rc, rg = _both(ops, gpu, call, T, C, None, A, fill=-7.0)
    assert torch.equal(got, want) and rc == rg
    x0, x1, y0, y1, z0, z1 = box
    ref = ops.PaddedField(n, dtype=dtype)
    ref.flat.copy_(got)
    assert (ref.owned()[x0:x1, y0:y1, z0:z1] != -7.0).all()
    ref.owned()[x0:x1, y0:y1, z0:z1] = -7.0
    assert (ref.flat == -7.0).all()


@pytest.mark.parametrize("kernel", KERNELS)
def test_done_flag_writes_nothing(h3d, gpu, kernel):
    _need(h3d, torch.float64, kernel, False)
    ops, ext = h3d.ops, h3d.native()
    n, dtype = (9, 13, 130), torch.float64
    T, C, A = (_to(ops, f, gpu) for f in (_field(ops, n, dtype, 1), _cond(ops, n, dtype, 2), _cap(ops, n, dtype, 6)))
    out = ops.PaddedField(n, dtype=dtype, device=gpu)
    out.flat.fill_(-7.0)
    st = ops.new_state(gpu)
    st.view(torch.int32)[ext.STATE_DONE_OFFSET // 4] = 1
    before = st.clone()
    ops.sweep(T, out, D, [0, n[0], 0, n[1], 0, n[2]], kernel=kernel, state=st, conductivity=C, cap=A)
    torch.cuda.synchronize()
    assert (out.flat == -7.0).all() and torch.equal(st, before)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_spreads_as_on_the_cpu(h3d, gpu, kernel, dtype):
    """One NaN in the field: the CPU's bits (NaNs taken as equal), and every
    stage's residual says so."""
    _need(h3d, dtype, kernel, True)
    ops = h3d.ops
    n = (9, 50, 130)
    T = vf.spike(ops, "nan", (4, 17, 64), n, dtype, 9)
    C, S, A = _cond(ops, n, dtype, 2), _source(ops, n, dtype, 3), _cap(ops, n, dtype, 6)
    box = [0, n[0], 0, n[1], 0, n[2]]

    def call(src, dst, st, q, c, a):
        ops.sweep(src, dst, D, box, kernel=kernel, state=st, source=q, conductivity=c, cap=a)

    want, got, rc, rg = _both(ops, gpu, call, T, C, S, A)
    assert vf.same_bits(got, want)
    K = int(kernel[2])
    assert all(r != r for r in rc[:K]) and all(r != r for r in rg[:K])
    assert want.isnan().sum().item() > 1


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_capacity_is_seen(h3d, gpu, kernel, dtype):
    """The same launch with s = 1/2 everywhere differs from s = 1."""
    _need(h3d, dtype, kernel, False)
    ops = h3d.ops
    n = (9, 13, 130)
    box = [0, n[0], 0, n[1], 0, n[2]]
    T, C = _to(ops, _field(ops, n, dtype, 1), gpu), _to(ops, _cond(ops, n, dtype, 2), gpu)
    outs = []
    for s in (1.0, 0.5):
        A = ops.PaddedField(n, dtype=dtype, device=gpu)
        A.flat.fill_(s)
        out = ops.PaddedField(n, dtype=dtype, device=gpu)
        ops.sweep(T, out, D, box, kernel=kernel, conductivity=C, cap=A)
        torch.cuda.synchronize()
        outs.append(out.owned().cpu())
    assert not torch.equal(outs[0], outs[1])


def test_a_missing_field_is_an_error_and_writes_nothing(h3d, gpu):
    ops = h3d.ops
    n, dtype = (9, 13, 130), torch.float64
    T, C, A = (_to(ops, f, gpu) for f in (_field(ops, n, dtype, 1), _cond(ops, n, dtype, 2), _cap(ops, n, dtype, 6)))
    out = ops.PaddedField(n, dtype=dtype, device=gpu)
    out.flat.fill_(-7.0)
    box = [0, n[0], 0, n[1], 0, n[2]]
    with pytest.raises(RuntimeError, match="need a heat-capacity field"):
        ops.sweep(T, out, D, box, kernel="tc3", conductivity=C)
    with pytest.raises(RuntimeError, match="need a conductivity field"):
        ops.sweep(T, out, D, box, kernel="tc3", cap=A)
    with pytest.raises(RuntimeError, match="tc"):
        ops.sweep(T, out, D, box, kernel="tc4", conductivity=C, cap=A)
    torch.cuda.synchronize()
    assert (out.flat == -7.0).all()


# ---- the wall forms (the cases of tests/test_gpu_cond_wall_sweeps.py with the capacity added)

@pytest.mark.parametrize("with_source", [False, True])
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", BOXES)
def test_wall_sweep_matches_cpu(h3d, gpu, n, dtype, kernel, form, with_source):
    """Every built form with all six faces walled, on the boxes above."""
    _need(h3d, dtype, kernel, with_source, form)
    ops = h3d.ops
    T, C, A = _field(ops, n, dtype, 1), _cond(ops, n, dtype, 2), _cap(ops, n, dtype, 6)
    S = _source(ops, n, dtype, 3) if with_source else None
    box, u = [0, n[0], 0, n[1], 0, n[2]], (0, -1, 0, -1, 0, -1)
    walls = ops.wall_coords(63, n)
    conv, ambient = FORMS[form](63)

    def call(src, dst, st, q, c, a):
        ops.sweep3(src, dst, D, box, u, kernel=kernel, state=st, source=q, conductivity=c, cap=a, walls=walls,
                   conv=conv, ambient=ambient)

    want, got, rc, rg = _both(ops, gpu, call, T, C, S, A)
    assert vf.same_bits(got, want)
    assert rc == rg, (rc, rg)
    K = int(kernel[2])
    assert all(r > 1e-300 for r in rg[:K])
    # the walls matter on this box: the sweep without them gives another field
    plain = ops.PaddedField(n, dtype=dtype)
    ops.sweep3(T, plain, D, box, u, kernel=kernel, source=S, conductivity=C, cap=A)
    ref = ops.PaddedField(n, dtype=dtype)
    ref.flat.copy_(want)
    assert not torch.equal(plain.owned(), ref.owned())


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mask", [0b010101, 0b101010], ids=["low", "high"])
def test_one_face_per_axis(h3d, gpu, mask, dtype, kernel, form):
    """Only the low, or only the high, face of each axis walled."""
    _need(h3d, dtype, kernel, True, form)
    ops = h3d.ops
    n = (9, 13, 130)
    T, C, S, A = _field(ops, n, dtype, 21), _cond(ops, n, dtype, 22), _source(ops, n, dtype, 23), _cap(ops, n, dtype, 24)
    box, u = [0, n[0], 0, n[1], 0, n[2]], (0, -1, 0, -1, 0, -1)
    walls = ops.wall_coords(mask, n)
    conv, ambient = FORMS[form](mask)

    def call(src, dst, st, q, c, a):
        ops.sweep3(src, dst, D, box, u, kernel=kernel, state=st, source=q, conductivity=c, cap=a, walls=walls,
                   conv=conv, ambient=ambient)

    want, got, rc, rg = _both(ops, gpu, call, T, C, S, A)
    assert vf.same_bits(got, want)
    assert rc == rg, (rc, rg)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_walls_inside_deep_halos(h3d, gpu, dtype, kernel, form):
    """Deep ghosts and update ranges on every axis; the x- wall-adjacent plane
    (-1) and the y+ / z+ wall-adjacent row and column (n) are computed inside
    the halos, where s is read too."""
    _need(h3d, dtype, kernel, True, form)
    ops = h3d.ops
    K = int(kernel[2])
    n, box = (12, 50, 140), (0, 12, 0, 50, 0, 140)
    mask = 0b101001  # x-, y+, z+
    walls = ops.wall_coords(mask, n, gstart=(2, 1, 1), N=(n[0] + 100, n[1] + 3, n[2] + 3))
    none = h3d.native().NO_WALL
    assert walls == [-1, none, none, n[1], none, n[2]]
    u = [max(-(K - 1), -1), n[0] + K - 1, -(K - 1), min(n[1] + K - 1, n[1] + 1), -(K - 1), min(n[2] + K - 1, n[2] + 1)]
    g = (K, K, K)
    T, C, S, A = _field(ops, n, dtype, 11, g), _cond(ops, n, dtype, 12, g), _source(ops, n, dtype, 13, g), _cap(ops, n, dtype, 14, g)
    conv, ambient = FORMS[form](mask)

    def call(src, dst, st, q, c, a):
        ops.sweep3(src, dst, D, box, u, kernel=kernel, state=st, source=q, conductivity=c, cap=a, walls=walls,
                   conv=conv, ambient=ambient)

    want, got, rc, rg = _both(ops, gpu, call, T, C, S, A)
    assert vf.same_bits(got, want)
    assert rc == rg, (rc, rg)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n0,box_x,side", [(4, (0, 4), "both"), (9, (0, 9), "hi"), (12, (4, 8), "both")])
def test_x_slab_deep_halo_with_yz_walls(h3d, gpu, kernel, dtype, form, n0, box_x, side):
    _need(h3d, dtype, kernel, True, form)
    ops = h3d.ops
    K = int(kernel[2])
    n = (n0, 37, 133)
    u = (-(K - 1) if side in ("lo", "both") else 0, n0 + (K - 1 if side in ("hi", "both") else 0), 0, -1, 0, -1)
    box = (box_x[0], box_x[1], 0, n[1], 0, n[2])
    g = (K, 1, 1)
    mask = 0b111100
    walls = ops.wall_coords(mask, n)
    conv, ambient = FORMS[form](mask)
    T, C, S, A = _field(ops, n, dtype, 7, g), _cond(ops, n, dtype, 8, g), _source(ops, n, dtype, 9, g), _cap(ops, n, dtype, 10, g)

    def call(src, dst, st, q, c, a):
        ops.sweep3(src, dst, D, box, u, kernel=kernel, state=st, source=q, conductivity=c, cap=a, walls=walls,
                   conv=conv, ambient=ambient)

    want, got, rc, rg = _both(ops, gpu, call, T, C, S, A)
    assert vf.same_bits(got, want)
    assert rc == rg, (rc, rg)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_wall_sub_box_writes_nothing_outside(h3d, gpu, kernel, dtype, form):
    """A sub-box that touches the x-, y+ and z+ walls."""
    _need(h3d, dtype, kernel, False, form)
    ops = h3d.ops
    n, box = (12, 14, 200), [0, 7, 2, 14, 5, 200]
    T, C, A = _field(ops, n, dtype, 4), _cond(ops, n, dtype, 5), _cap(ops, n, dtype, 6)
    walls = ops.wall_coords(63, n)
    conv, ambient = FORMS[form](63)

    def call(src, dst, st, q, c, a):
        ops.sweep3(src, dst, D, box, (0, -1, 0, -1, 0, -1), kernel=kernel, state=st, conductivity=c, cap=a, walls=walls,
                   conv=conv, ambient=ambient)

    want, got, rc, rg = _both(ops, gpu, call, T, C, None, A, fill=-7.0)
    assert torch.equal(got, want) and rc == rg
    x0, x1, y0, y1, z0, z1 = box
    ref = ops.PaddedField(n, dtype=dtype)
    ref.flat.copy_(got)
    assert (ref.owned()[x0:x1, y0:y1, z0:z1] != -7.0).all()
    ref.owned()[x0:x1, y0:y1, z0:z1] = -7.0
    assert (ref.flat == -7.0).all()


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kernel", KERNELS)
def test_wall_done_flag_writes_nothing(h3d, gpu, kernel, form):
    _need(h3d, torch.float64, kernel, False, form)
    ops, ext = h3d.ops, h3d.native()
    n, dtype = (9, 13, 130), torch.float64
    T, C, A = (_to(ops, f, gpu) for f in (_field(ops, n, dtype, 1), _cond(ops, n, dtype, 2), _cap(ops, n, dtype, 6)))
    out = ops.PaddedField(n, dtype=dtype, device=gpu)
    out.flat.fill_(-7.0)
    st = ops.new_state(gpu)
    st.view(torch.int32)[ext.STATE_DONE_OFFSET // 4] = 1
    before = st.clone()
    conv, ambient = FORMS[form](63)
    ops.sweep3(T, out, D, [0, n[0], 0, n[1], 0, n[2]], (0, -1, 0, -1, 0, -1), kernel=kernel, state=st, conductivity=C,
               cap=A, walls=ops.wall_coords(63, n), conv=conv, ambient=ambient)
    torch.cuda.synchronize()
    assert (out.flat == -7.0).all() and torch.equal(st, before)


# ---- the solver (N_SOLVER, WALLS and the inputs of tests/test_gpu_capacity.py)

N_SOLVER = (33, 33, 33)
WALLS = dict(insulated="x-,z+", convective={"y-": 0.5}, ambient=0.25)
STEPS = 40  # thirteen sweeps of three steps and a single step


def _inputs():
    rng = np.random.default_rng(5)
    return (rng.uniform(0.0, 1.0, N_SOLVER), rng.uniform(1.0, 9.0, N_SOLVER), rng.uniform(0.05, 1.0, N_SOLVER),
            rng.uniform(-50.0, 50.0, N_SOLVER))


def _solver(h3d, backend, dt, walls, flag, vr=1, dec=None, eps=0.0, graph=True):
    s = h3d.HeatSolver(N_SOLVER, 100000, eps, dtype=dt, backend=backend, virtual_ranks=vr, decomp=dec, graph=graph,
                       capacity_sweeps=flag, **(WALLS if walls else {}))
    T0, rc, c, q = _inputs()
    s.set_field(T0)
    s.set_conductivity(c)
    s.set_source(q)
    s.set_capacity(rc)
    assert s.native.has_capacity and s.native.sweeps_active == flag
    assert ("tc" in s.kernel) == flag, s.kernel
    return s


def _steps(s):
    s.step(STEPS)
    s.synchronize()
    return s.state()["iter"], s.native.residual_history(), s.gather()


def _upto(s, conv_iter):
    """{iteration: residual} of the kept history up to the convergence iteration
    (what follows are the checks of iterations issued after convergence)."""
    hist = s.native.residual_history()
    first = s.state()["iter"] - len(hist)
    return {first + i: r for i, r in enumerate(hist) if first + i <= conv_iter}


@pytest.fixture(scope="module")
def cpu_flag_off(h3d):
    """CPU backend, flag off (single steps), per dtype and wall set."""
    return {(dt, w): _steps(_solver(h3d, "cpu", dt, w, False)) for dt in ("fp64", "fp32") for w in (False, True)}


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("walls", [False, True], ids=["dirichlet", "walls"])
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
@pytest.mark.parametrize("vr,dec", [(1, None), (8, (2, 2, 2))], ids=["one", "2x2x2"])
def test_solver_gpu_flag_on_equals_cpu_flag_off(h3d, gpu, cpu_flag_off, dt, walls, vr, dec, graph):
    s = _solver(h3d, "hip", dt, walls, True, vr, dec, graph=graph)
    assert s.native.temporal_blocking and s.kernel.startswith("tc"), s.kernel
    it, hist, field = _steps(s)
    assert s.native.sweeps_active and "tc" in s.kernel
    want = cpu_flag_off[dt, walls]
    assert it == want[0] == STEPS
    assert hist == want[1]
    assert np.array_equal(field, want[2])
    if graph and vr == 1:
        assert s.native.graph_launches > 0


@pytest.mark.parametrize("walls", [False, True], ids=["dirichlet", "walls"])
def test_solver_convergence_equals_cpu(h3d, gpu, walls):
    """eps 1e-3: the same conv_iter, the same history up to it and the same field
    (the rollback inside a sweep), one domain and 2x2x2."""
    runs = []
    for backend, flag, vr, dec in (("cpu", False, 1, None), ("hip", True, 1, None), ("hip", True, 8, (2, 2, 2))):
        s = _solver(h3d, backend, "fp64", walls, flag, vr, dec, eps=1e-3)
        r = s.run()
        assert r["converged"] and s.native.sweeps_active == flag
        runs.append((r["conv_iter"], _upto(s, r["conv_iter"]), s.gather()))
    a, b, c = runs
    assert a[0] == b[0] == c[0] > 10
    both = sorted(a[1].keys() & b[1].keys() & c[1].keys())
    print(f"conv_iter {a[0]}, {len(both)} iterations compared")
    assert len(both) >= 64 and both[-1] == a[0]
    assert [a[1][t] for t in both] == [b[1][t] for t in both] == [c[1][t] for t in both]
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[2], c[2])


@pytest.mark.parametrize("walls", [False, True], ids=["dirichlet", "walls"])
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
def test_heat_balance_after_the_run(h3d, gpu, dt, walls):
    """heat_balance() after a flag-on run returns the flag-off values (the same
    field, the same fixed reduction)."""
    out = []
    for flag in (False, True):
        s = _solver(h3d, "hip", dt, walls, flag)
        _steps(s)
        out.append(s.heat_balance())
    assert out[0]["capacity"] is True
    assert out[0] == out[1]


def test_clear_returns_to_the_earlier_schedule(h3d, gpu):
    """clear_capacity() puts a flag-on run back on single steps with the
    conductivity, clear_conductivity() then on the lean sweeps."""
    s = _solver(h3d, "hip", "fp64", False, True)
    _steps(s)
    s.clear_capacity()
    assert not s.native.has_capacity and not s.native.sweeps_active and "tc" not in s.kernel, s.kernel
    s.set_field(_inputs()[0])
    got = _steps(s)
    t = h3d.HeatSolver(N_SOLVER, 100000, 0.0, backend="hip")
    T0, _, c, q = _inputs()
    t.set_field(T0)
    t.set_conductivity(c)
    t.set_source(q)
    want = _steps(t)
    assert got[1] == want[1] and np.array_equal(got[2], want[2])
    s.clear_conductivity()
    assert s.native.sweeps_active and "tl" in s.kernel


def test_a_nan_is_a_fault_not_convergence(h3d, gpu):
    s = _solver(h3d, "hip", "fp64", False, True, eps=1e-12)
    s.step(12)
    s.synchronize()
    s.native.inject(0, 16, 16, 16, float("nan"))
    r = s.run()
    assert r["fault"] and not r["converged"], r
