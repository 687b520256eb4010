"""Convective (Robin) walls, CPU side: parsing and usage errors, checkpoints,
sweeps against single steps and the PyTorch oracle in both builds of the row
kernels, beta = 0 against the insulated run, the exact steady state of the slab
problem, the heat balance of the fully convective cube and decomposition
invariance of the solver."""
import json
import math

import numpy as np
import pytest
import torch

from conftest import run_cli

D = (0.06, 0.05, 0.04)
FACES = ("x-", "x+", "y-", "y+", "z-", "z+")
USAGE = "bin/HeatEquation3D NUM_CELLS_X NUM_CELLS_Y NUM_CELLS_Z ITER_MAX EPS"
TORCH = {"fp64": torch.float64, "fp32": torch.float32}
# a coefficient per face, all different; -1: that face is insulated (where it has a wall)
CONV = [0.5, -1.0, 1.0, 0.3, -1.0, 0.9]
AMBIENT = 1.75


# ---- 1. parsing, usage errors, checkpoints

def test_parsing_and_usage_errors(h3d, heat3d_bin, tmp_path):
    ext = h3d.native()
    assert "--convective" in ext.usage() and "--ambient" in ext.usage()
    assert list(ext.parse_convective("y-=0.5,x+=0.25")) == [-1, 0.25, 0.5, -1, -1, -1]
    assert list(ext.parse_convective("all=0.5")) == [0.5] * 6
    assert list(ext.parse_convective("all=0.5,z+=1")) == [0.5] * 5 + [1.0]
    assert ext.convective_str(ext.parse_convective("y-=0.5,x+=0.25")) == "x+=0.25,y-=0.5"
    assert ext.convective_str([-1.0] * 6) == "none"
    third = ext.convective_str(ext.parse_convective(f"z-={1 / 3!r}"))
    assert list(ext.parse_convective(third))[4] == 1 / 3  # the canonical string round-trips the value
    for bad in ("w-=0.5", "x-", "x-=", "x-=0.5,", "x-=1.5", "x-=-0.1", "x-=nan", "x-=inf", "x-=0.5x", ""):
        with pytest.raises(RuntimeError, match="--convective"):
            ext.parse_convective(bad)
    cfg = ext.config_parse(["9", "9", "9", "10", "1e-4", "--convective", "y-=0.5", "--ambient", "0.25"])
    assert cfg["convective"] == "y-=0.5" and cfg["ambient"] == 0.25
    assert "convective walls:         y-=0.5\nambient temperature:      0.25\n" in cfg["banner"]
    assert "convective" not in ext.config_parse(["9", "9", "9", "10", "1e-4"])["banner"]
    # Python: unknown face, coefficient out of range, insulated and convective, non-finite ambient
    mk = lambda **kw: h3d.HeatSolver((9, 9, 9), 10, 0.0, backend="cpu", **kw)  # noqa: E731
    with pytest.raises(RuntimeError, match="--convective"):
        mk(convective={"top": 0.5})
    with pytest.raises(RuntimeError, match=r"outside \[0, 1\]"):
        mk(convective={"y-": 1.25})
    with pytest.raises(RuntimeError, match="either insulated or convective"):
        mk(convective={"y-": 0.5, "x-": 0.5}, insulated="x-,x+")
    with pytest.raises(RuntimeError, match="--ambient"):
        mk(convective={"y-": 0.5}, ambient=float("inf"))
    base = ["9", "9", "9", "10", "1e-4", "--backend", "cpu"]
    for args, word in ((["--convective", "q+=0.5"], "--convective"), (["--convective", "x-=2"], "[0, 1]"),
                       (["--convective", "x-=0.5", "--insulated", "x-"], "either insulated or convective"),
                       (["--convective", "x-=0.5", "--ambient", "nan"], "--ambient"),
                       (["--convective", "x-=0.5", "--compat"], "--compat"),
                       (["--convective", "x-=0.5", "--scheme", "reference"], "--scheme reference")):
        r = run_cli(base + args, tmp_path)
        assert r.returncode != 0 and USAGE in r.stdout and word in r.stderr, (args, r.stderr)


def _solver(h3d, N, insulated=None, convective=None, ambient=0.0, vr=1, dec=None, temporal=3, dtype="fp64",
            iters=1000, eps=0.0, extra=()):
    return h3d.HeatSolver(N, iters, eps, dtype=dtype, backend="cpu", virtual_ranks=vr, decomp=dec, insulated=insulated,
                          convective=convective, ambient=ambient, extra_args=["--temporal", str(temporal), *extra])


def test_cli_report_and_checkpoints(h3d, heat3d_bin, tmp_path):
    N, faces = (15, 13, 17), {"y-": 0.5, "x+": 1 / 3}
    r = run_cli(["15", "13", "17", "40", "0", "--backend", "cpu", "--temporal", "3", "--insulated", "z-,z+",
                 "--convective", f"y-=0.5,x+={1 / 3!r}", "--ambient", "0.1", "--output", "none", "--json-out", "run.json",
                 "--checkpoint-dir", "ck", "--checkpoint-every", "40"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "convective walls:" in r.stdout and "ambient temperature:      0.1" in r.stdout
    j = json.loads((tmp_path / "run.json").read_text())
    want = h3d.native().convective_str(h3d.native().parse_convective(f"y-=0.5,x+={1 / 3!r}"))
    assert j["convective"] == want and j["ambient"] == 0.1 and j["insulated"] == "z-,z+"
    meta = json.loads((tmp_path / "ck" / "meta.json").read_text())
    assert meta["convective"] == want and float(meta["ambient"]) == 0.1 and meta["insulated"] == "z-,z+"
    s = _solver(h3d, N, "z-,z+", faces, 0.1, iters=40)
    s.step(40)
    s.synchronize()
    raw = np.fromfile(tmp_path / "ck" / meta["field"]).reshape(N)
    assert np.array_equal(raw, s.gather())
    # restart under the same values; other coefficients, faces or ambient are errors
    t = _solver(h3d, N, "z-,z+", faces, 0.1)
    t.initialize()
    t.load_checkpoint(str(tmp_path / "ck"))
    assert np.array_equal(t.gather(), raw) and t.state()["iter"] == 40
    for ins, conv, amb, word in (("z-,z+", {"y-": 0.5, "x+": 0.25}, 0.1, "convective"),
                                 ("z-,z+", {"y-": 0.5}, 0.1, "convective"), ("z-,z+", None, 0.0, "convective"),
                                 ("z-,z+", faces, 0.2, "ambient"), ("z-", faces, 0.1, "insulated")):
        u = _solver(h3d, N, ins, conv, amb)
        u.initialize()
        with pytest.raises(RuntimeError, match=word):
            u.load_checkpoint(str(tmp_path / "ck"))
    # a checkpoint without the keys loads as before: no convective face
    for k in ("convective", "ambient"):
        del meta[k]
    (tmp_path / "ck" / "meta.json").write_text(json.dumps(meta))
    u = _solver(h3d, N, "z-,z+")
    u.initialize()
    u.load_checkpoint(str(tmp_path / "ck"))
    with pytest.raises(RuntimeError, match="convective"):
        t.load_checkpoint(str(tmp_path / "ck"))


def test_model_helpers(h3d):
    m = h3d.HeatEquation3D((9, 17, 9))
    hy = m.h[1]
    assert m.wall_coefficient(0.0, 1) == 0.0
    assert m.wall_coefficient(2.0 / hy, 1) == pytest.approx(1.0) and m.wall_coefficient(4.0, 1, k=2.0) == \
        pytest.approx(2 * (2 * hy) / (2 + 2 * hy))
    with pytest.raises(ValueError, match="beta"):
        m.wall_coefficient(2.5 / hy, 1)
    T = m.convective_slab_steady(0.5, 0.25)
    s = (1 - 0.25) / (1 / 0.5 + 17 - 2)
    assert T.shape == (9, 17, 9) and np.all(T[:, -1] == 1.0)
    assert np.allclose(T[3, 1:-1, 4], 0.25 + s * (1 / 0.5 + np.arange(1, 16) - 1), rtol=0, atol=1e-15)
    assert np.allclose(T[:, 0], T[:, 1] + 0.5 * (0.25 - T[:, 1]), rtol=0, atol=1e-15)


# ---- 2. kernels: sweep == single steps == oracle, both builds of the rows

def _ghost(c, beta, dtype):
    from heat3d_amd.utils.fma import fma

    return fma(beta, torch.tensor(AMBIENT, dtype=dtype) - c, c)


def _single_step_deep(ops, a, b, box, walls, conv, st):
    """One step of `box` (deep-ghost coordinates allowed): the torch oracle on the
    box's block with the neighbour across a wall replaced by the ghost of that
    face (the centre value on an insulated one), written into b."""
    from heat3d_amd.utils.fma import ftcs_update

    g = (a.gx, a.gy, a.gz)
    F = a.deep3()
    lo = [box[2 * ax] + g[ax] for ax in range(3)]
    hi = [box[2 * ax + 1] + g[ax] for ax in range(3)]

    def sl(shift):
        return F[tuple(slice(lo[ax] + shift[ax], hi[ax] + shift[ax]) for ax in range(3))]

    c = sl((0, 0, 0))
    nb = []
    for ax in range(3):
        for e, sh in ((0, -1), (1, 1)):
            shift = [0, 0, 0]
            shift[ax] = sh
            v = sl(shift).clone()
            w = walls[2 * ax + e]
            if box[2 * ax] <= w < box[2 * ax + 1]:
                idx = [slice(None)] * 3
                idx[ax] = w - box[2 * ax]
                beta = conv[2 * ax + e]
                v[tuple(idx)] = _ghost(c[tuple(idx)], beta, c.dtype) if beta >= 0 else c[tuple(idx)]
            nb.append(v)
    new = ftcs_update(c, *nb, D)
    b.deep3()[tuple(slice(lo[ax], hi[ax]) for ax in range(3))] = new
    st.view(torch.float64)[0] = (new - c).abs().max().double().item()


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("K", [2, 3])
def test_sweep_equals_single_steps(h3d, dtype, K):
    """cpu::stencil_multi with convective and insulated faces mixed (a coefficient
    per face) against K single steps of the oracle on the same boxes: the low
    walls inside the deep ghosts, the high walls on the box's last planes."""
    ops = h3d.ops
    n = (7, 6, 9)
    none = h3d.native().NO_WALL
    gen = torch.Generator().manual_seed(11)
    src = ops.PaddedField(n, dtype=TORCH[dtype], gx=K, gy=K, gz=K)
    src.deep3().copy_(torch.rand(src.deep3().shape, generator=gen, dtype=torch.float64).to(TORCH[dtype]))
    box = (0, n[0], 0, n[1], 0, n[2])
    for walls, u in (
        ([-(K - 1), n[0] - 1, -(K - 1), n[1] - 1, -(K - 1), n[2] - 1], (-(K - 1), n[0], -(K - 1), n[1], -(K - 1), n[2])),
        ([0, none, none, n[1] - 1, 0, none], (0, n[0] + K - 1, -(K - 1), n[1], 0, n[2])),
    ):
        got = ops.PaddedField(n, dtype=TORCH[dtype], gx=K, gy=K, gz=K)
        st = ops.new_state("cpu")
        ops.sweep3(src, got, D, box, u, kernel=f"tl{K}", state=st, walls=walls, conv=CONV, ambient=AMBIENT)
        ins = ops.PaddedField(n, dtype=TORCH[dtype], gx=K, gy=K, gz=K)
        ops.sweep3(src, ins, D, box, u, kernel=f"tl{K}", walls=walls)
        assert not torch.equal(ins.owned(), got.owned())
        a = ops.PaddedField(n, dtype=TORCH[dtype], gx=K, gy=K, gz=K)
        a.flat.copy_(src.flat)
        b = ops.PaddedField(n, dtype=TORCH[dtype], gx=K, gy=K, gz=K)
        b.flat.copy_(src.flat)
        for s in range(K):
            w = K - 1 - s
            bx = []
            for ax in range(3):
                bx += [max(box[2 * ax] - w, u[2 * ax]), min(box[2 * ax + 1] + w, u[2 * ax + 1])]
            st1 = ops.new_state("cpu")
            _single_step_deep(ops, a, b, bx, walls, CONV, st1)
            assert ops.residual_from_state(st1) == ops.residual_from_state(st, s), (walls, s)
            a.flat.copy_(b.flat)
        x0, x1, y0, y1, z0, z1 = box
        assert torch.equal(got.owned()[x0:x1, y0:y1, z0:z1], a.owned()[x0:x1, y0:y1, z0:z1]), walls


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_step_matches_oracle_on_refreshed_planes(h3d, dtype):
    """cpu::stencil with convective and insulated faces against
    ftcs_reference(convective=, insulated=): 5 steps, field and residual."""
    ops = h3d.ops
    n = (7, 6, 5)
    walls = ops.wall_coords(63, n)
    gen = torch.Generator().manual_seed(3)
    a = ops.PaddedField(n, dtype=TORCH[dtype])
    a.ghosted().copy_(torch.rand(tuple(e + 2 for e in n), generator=gen, dtype=torch.float64).to(TORCH[dtype]))
    b = ops.PaddedField(n, dtype=TORCH[dtype])
    b.flat.copy_(a.flat)
    T = a.ghosted().clone()
    conv = {f: v for f, v in zip(FACES, CONV) if v >= 0}
    ins = [f for f, v in zip(FACES, CONV) if v < 0]
    for _ in range(5):
        st = ops.new_state("cpu")
        ops.ftcs_step(a, b, D, state=st, walls=walls, conv=CONV, ambient=AMBIENT)
        new, res = ops.ftcs_reference(T, D, insulated=ins, convective=conv, ambient=AMBIENT)
        T[1:-1, 1:-1, 1:-1] = new
        assert torch.equal(b.owned(), new)
        assert ops.residual_from_state(st) == res
        a, b = b, a


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_both_row_builds(h3d, dtype):
    """The row kernel of the generic build (libm fma) and of the FMA build on a
    row with every face a wall: the same bits, and the oracle's."""
    from heat3d_amd.utils.fma import ftcs_update

    cpu = h3d.native().cpu
    td, nk = TORCH[dtype], 11
    gen = torch.Generator().manual_seed(5)
    blk = torch.rand((3, 3, nk + 2), generator=gen, dtype=torch.float64).to(td).contiguous()
    sx, sy = blk.stride(0), blk.stride(1)
    esize = blk.element_size()
    base = blk.data_ptr() + (sx + sy + 1) * esize
    beta = [0.5, 0.3, 1.0, 0.125, 0.7, 0.9]
    Dr = [float(torch.tensor(d, dtype=td)) for d in D]
    c = blk[1, 1, 1:-1]
    gh = [_ghost(c, b, td) for b in beta]
    zm, zp = blk[1, 1, :-2].clone(), blk[1, 1, 2:].clone()
    zm[0], zp[-1] = gh[4][0], gh[5][-1]
    for off, nbr in (([0, 0, 0, 0], gh[:4]),
                     ([-sx, sx, -sy, sy], [blk[0, 1, 1:-1], blk[2, 1, 1:-1], blk[1, 0, 1:-1], blk[1, 2, 1:-1]])):
        want = ftcs_update(c, *nbr, zm, zp, Dr)
        outs = []
        builds = ["generic"] + (["fma"] if cpu.has_fma() else [])
        for build in builds:
            out = torch.zeros(nk, dtype=td)
            res = cpu.conv_row(build, dtype, base, out.data_ptr(), nk, off, [0, nk - 1], beta, AMBIENT, list(D))
            assert torch.equal(out, want), (build, off)
            assert res == (want - c).abs().max().double().item()
            outs.append(out)
    assert cpu.has_fma()  # the machines that run this suite have FMA + AVX2: both builds were compared


# ---- 3. beta = 0 is the insulated run

@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("temporal", [1, 3])
def test_beta_zero_is_the_insulated_run(h3d, dtype, temporal):
    N, faces = (17, 13, 15), "x-,y+,z-,z+"
    T0 = np.random.default_rng(2).uniform(0.1, 1.0, N)
    out = []
    for ins, conv, amb in ((faces, None, 0.0), (None, {f: 0.0 for f in faces.split(",")}, 3.5),
                           ("x-,z+", {"y+": 0.0, "z-": 0.0}, -2.0)):
        s = _solver(h3d, N, ins, conv, amb, temporal=temporal, dtype=dtype)
        s.set_field(T0)
        assert s.native.sweeps_active == (temporal == 3)
        s.step(14)
        s.synchronize()
        out.append((s.gather(), s.native.residual_history()))
    for T, h in out[1:]:
        assert np.array_equal(T, out[0][0]) and h == out[0][1]


# ---- 4. the slab problem

SLAB = (9, 15, 9)  # (h_y = 1/14 is not a binary fraction: T = y is not an exact fixed point of the Dirichlet run)


def _slab(h3d, eps, iters=400000, temporal=3):
    return _solver(h3d, SLAB, "x-,x+,z-,z+", {"y-": 0.5}, 0.25, temporal=temporal, iters=iters, eps=eps)


def test_slab_steady_state_is_a_fixed_point(h3d):
    """Started from convective_slab_steady the first step's residual is rounding
    only: no larger than 4x (the ghost's extra FMA) the first-step residual of
    the plain Dirichlet solver started from its steady state T = y."""
    s = _slab(h3d, 0.0, temporal=1)
    s.set_field(s.model.convective_slab_steady(0.5, 0.25))
    s.step(1)
    s.synchronize()
    got = s.native.residual_history()[-1]
    p = h3d.HeatSolver(SLAB, 10, 0.0, backend="cpu", extra_args=["--temporal", "1"])
    p.set_field(p.model.steady_state())
    p.step(1)
    p.synchronize()
    ref = p.native.residual_history()[-1]
    print(f"slab first-step residual {got:.3e}, Dirichlet T = y first-step residual {ref:.3e}")
    assert ref > 0.0
    assert got <= 4 * ref


def test_slab_converges_to_the_steady_state(h3d):
    """From a zero interior the error against convective_slab_steady shrinks by
    at least 10x from eps 1e-6 to 1e-8 (theory: 100x, the error is proportional
    to the residual once the slowest mode dominates)."""
    err = {}
    for eps in (1e-6, 1e-8):
        s = _slab(h3d, eps)
        r = s.run()
        assert r["converged"]
        err[eps] = np.abs(s.gather() - s.model.convective_slab_steady(0.5, 0.25))[1:-1, 1:-1, 1:-1].max()
    print(f"slab error {err}")
    assert err[1e-8] * 10 <= err[1e-6]


# ---- 5. heat balance

def test_heat_balance_of_the_convective_cube(h3d):
    """All six faces convective: sum T^{n+1} - sum T^n over the interior equals
    sum_f D_a beta_f sum_{wall-adjacent} (T_inf - T^n), up to the rounding bound
    of the insulated cube's balance test, 10 n M_points 2^-53."""
    N, n = (18, 14, 22), 30
    beta = dict(zip(FACES, (0.5, 0.3, 1.0, 0.125, 0.7, 0.9)))
    amb = 0.4
    T0 = np.random.default_rng(9).uniform(0.0, 1.0, N)
    points = (N[0] - 2) * (N[1] - 2) * (N[2] - 2)
    bound = 10 * n * points * 2.0 ** -53
    s = _solver(h3d, N, None, beta, amb, temporal=1)
    s.set_field(T0)
    Dm = s.model.D
    T, want = s.gather(), 0.0
    start = math.fsum(T[1:-1, 1:-1, 1:-1].ravel())
    for _ in range(n):
        I = T[1:-1, 1:-1, 1:-1]
        for f, name in enumerate(FACES):
            a, e = divmod(f, 2)
            want += Dm[a] * beta[name] * math.fsum((amb - np.take(I, -1 if e else 0, axis=a)).ravel())
        s.step(1)
        s.synchronize()
        T = s.gather()
    got = math.fsum(T[1:-1, 1:-1, 1:-1].ravel()) - start
    print(f"heat balance: moved {got:.6e}, through the walls {want:.6e}, bound {bound:.3e}")
    assert abs(want) > 1e3 * bound  # (the bound discriminates)
    assert abs(got - want) <= bound
    # the sweep schedule moves the same heat: the same field
    t = _solver(h3d, N, None, beta, amb, temporal=3)
    t.set_field(T0)
    t.step(n)
    t.synchronize()
    assert np.array_equal(t.gather(), T)


# ---- 6. decomposition invariance, host view

MIXED = dict(insulated="x-,z+", convective={"x+": 0.25, "y-": 0.5, "z-": 1.0}, ambient=0.375)


@pytest.fixture(scope="module")
def one_rank(h3d):
    s = _solver(h3d, (17, 17, 17), temporal=1, **MIXED)
    s.set_field(np.random.default_rng(2).uniform(0.0, 1.0, (17, 17, 17)))
    assert not s.native.sweeps_active
    s.step(14)
    s.synchronize()
    return s.gather(), s.native.residual_history()


@pytest.mark.parametrize("vr,dec", [(1, None), (8, (2, 2, 2)), (4, (4, 1, 1))])
@pytest.mark.parametrize("temporal", [1, 3])
def test_decomposition_invariance(h3d, one_rank, vr, dec, temporal):
    s = _solver(h3d, (17, 17, 17), vr=vr, dec=dec, temporal=temporal, **MIXED)
    s.set_field(np.random.default_rng(2).uniform(0.0, 1.0, (17, 17, 17)))
    assert s.native.sweeps_active == (temporal == 3)
    s.step(14)
    s.synchronize()
    assert s.state()["iter"] == 14
    assert s.native.residual_history() == one_rank[1]
    assert np.array_equal(s.gather(), one_rank[0])


def test_wall_vertices_show_the_ghost(h3d):
    """What the host sees on a convective wall: g of the inward neighbour;
    set_field ignores values given there; Dirichlet vertices keep theirs."""
    N = (9, 8, 7)
    s = _solver(h3d, N, "x-", {"y-": 0.5}, 0.25, temporal=1)
    T0 = np.random.default_rng(4).uniform(0.0, 1.0, N)
    s.set_field(T0)
    want = T0.copy()
    want[0, :-1, 1:-1] = want[1, :-1, 1:-1]   # x- (insulated; y+ and the z faces are Dirichlet: kept)
    c = want[:-1, 1, 1:-1]
    want[:-1, 0, 1:-1] = np.array(_ghost_np(c, 0.5, 0.25))
    assert np.array_equal(s.gather(), want)
    s.step(3)
    s.synchronize()
    T = s.gather()
    assert np.array_equal(T[1:-1, 0, 1:-1], _ghost_np(T[1:-1, 1, 1:-1], 0.5, 0.25))
    assert np.array_equal(T[-1], T0[-1]) and np.array_equal(T[:, :, 0], want[:, :, 0])


def _ghost_np(c, beta, amb):
    from heat3d_amd.utils.fma import fma

    t = torch.from_numpy(np.ascontiguousarray(c))
    return fma(beta, torch.tensor(amb, dtype=t.dtype) - t, t).numpy()


def test_conv_forms_listed(h3d):
    """The convective forms: the default shapes at depth 2, 3 and 4; a sweep with
    a convective face and no such form is an error, never other arithmetic."""
    ext, ops = h3d.native(), h3d.ops
    for dt in ("fp64", "fp32"):
        for spec in ("tl2", "tl3", "tl4"):
            assert ext.lean_conv_supported(dt, spec), (dt, spec)
        for spec in ("tl3:2", "tl5", "tl3:1:2:1:16", "tv3"):
            assert not ext.lean_conv_supported(dt, spec), (dt, spec)
    n = (8, 40, 70)
    T, out = ops.PaddedField(n), ops.PaddedField(n)
    args = ("fp64", T.data_ptr(), out.data_ptr(), list(n), [1, 1, 1], [0, n[0], 0, n[1], 0, n[2]],
            [0, -1, 0, -1, 0, -1], list(D), 0, 0)
    with pytest.raises(RuntimeError, match="no convective-wall form"):
        ext.hip.stencil_sweep3(*args, "tl5", 0, 0, 0, ops.wall_coords(1, n), [0.5, -1, -1, -1, -1, -1], 0.0)
    with pytest.raises(RuntimeError, match="wall"):
        ext.hip.stencil_sweep3(*args, "tl3:2", 0, 0, 0, ops.wall_coords(63, n), [0.5] * 6, 0.0)
    assert torch.count_nonzero(out.flat) == 0
