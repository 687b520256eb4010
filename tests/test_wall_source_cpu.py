"""A heat source behind insulated or convective walls, CPU side: the row
kernels that take walls and a source together against the PyTorch oracle, the
opt-in K-step sweeps (--wall-source-sweeps) against the single-step schedule,
the heat balance of the insulated cube with a uniform source, the exact steady
state of the heated slab, and the interfaces (CLI, Python)."""
import json
import math

import numpy as np
import pytest
import torch

from conftest import run_cli

D = (0.06, 0.05, 0.04)
USAGE = "bin/HeatEquation3D NUM_CELLS_X NUM_CELLS_Y NUM_CELLS_Z ITER_MAX EPS"
TORCH = {"fp64": torch.float64, "fp32": torch.float32}
# the two face sets of the issue: insulated only, and insulated and convective mixed
INSULATED = dict(insulated="x-,y+,z-", convective=None, ambient=0.0)
MIXED = dict(insulated="x-,z+", convective={"y+": 0.5, "z-": 0.75}, ambient=0.375)
FACE_SETS = {"insulated": INSULATED, "mixed": MIXED}
N17 = (17, 17, 17)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("faces", sorted(FACE_SETS))
def test_step_matches_oracle(h3d, dtype, faces):
    """cpu::stencil with StencilParams::wall and src together against the torch
    oracle (wall planes refreshed by hand, the update, then the source), bitwise,
    field and residual, 3 steps on n = (13, 12, 11) with a source in [-5, 5]."""
    ops, fs, td = h3d.ops, FACE_SETS[faces], TORCH[dtype]
    n = (13, 12, 11)
    mask = ops.insulated_mask(fs["insulated"]) | ops.convective_mask(fs["convective"])
    walls = ops.wall_coords(mask, n)
    conv = ops.convective_faces(fs["convective"]) if fs["convective"] else None
    gen = torch.Generator().manual_seed(5)
    a = ops.PaddedField(n, dtype=td)
    a.ghosted().copy_(torch.rand(tuple(e + 2 for e in n), generator=gen, dtype=torch.float64).to(td))
    b = ops.PaddedField(n, dtype=td)
    b.flat.copy_(a.flat)
    S = ops.PaddedField(n, dtype=td)
    S.ghosted().copy_((10.0 * torch.rand(tuple(e + 2 for e in n), generator=gen, dtype=torch.float64) - 5.0).to(td))
    T = a.ghosted().clone()
    for _ in range(3):
        st = ops.new_state("cpu")
        ops.ftcs_step(a, b, D, state=st, source=S, walls=walls, conv=conv, ambient=fs["ambient"])
        new, res = ops.ftcs_reference(T, D, src=S.owned(), insulated=fs["insulated"], convective=fs["convective"],
                                      ambient=fs["ambient"])
        T[1:-1, 1:-1, 1:-1] = new
        assert torch.equal(b.owned(), new)
        assert ops.residual_from_state(st) == res
        a, b = b, a
    # both matter: without the source, and without the walls, the step differs
    nosrc, _ = ops.ftcs_reference(T, D, insulated=fs["insulated"], convective=fs["convective"], ambient=fs["ambient"])
    nowall, _ = ops.ftcs_reference(T, D, src=S.owned())
    full, _ = ops.ftcs_reference(T, D, src=S.owned(), insulated=fs["insulated"], convective=fs["convective"],
                                 ambient=fs["ambient"])
    assert not torch.equal(full, nosrc) and not torch.equal(full, nowall)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("faces", sorted(FACE_SETS))
def test_sweep_is_k_single_steps(h3d, dtype, faces):
    """cpu::stencil_multi with walls and a source: K = 3 single steps with both."""
    ops, fs, td = h3d.ops, FACE_SETS[faces], TORCH[dtype]
    n, K = (7, 6, 9), 3
    mask = ops.insulated_mask(fs["insulated"]) | ops.convective_mask(fs["convective"])
    walls = ops.wall_coords(mask, n)
    conv = ops.convective_faces(fs["convective"]) if fs["convective"] else None
    gen = torch.Generator().manual_seed(8)
    src = ops.PaddedField(n, dtype=td)
    src.ghosted().copy_(torch.rand(tuple(e + 2 for e in n), generator=gen, dtype=torch.float64).to(td))
    S = ops.PaddedField(n, dtype=td)
    S.ghosted().copy_((10.0 * torch.rand(tuple(e + 2 for e in n), generator=gen, dtype=torch.float64) - 5.0).to(td))
    got = ops.PaddedField(n, dtype=td)
    st = ops.new_state("cpu")
    ops.sweep3(src, got, D, (0, n[0], 0, n[1], 0, n[2]), (0, -1, 0, -1, 0, -1), kernel=f"tl{K}", state=st, source=S,
               walls=walls, conv=conv, ambient=fs["ambient"])
    a, b = ops.PaddedField(n, dtype=td), ops.PaddedField(n, dtype=td)
    a.flat.copy_(src.flat)
    b.flat.copy_(src.flat)
    for s in range(K):
        st1 = ops.new_state("cpu")
        ops.ftcs_step(a, b, D, state=st1, source=S, walls=walls, conv=conv, ambient=fs["ambient"])
        assert ops.residual_from_state(st1) == ops.residual_from_state(st, s)
        a, b = b, a
    assert torch.equal(got.owned(), a.owned())


def _solver(h3d, N, fs, flag, vr=1, dec=None, temporal=3, dtype="fp64", iters=1000, eps=0.0, extra=()):
    return h3d.HeatSolver(N, iters, eps, dtype=dtype, backend="cpu", virtual_ranks=vr, decomp=dec,
                          wall_source_sweeps=flag, extra_args=["--temporal", str(temporal), *extra], **fs)


def _inputs(N, seed=2):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, N), rng.uniform(-5.0, 5.0, N)


def _run(s, T0, q, steps):
    s.set_field(T0)
    if q is not None:
        s.set_source(q)
    s.step(steps)
    s.synchronize()
    return s.gather(), s.native.residual_history()


@pytest.fixture(scope="module")
def flag_off(h3d):
    """17^3, 14 steps at --temporal 3 with the flag off (single steps), per face set."""
    out = {}
    for name, fs in FACE_SETS.items():
        s = _solver(h3d, N17, fs, False)
        T0, q = _inputs(N17)
        out[name] = _run(s, T0, q, 14)
        assert not s.native.sweeps_active
    return out


@pytest.mark.parametrize("faces", sorted(FACE_SETS))
@pytest.mark.parametrize("vr,dec", [(1, None), (8, (2, 2, 2)), (4, (4, 1, 1))])
def test_sweeps_equal_single_steps(h3d, flag_off, faces, vr, dec):
    """The flag on: K = 3 sweeps of walls and source together on 1, 2x2x2 and
    4x1x1 virtual ranks, bitwise the flag-off run, field and residual history."""
    s = _solver(h3d, N17, FACE_SETS[faces], True, vr, dec)
    T0, q = _inputs(N17)
    s.set_field(T0)
    s.set_source(q)
    assert s.native.sweeps_active
    T, hist = _run(s, T0, None, 14)
    assert s.native.sweeps_active and s.state()["iter"] == 14
    want, whist = flag_off[faces]
    assert hist == whist
    assert np.array_equal(T, want)


@pytest.mark.parametrize("faces", sorted(FACE_SETS))
def test_flag_without_source_or_with_conductivity(h3d, faces):
    """Without a source the flag does nothing (the plain wall forms sweep either
    way); with a conductivity every iteration stays a single step."""
    fs = FACE_SETS[faces]
    T0, q = _inputs(N17)
    c = np.random.default_rng(4).uniform(0.1, 1.0, N17)
    for what in ("no source", "conductivity", "conductivity and source"):
        out = []
        for flag in (False, True):
            s = _solver(h3d, N17, fs, flag)
            s.set_field(T0)
            if "conductivity" in what:
                s.set_conductivity(c)
            if "and source" in what:
                s.set_source(q)
            s.step(7)
            s.synchronize()
            out.append((s.native.sweeps_active, s.gather(), s.native.residual_history()))
        assert out[0][0] == out[1][0] == (what == "no source"), what
        assert np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2], what


def test_clear_source_returns_to_the_wall_forms(h3d):
    """clear_source() after 7 steps, then 6 more: the run that starts from that
    field and never had a source."""
    T0, q = _inputs(N17)
    s = _solver(h3d, N17, MIXED, True)
    T7, _ = _run(s, T0, q, 7)
    s.clear_source()
    assert s.native.sweeps_active and not s.native.has_source
    s.step(6)
    s.synchronize()
    t = _solver(h3d, N17, MIXED, True)
    want, whist = _run(t, T7, None, 6)
    assert np.array_equal(s.gather(), want) and s.native.residual_history() == whist
    # and the source mattered
    u = _solver(h3d, N17, MIXED, True)
    assert not np.array_equal(_run(u, T0, None, 7)[0], T7)


def test_heat_balance(h3d):
    """All six faces insulated, a uniform source S = float64(dt q): every step
    adds S to every interior point and the walls pass nothing, so after n steps
    the interior sum is the initial one + n points S up to the roundings of the
    updates, at most 10 n points 2^-53 max|T|.  With one face left Dirichlet the
    sum misses that by orders of magnitude (the bound discriminates)."""
    N, n, q = (18, 14, 22), 30, 3.0
    rng = np.random.default_rng(9)
    T0 = rng.uniform(0.0, 1.0, N)
    points = (N[0] - 2) * (N[1] - 2) * (N[2] - 2)
    S = np.float64(h3d.native().physics(*N)["dt"] * q)
    miss = {}
    for faces in ("all", "x-,x+,y-,z-,z+"):
        s = _solver(h3d, N, dict(insulated=faces), True)
        s.set_field(T0)
        s.set_source(np.full(N, q))
        assert s.native.sweeps_active
        s.step(n)
        s.synchronize()
        T = s.gather()
        tmax = max(np.abs(T).max(), np.abs(T0).max())
        bound = 10 * n * points * 2.0 ** -53 * tmax
        want = math.fsum(T0[1:-1, 1:-1, 1:-1].ravel()) + n * points * float(S)
        miss[faces] = (abs(math.fsum(T[1:-1, 1:-1, 1:-1].ravel()) - want), bound)
    print(f"heat balance (miss, bound): {miss}")
    assert miss["all"][0] <= miss["all"][1]
    assert miss["x-,x+,y-,z-,z+"][0] > 1e3 * miss["x-,x+,y-,z-,z+"][1]


def test_heated_slab_steady_state(h3d):
    """convective_slab_source_steady is a fixed point of the sweeps: x, z
    insulated, y- convective, y+ at 1, a uniform source.  30 steps move no
    interior value by more than 10 n 2^-53 * max|T| * 4 with max|T| <= 2 (the
    bound of test_walls_cpu.test_eigenmode scaled by the field's range)."""
    N, n, q = (9, 33, 9), 30, 8.0
    fs = dict(insulated="x-,x+,z-,z+", convective={"y-": 0.5}, ambient=0.25)
    s = _solver(h3d, N, fs, True)
    T0 = s.model.convective_slab_source_steady(0.5, 0.25, q)
    assert 1.5 < np.abs(T0).max() <= 2.0  # the source matters (without it max|T| is 1), and the bound's range holds
    # the defining relations: the update of every interior vertex is 0
    sigma = s.model.dt * q / s.model.D[1]
    v = T0[4, :, 4]
    assert np.abs(v[2:] - 2 * v[1:-1] + v[:-2] + sigma)[1:-1].max() < 1e-14
    assert v[-1] == 1.0 and v[0] == v[1] + 0.5 * (0.25 - v[1])
    s.set_field(T0)
    s.set_source(np.full(N, q))
    assert s.native.sweeps_active
    s.step(n)
    s.synchronize()
    err = np.abs(s.gather() - T0)[1:-1, 1:-1, 1:-1].max()
    bound = 10 * n * 2.0 ** -53 * 2 * 4
    print(f"heated slab: moved {err:.3e} bound {bound:.3e}")
    assert err <= bound
    # not a fixed point without the source
    t = _solver(h3d, N, fs, True)
    t.set_field(T0)
    t.step(n)
    t.synchronize()
    assert np.abs(t.gather() - T0)[1:-1, 1:-1, 1:-1].max() > 1e3 * bound


def test_usage_cli_and_report(h3d, heat3d_bin, tmp_path):
    ext = h3d.native()
    assert "--wall-source-sweeps" in ext.usage()
    base = ["15", "13", "17", "20", "0", "--backend", "cpu"]
    r = run_cli(base + ["--wall-source-sweeps", "--compat"], tmp_path)
    assert r.returncode != 0 and USAGE in r.stdout and "--wall-source-sweeps" in r.stderr
    N = (15, 13, 17)
    T0, q = _inputs(N, seed=12)
    q.tofile(tmp_path / "q.bin")
    T0.tofile(tmp_path / "T0.bin")
    fields = {}
    for flag in (True, False):
        args = base + ["--temporal", "3", "--insulated", "x-,z+", "--convective", "y+=0.5,z-=0.75", "--ambient", "0.375",
                       "--source", "q.bin", "--initial", "T0.bin", "--output", "none", "--json-out", "run.json",
                       "--checkpoint-dir", f"ck{int(flag)}", "--checkpoint-every", "20"]
        r = run_cli(args + (["--wall-source-sweeps"] if flag else []), tmp_path)
        assert r.returncode == 0, r.stderr
        j = json.loads((tmp_path / "run.json").read_text())
        assert j["wall_source_sweeps"] is flag
        meta = json.loads((tmp_path / f"ck{int(flag)}" / "meta.json").read_text())
        fields[flag] = np.fromfile(tmp_path / f"ck{int(flag)}" / meta["field"]).reshape(N)
    s = _solver(h3d, N, MIXED, True, iters=20)
    want, _ = _run(s, T0, q, 20)
    assert s.native.sweeps_active
    assert np.array_equal(fields[True], want) and np.array_equal(fields[False], want)
