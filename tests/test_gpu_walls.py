"""Insulated walls on the GPU: every wall form of the lean sweep
(csrc/kernels/stencil_tbl_wall_variants.inc is the test matrix) against the
CPU's K-single-steps definition, bitwise; the solver with walls (sweeps ==
single steps == CPU backend, decomposition, schedule and graph invariance,
convergence with the rollback, source / conductivity on the single-step path)
and the eigenmodes of the insulated cube through the K = 3 sweeps."""
import os
import re

import numpy as np
import pytest
import torch

import _lean_variants as lv

pytestmark = pytest.mark.gpu

D = (0.06, 0.05, 0.04)
SENTINEL = -5.0
TORCH = {"fp64": torch.float64, "fp32": torch.float32}
_ENTRY = re.compile(r"^H3D_VW\(\s*(double|float)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,"
                    r"\s*(true|false)\s*\)\s*$", re.M)


def wall_variants():
    with open(os.path.join(lv.KERNELS, "stencil_tbl_wall_variants.inc")) as f:
        text = f.read()
    out = [lv.Variant("fp64" if m.group(1) == "double" else "fp32", *(int(m.group(i)) for i in range(2, 7)),
                      m.group(7) == "true", 0, False) for m in _ENTRY.finditer(text)]
    assert len(out) == ("\n" + text).count("\nH3D_VW") and out
    return out


VARIANTS = wall_variants()


def _vid(v):
    return f"{v.dtype}-{'sw-' if v.SW else ''}{v.R}x{v.WY}-K{v.K}-{v.NTS}"


def _boxes(v):
    """(n, mask): smaller than a tile with every wall in one wave; two tiles
    and a remainder along the tile's two axes with every face insulated; the
    same with the + faces only.  The y-marching forms are picked by the box's
    shape (a thin x slab, a long y extent): their tile rows lie along x."""
    TY, YS, zs, U = lv.geometry(v)
    if v.SW:
        ex = 4 if (v.R, v.WY) != (3, 3) else 5  # what dispatch_tbl_wall sends to this form
        small = (ex, 16 * ex, 9)
        big = (ex, 16 * ex + 2 * (v.K - 1) + U + 3, 2 * zs + 3)
    else:
        small = (7, 6, 9)
        big = (2 * (v.K - 1) + U + 3, 2 * YS + 3, 2 * zs + 3)
    return [(small, 63), (big, 63), (big, 0b101010)]


@pytest.mark.parametrize("v", VARIANTS, ids=_vid)
def test_wall_variant_bitwise(h3d, gpu, v):
    """One launch per box of every listed wall form against cpu::stencil_multi
    with the same walls: the stored box, the sentinel everywhere else, every
    residual slot the variant computes."""
    ops, dtype = h3d.ops, TORCH[v.dtype]
    zs = lv.geometry(v)[2]
    kernel = f"tl{v.K}" if v.SW else lv.spec(v, zs=zs)
    last_only = bool(v.NTS & lv.LAST_ONLY)
    for n, mask in _boxes(v):
        if v.SW:
            assert lv.thin_slab_form(v.K, n[0], n[1]) == (v.R, v.WY, v.K), (n, v)
        walls = ops.wall_coords(mask, n)
        box, u = (0, n[0], 0, n[1], 0, n[2]), (0, -1, 0, -1, 0, -1)
        gen = torch.Generator().manual_seed(7)
        src = ops.PaddedField(n, dtype=dtype)
        src.deep3().copy_(torch.rand(src.deep3().shape, generator=gen, dtype=torch.float64).to(dtype))
        want = ops.PaddedField(n, dtype=dtype)
        want.flat.fill_(SENTINEL)
        st = ops.new_state("cpu")
        ops.sweep3(src, want, D, box, u, kernel=f"tl{v.K}", state=st, walls=walls)
        plain = ops.PaddedField(n, dtype=dtype)
        ops.sweep3(src, plain, D, box, u, kernel=f"tl{v.K}")
        assert not torch.equal(plain.owned(), want.owned())  # the walls matter on this box
        dsrc = ops.PaddedField(n, dtype=dtype, device=gpu)
        dsrc.flat.copy_(src.flat)
        got = ops.PaddedField(n, dtype=dtype, device=gpu)
        got.flat.fill_(SENTINEL)
        dst = ops.new_state(gpu)
        ops.sweep3(dsrc, got, D, box, u, kernel=kernel, state=dst, walls=walls)
        torch.cuda.synchronize()
        what = f"{_vid(v)} n={n} mask={mask:06b}"
        bad = (got.flat.cpu() != want.flat).nonzero()
        assert not len(bad), f"{what}: {len(bad)} values differ, first flat index {int(bad[0])}"
        for s in range(v.K - 1 if last_only else 0, v.K):
            assert ops.residual_from_state(dst, s) == ops.residual_from_state(st, s), f"{what}: residual of step {s}"


# ---- the solver

N = (66, 101, 131)
FACES = "x-,x+,z-,z+"


def _field(N, seed=3):
    return np.random.default_rng(seed).uniform(0.0, 1.0, N)


def _run(h3d, backend, dtype, steps, N=N, faces=FACES, extra=(), T0=None, **kw):
    s = h3d.HeatSolver(N, 100000, 0.0, dtype=dtype, backend=backend, insulated=faces, extra_args=list(extra), **kw)
    s.set_field(_field(N) if T0 is None else T0)
    s.step(steps)
    s.synchronize()
    return s, s.gather(), s.native.residual_history()


@pytest.fixture(scope="module")
def cpu_13(h3d):
    """13 single steps of the CPU backend, per dtype (computed once)."""
    return {dt: _run(h3d, "cpu", dt, 13, extra=["--temporal", "1"])[1:] for dt in ("fp64", "fp32")}


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_solver_sweeps_equal_single_steps_equal_cpu(h3d, gpu, cpu_13, dtype):
    """13 steps at K = 3 (four sweeps and a single-step remainder, or long
    sweeps where the start-up timing prefers them): the wall-form sweeps, the
    single-step schedule on refreshed wall planes and the CPU backend agree bit
    for bit, field and residuals."""
    want, hist = cpu_13[dtype]
    s, T, h = _run(h3d, "hip", dtype, 13, extra=["--temporal", "3"])
    assert s.native.sweeps_active and s.kernel.startswith("tl3:1:"), s.kernel
    assert np.array_equal(T, want)
    one, T1, h1 = _run(h3d, "hip", dtype, 13, extra=["--temporal", "1"])
    assert not one.native.sweeps_active
    assert np.array_equal(T1, want) and h1 == hist
    # every residual of every sweep (no monotone check): the history too
    _, T2, h2 = _run(h3d, "hip", dtype, 13, extra=["--temporal", "3", "--no-monotone-check"])
    assert np.array_equal(T2, want) and h2 == hist


@pytest.mark.parametrize("vr,dec,extra", [(8, (2, 2, 2), ()), (8, (2, 2, 2), ("--no-overlap",)), (4, (4, 1, 1), ()),
                                          (4, (4, 1, 1), ("--no-overlap",)), (1, None, ("--no-graph",)),
                                          (4, (4, 1, 1), ("--no-graph",))])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_solver_decomposition_schedule_graphs(h3d, gpu, cpu_13, dtype, vr, dec, extra):
    """Virtual ranks: the overlapped sweep schedule (interior on the compute
    stream; deep halo and boundary pieces, the x slabs' as y-marching thin-slab
    wall tiles, on the comm stream; lagged check in a third buffer) and the
    exchange-then-sweep one, and graphs off."""
    want, _ = cpu_13[dtype]
    s, T, _ = _run(h3d, "hip", dtype, 13, extra=["--temporal", "3", *extra], virtual_ranks=vr, decomp=dec)
    assert s.native.sweeps_active
    overlapped = vr > 1 and "--no-overlap" not in extra
    assert s.native.sweeps_overlapped == overlapped
    pieces = s.native.sweep_pieces(0)
    assert (len(pieces) > 1) == overlapped and s.native.field_buffers == (3 if overlapped else 2)
    if overlapped and dec == (4, 1, 1):
        # rank 0's one boundary piece: K planes next to its neighbour, a shape the thin-slab form takes
        (b,) = pieces[1:]
        assert lv.thin_slab_form(3, b[1] - b[0], b[3] - b[2]) == (3, 3, 3), b
    assert np.array_equal(T, want), (vr, dec, extra)


def test_convergence_and_rollback(h3d, gpu):
    """Bottom 0, top 1, the four sides insulated: converges to T = y; the
    convergence iteration is the same with the monotone check (a converged
    sweep replayed with every residual) and without."""
    N33 = (33, 33, 33)
    res = []
    for extra in ((), ("--no-monotone-check",)):
        s = h3d.HeatSolver(N33, 200000, 1e-6, backend="hip", insulated=FACES, extra_args=list(extra))
        r = s.run()
        assert r["converged"]
        res.append((r["conv_iter"], r["last_residual"], s.gather()))
        # error_percent: 100 * mean |T - y| over the interior; the criterion stops
        # 33^3 short of the steady state by what the Dirichlet run of the smoke test leaves (< 0.03 %)
        print("walls 33^3 eps 1e-6:", r["conv_iter"], r["error_percent"])
        assert r["error_percent"] < 0.03
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    assert np.array_equal(res[0][2], res[1][2])


@pytest.mark.parametrize("what", ["source", "conductivity"])
def test_walls_with_source_or_conductivity(h3d, gpu, what):
    """No sweep form: single steps on refreshed wall planes, GPU == CPU."""
    N33 = (33, 33, 33)
    rng = np.random.default_rng(6)
    q, c, T0 = rng.uniform(-5.0, 5.0, N33), rng.uniform(0.1, 1.0, N33), rng.uniform(0.0, 1.0, N33)
    out = []
    for backend in ("cpu", "hip"):
        s = h3d.HeatSolver(N33, 1000, 0.0, backend=backend, insulated="x-,y+,z-,z+")
        s.set_field(T0)
        s.set_source(q) if what == "source" else s.set_conductivity(c)
        s.set_field(T0)
        assert not s.native.sweeps_active
        s.step(12)
        s.synchronize()
        out.append(s.gather())
    assert np.array_equal(out[0], out[1])


@pytest.mark.parametrize("axis", [1, 2])
@pytest.mark.parametrize("m", [1, 3])
def test_eigenmode_sweeps(h3d, gpu, axis, m):
    """tests/test_walls_cpu.py test_eigenmode through the K = 3 wall-form
    sweeps, the same bound: |err| <= 10 n 2^-53 * 4."""
    Ne, n = (18, 14, 22), 30
    s = h3d.HeatSolver(Ne, 1000, 0.0, backend="hip", insulated="all", extra_args=["--temporal", "3"])
    T0, g = s.model.neumann_mode(axis, m)
    s.set_field(T0)
    assert s.native.sweeps_active
    s.step(n)
    s.synchronize()
    err = np.abs(s.gather() - g ** n * T0)[1:-1, 1:-1, 1:-1].max()
    bound = 10 * n * 2.0 ** -53 * 4
    print(f"eigenmode axis {axis} m {m}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound
