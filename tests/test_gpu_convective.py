"""Convective (Robin) walls on the GPU: every convective form of the lean sweep
(csrc/kernels/stencil_tbl_conv_variants.inc is the test matrix) against the
CPU's K-single-steps definition, bitwise; the solver with convective and
insulated faces mixed (sweeps == single steps == CPU backend; decomposition,
schedule and graph invariance), beta = 0 against the insulated run, convergence
with the rollback on the slab problem, and source / conductivity on the
single-step path with the refresh kernel."""
import os
import re

import numpy as np
import pytest
import torch

import _lean_variants as lv
import test_gpu_walls as gw

pytestmark = pytest.mark.gpu

D = gw.D
SENTINEL = gw.SENTINEL
TORCH = gw.TORCH
_ENTRY = re.compile(r"^H3D_VC\(\s*(double|float)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,"
                    r"\s*(true|false)\s*\)\s*$", re.M)
# a coefficient per face, all different (exact in fp32 and not); AMBIENT outside the field's range [0, 1)
BETA = (0.5, 0.3, 1.0, 0.125, 0.7, 0.9)
AMBIENT = 1.75


def conv_variants():
    with open(os.path.join(lv.KERNELS, "stencil_tbl_conv_variants.inc")) as f:
        text = f.read()
    out = [lv.Variant("fp64" if m.group(1) == "double" else "fp32", *(int(m.group(i)) for i in range(2, 7)),
                      m.group(7) == "true", 0, False) for m in _ENTRY.finditer(text)]
    assert len(out) == ("\n" + text).count("\nH3D_VC") and out
    return out


VARIANTS = conv_variants()


def _mixed(mask):
    """The faces of `mask`, alternately convective (BETA) and insulated (-1),
    starting with a convective one."""
    conv, k = [-1.0] * 6, 0
    for f in range(6):
        if (mask >> f) & 1:
            if k % 2 == 0:
                conv[f] = BETA[f]
            k += 1
    return conv


def test_list_mirrors_the_wall_list():
    key = lambda v: (v.dtype, v.R, v.WY, v.K, v.NTS, v.SW)  # noqa: E731
    assert sorted(map(key, VARIANTS)) == sorted(map(key, gw.VARIANTS))


@pytest.mark.parametrize("v", VARIANTS, ids=gw._vid)
def test_conv_variant_bitwise(h3d, gpu, v):
    """One launch per box of every listed convective form against
    cpu::stencil_multi with the same faces (convective and insulated mixed, a
    coefficient per face): the stored box, the sentinel everywhere else, every
    residual slot the variant computes.  The result differs from the
    all-insulated one on every box."""
    ops, dtype = h3d.ops, TORCH[v.dtype]
    zs = lv.geometry(v)[2]
    kernel = f"tl{v.K}" if v.SW else lv.spec(v, zs=zs)
    last_only = bool(v.NTS & lv.LAST_ONLY)
    for n, mask in gw._boxes(v):
        if v.SW:
            assert lv.thin_slab_form(v.K, n[0], n[1]) == (v.R, v.WY, v.K), (n, v)
        walls, conv = ops.wall_coords(mask, n), _mixed(mask)
        assert any(b >= 0 for b in conv) and any(b < 0 and (mask >> f) & 1 for f, b in enumerate(conv))
        box, u = (0, n[0], 0, n[1], 0, n[2]), (0, -1, 0, -1, 0, -1)
        gen = torch.Generator().manual_seed(7)
        src = ops.PaddedField(n, dtype=dtype)
        src.deep3().copy_(torch.rand(src.deep3().shape, generator=gen, dtype=torch.float64).to(dtype))
        want = ops.PaddedField(n, dtype=dtype)
        want.flat.fill_(SENTINEL)
        st = ops.new_state("cpu")
        ops.sweep3(src, want, D, box, u, kernel=f"tl{v.K}", state=st, walls=walls, conv=conv, ambient=AMBIENT)
        ins = ops.PaddedField(n, dtype=dtype)
        ops.sweep3(src, ins, D, box, u, kernel=f"tl{v.K}", walls=walls)
        assert not torch.equal(ins.owned(), want.owned())  # not the insulated kernel's result
        dsrc = ops.PaddedField(n, dtype=dtype, device=gpu)
        dsrc.flat.copy_(src.flat)
        got = ops.PaddedField(n, dtype=dtype, device=gpu)
        got.flat.fill_(SENTINEL)
        dst = ops.new_state(gpu)
        ops.sweep3(dsrc, got, D, box, u, kernel=kernel, state=dst, walls=walls, conv=conv, ambient=AMBIENT)
        torch.cuda.synchronize()
        what = f"{gw._vid(v)} n={n} mask={mask:06b}"
        bad = (got.flat.cpu() != want.flat).nonzero()
        assert not len(bad), f"{what}: {len(bad)} values differ, first flat index {int(bad[0])}"
        for s in range(v.K - 1 if last_only else 0, v.K):
            assert ops.residual_from_state(dst, s) == ops.residual_from_state(st, s), f"{what}: residual of step {s}"


# ---- the solver

N = gw.N
INSULATED = "x-,z+"
CONVECTIVE = {"x+": 0.25, "y-": 0.5, "z-": 1.0}
T_INF = 0.375


def _run(h3d, backend, dtype, steps, N=N, insulated=INSULATED, convective=CONVECTIVE, extra=(), T0=None, **kw):
    s = h3d.HeatSolver(N, 100000, 0.0, dtype=dtype, backend=backend, insulated=insulated, convective=convective,
                       ambient=T_INF, extra_args=list(extra), **kw)
    s.set_field(gw._field(N) if T0 is None else T0)
    s.step(steps)
    s.synchronize()
    return s, s.gather(), s.native.residual_history()


@pytest.fixture(scope="module")
def cpu_13(h3d):
    """13 single steps of the CPU backend, per dtype (computed once)."""
    return {dt: _run(h3d, "cpu", dt, 13, extra=["--temporal", "1"])[1:] for dt in ("fp64", "fp32")}


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_solver_sweeps_equal_single_steps_equal_cpu(h3d, gpu, cpu_13, dtype):
    """13 steps at K = 3: the convective-form sweeps, the single-step schedule on
    refreshed wall planes and the CPU backend agree bit for bit, field and
    residuals; again with every residual of every sweep."""
    want, hist = cpu_13[dtype]
    s, T, h = _run(h3d, "hip", dtype, 13, extra=["--temporal", "3"])
    assert s.native.sweeps_active and s.kernel.startswith("tl3:1:"), s.kernel
    assert np.array_equal(T, want)
    one, T1, h1 = _run(h3d, "hip", dtype, 13, extra=["--temporal", "1"])
    assert not one.native.sweeps_active
    assert np.array_equal(T1, want) and h1 == hist
    _, T2, h2 = _run(h3d, "hip", dtype, 13, extra=["--temporal", "3", "--no-monotone-check"])
    assert np.array_equal(T2, want) and h2 == hist
    # the convective faces matter: not the insulated run
    _, Ti, _ = _run(h3d, "cpu", dtype, 1, insulated="x-,z+,x+,y-,z-", convective=None, extra=["--temporal", "1"])
    _, Tc, _ = _run(h3d, "cpu", dtype, 1, extra=["--temporal", "1"])
    assert not np.array_equal(Ti, Tc)


@pytest.mark.parametrize("vr,dec,extra", [(8, (2, 2, 2), ()), (8, (2, 2, 2), ("--no-overlap",)), (4, (4, 1, 1), ()),
                                          (4, (4, 1, 1), ("--no-overlap",)), (1, None, ("--no-graph",)),
                                          (4, (4, 1, 1), ("--no-graph",))])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_solver_decomposition_schedule_graphs(h3d, gpu, cpu_13, dtype, vr, dec, extra):
    """The matrix of test_gpu_walls: the overlapped sweep schedule, the
    exchange-then-sweep one, and graphs off."""
    want, _ = cpu_13[dtype]
    s, T, _ = _run(h3d, "hip", dtype, 13, extra=["--temporal", "3", *extra], virtual_ranks=vr, decomp=dec)
    assert s.native.sweeps_active
    overlapped = vr > 1 and "--no-overlap" not in extra
    assert s.native.sweeps_overlapped == overlapped
    pieces = s.native.sweep_pieces(0)
    assert (len(pieces) > 1) == overlapped and s.native.field_buffers == (3 if overlapped else 2)
    assert np.array_equal(T, want), (vr, dec, extra)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_beta_zero_is_the_insulated_run(h3d, gpu, dtype):
    """beta = 0 on a set of faces (any ambient) against the insulated run with
    the same faces, through the convective forms: field and residuals."""
    faces = "x-,y+,z-"
    _, Ti, hi = _run(h3d, "hip", dtype, 13, insulated=faces, convective=None, extra=["--temporal", "3"])
    s, Tc, hc = _run(h3d, "hip", dtype, 13, insulated=None, convective={f: 0.0 for f in faces.split(",")},
                     extra=["--temporal", "3"])
    assert s.native.sweeps_active
    assert np.array_equal(Tc, Ti) and hc == hi


def test_convergence_and_rollback(h3d, gpu):
    """The slab problem (x, z insulated, y- convective, y+ at 1): conv_iter, last
    residual and field identical to the CPU backend's, with the monotone check
    (a converged sweep replayed with every residual) and without."""
    Ns = (17, 17, 17)
    res = []
    for backend, extra in (("cpu", ()), ("hip", ()), ("hip", ("--no-monotone-check",))):
        s = h3d.HeatSolver(Ns, 200000, 1e-6, backend=backend, insulated="x-,x+,z-,z+", convective={"y-": 0.5},
                           ambient=0.25, extra_args=list(extra))
        r = s.run()
        assert r["converged"]
        T = s.gather()
        err = np.abs(T - s.model.convective_slab_steady(0.5, 0.25))[1:-1, 1:-1, 1:-1].max()
        print(f"slab {backend} {extra}: conv_iter {r['conv_iter']} last {r['last_residual']:.3e} err {err:.3e}")
        res.append((r["conv_iter"], r["last_residual"], T))
    for other in res[1:]:
        assert other[0] == res[0][0] and other[1] == res[0][1]
        assert np.array_equal(other[2], res[0][2])


@pytest.mark.parametrize("what", ["source", "conductivity"])
def test_convective_with_source_or_conductivity(h3d, gpu, what):
    """No sweep form: single steps on wall planes refreshed by the refresh
    kernel (convective) and by copies (insulated), GPU == CPU."""
    N33 = (33, 33, 33)
    rng = np.random.default_rng(6)
    q, c, T0 = rng.uniform(-5.0, 5.0, N33), rng.uniform(0.1, 1.0, N33), rng.uniform(0.0, 1.0, N33)
    out = []
    for backend in ("cpu", "hip"):
        s = h3d.HeatSolver(N33, 1000, 0.0, backend=backend, insulated="x-,z+", convective={"y+": 0.5, "z-": 0.75},
                           ambient=T_INF)
        s.set_field(T0)
        s.set_source(q) if what == "source" else s.set_conductivity(c)
        s.set_field(T0)
        assert not s.native.sweeps_active
        s.step(12)
        s.synchronize()
        out.append(s.gather())
    assert np.array_equal(out[0], out[1])
