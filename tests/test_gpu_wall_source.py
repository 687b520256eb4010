"""A heat source behind insulated or convective walls on the GPU: every form of
the lean sweep with walls and a source (csrc/kernels/stencil_tbl_wall_src_variants.inc
and stencil_tbl_conv_src_variants.inc are the test matrix) against the CPU's
K-single-steps definition, bitwise; the solver with --wall-source-sweeps (sweeps
== the flag-off single steps == CPU backend; decomposition, schedule and graph
invariance) and convergence with the rollback on the heated slab."""
import os
import re

import numpy as np
import pytest
import torch

import _lean_variants as lv
import test_gpu_convective as gc
import test_gpu_walls as gw

pytestmark = pytest.mark.gpu

D = gw.D
SENTINEL = gw.SENTINEL
TORCH = gw.TORCH
AMBIENT = gc.AMBIENT
LISTS = {"wall": ("stencil_tbl_wall_src_variants.inc", "H3D_VWS"), "conv": ("stencil_tbl_conv_src_variants.inc", "H3D_VCS")}


def src_variants(kind):
    name, macro = LISTS[kind]
    entry = re.compile(r"^" + macro + r"\(\s*(double|float)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,"
                       r"\s*(true|false)\s*\)\s*$", re.M)
    with open(os.path.join(lv.KERNELS, name)) as f:
        text = f.read()
    out = [lv.Variant("fp64" if m.group(1) == "double" else "fp32", *(int(m.group(i)) for i in range(2, 7)),
                      m.group(7) == "true", 0, True) for m in entry.finditer(text)]
    assert len(out) == ("\n" + text).count("\n" + macro) and out
    return out


CASES = [(kind, v) for kind in ("wall", "conv") for v in src_variants(kind)]


def test_lists_cover_the_source_forms():
    """Both lists hold what stencil_tbl_src_variants.inc holds: per dtype the three
    thin-slab forms, depth 2, 3 and 4 with every residual, and for fp64 the same
    three with the last residual only (the tile shape of an entry may differ: a
    shape that spills in this form is replaced by one that does not)."""
    key = lambda v: (v.dtype, v.K, v.NTS, v.SW)  # noqa: E731
    want = sorted(key(v) for v in lv.variants() if v.src)
    for kind in LISTS:
        vs = src_variants(kind)
        assert sorted(map(key, vs)) == want and len(set(vs)) == len(vs), kind
        assert {(v.R, v.WY, v.K) for v in vs if v.SW} == {(2, 5, 3), (3, 3, 3), (3, 4, 4)}


@pytest.mark.parametrize("kind,v", CASES, ids=[f"{k}-{gw._vid(v)}" for k, v in CASES])
def test_source_variant_bitwise(h3d, gpu, kind, v):
    """One launch per box of every listed form with a random source against
    cpu::stencil_multi with the same faces and source: the stored box, the
    sentinel everywhere else, every residual slot the variant computes.  The
    result differs from the same sweep without the source."""
    ops, dtype = h3d.ops, TORCH[v.dtype]
    zs = lv.geometry(v)[2]
    kernel = f"tl{v.K}" if v.SW else lv.spec(v, zs=zs)
    assert h3d.native().lean_wall_source_supported(v.dtype, f"tl{v.K}" if v.SW else lv.spec(v), kind == "conv")
    last_only = bool(v.NTS & lv.LAST_ONLY)
    for n, mask in gw._boxes(v):
        if v.SW:
            assert lv.thin_slab_form(v.K, n[0], n[1]) == (v.R, v.WY, v.K), (n, v)
        walls = ops.wall_coords(mask, n)
        kw = dict(walls=walls, conv=gc._mixed(mask), ambient=AMBIENT) if kind == "conv" else dict(walls=walls)
        box, u = (0, n[0], 0, n[1], 0, n[2]), (0, -1, 0, -1, 0, -1)
        gen = torch.Generator().manual_seed(7)
        src = ops.PaddedField(n, dtype=dtype)
        src.deep3().copy_(torch.rand(src.deep3().shape, generator=gen, dtype=torch.float64).to(dtype))
        S = ops.PaddedField(n, dtype=dtype)
        S.deep3().copy_((2.0 * torch.rand(S.deep3().shape, generator=gen, dtype=torch.float64) - 1.0).to(dtype))
        want = ops.PaddedField(n, dtype=dtype)
        want.flat.fill_(SENTINEL)
        st = ops.new_state("cpu")
        ops.sweep3(src, want, D, box, u, kernel=f"tl{v.K}", state=st, source=S, **kw)
        dsrc, dS = ops.PaddedField(n, dtype=dtype, device=gpu), ops.PaddedField(n, dtype=dtype, device=gpu)
        dsrc.flat.copy_(src.flat)
        dS.flat.copy_(S.flat)
        got = ops.PaddedField(n, dtype=dtype, device=gpu)
        got.flat.fill_(SENTINEL)
        dst = ops.new_state(gpu)
        ops.sweep3(dsrc, got, D, box, u, kernel=kernel, state=dst, source=dS, **kw)
        nosrc = ops.PaddedField(n, dtype=dtype, device=gpu)
        ops.sweep3(dsrc, nosrc, D, box, u, kernel=f"tl{v.K}", **kw)  # (the plain wall form's default shape)
        torch.cuda.synchronize()
        what = f"{kind} {gw._vid(v)} n={n} mask={mask:06b}"
        bad = (got.flat.cpu() != want.flat).nonzero()
        assert not len(bad), f"{what}: {len(bad)} values differ, first flat index {int(bad[0])}"
        for s in range(v.K - 1 if last_only else 0, v.K):
            assert ops.residual_from_state(dst, s) == ops.residual_from_state(st, s), f"{what}: residual of step {s}"
        assert not torch.equal(nosrc.owned(), got.owned()), what


def test_forms_listed_and_others_refused(h3d, gpu):
    """The default specs at depth 2, 3 and 4 have the form in both dtypes and both
    wall kinds; a sweep with walls, a source and a spec without it is an error
    that writes nothing, never other arithmetic."""
    ext, ops = h3d.native(), h3d.ops
    for dt in ("fp64", "fp32"):
        for conv in (False, True):
            for spec in ("tl2", "tl3", "tl4"):
                assert ext.lean_wall_source_supported(dt, spec, conv), (dt, spec, conv)
            for spec in ("tl3:2", "tl5", "tv3"):
                assert not ext.lean_wall_source_supported(dt, spec, conv), (dt, spec, conv)
    n = (8, 40, 70)
    T, S, out = (ops.PaddedField(n, device=gpu) for _ in range(3))
    T.flat.fill_(0.5)
    S.flat.fill_(0.25)
    box, u = (0, n[0], 0, n[1], 0, n[2]), (0, -1, 0, -1, 0, -1)
    for conv in (None, [0.5] * 6):
        with pytest.raises(RuntimeError, match="with a heat source"):
            ops.sweep3(T, out, D, box, u, kernel="tl5", source=S, walls=ops.wall_coords(63, n), conv=conv)
        for spec in ("tl3:2", "tv3"):
            # (the pair kernel has no wall form; a tv kernel needs a conductivity field)
            with pytest.raises(RuntimeError, match="no insulated-wall form|need a conductivity"):
                ops.sweep3(T, out, D, box, u, kernel=spec, source=S, walls=ops.wall_coords(63, n), conv=conv)
    torch.cuda.synchronize()
    assert torch.count_nonzero(out.flat) == 0


# ---- the solver

N = gw.N
FACE_SETS = {"insulated": dict(insulated=gw.FACES, convective=None, ambient=0.0),
             "mixed": dict(insulated=gc.INSULATED, convective=gc.CONVECTIVE, ambient=gc.T_INF)}


def _source(N, seed=5):
    return np.random.default_rng(seed).uniform(-5.0, 5.0, N)


def _run(h3d, backend, dtype, steps, faces="mixed", flag=True, extra=(), **kw):
    s = h3d.HeatSolver(N, 100000, 0.0, dtype=dtype, backend=backend, wall_source_sweeps=flag, extra_args=list(extra),
                       **FACE_SETS[faces], **kw)
    s.set_field(gw._field(N))
    s.set_source(_source(N))
    s.step(steps)
    s.synchronize()
    return s, s.gather(), s.native.residual_history()


@pytest.fixture(scope="module")
def cpu_13(h3d):
    """13 single steps of the CPU backend with the source, per face set and dtype (computed once)."""
    return {(f, dt): _run(h3d, "cpu", dt, 13, faces=f, flag=False, extra=["--temporal", "1"])[1:]
            for f in FACE_SETS for dt in ("fp64", "fp32")}


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("faces", sorted(FACE_SETS))
def test_solver_sweeps_equal_single_steps_equal_cpu(h3d, gpu, cpu_13, faces, dtype):
    """13 steps at K = 3 with the flag on: the sweeps of walls and source
    together, the flag-off single-step schedule and the CPU backend agree bit
    for bit, field and residuals; again with every residual of every sweep."""
    want, hist = cpu_13[(faces, dtype)]
    s, T, h = _run(h3d, "hip", dtype, 13, faces=faces, extra=["--temporal", "3"])
    assert s.native.sweeps_active and s.kernel.startswith("tl3:1:"), s.kernel
    assert np.array_equal(T, want)
    off, T1, h1 = _run(h3d, "hip", dtype, 13, faces=faces, flag=False, extra=["--temporal", "3"])
    assert not off.native.sweeps_active
    assert np.array_equal(T1, want) and h1 == hist
    _, T2, h2 = _run(h3d, "hip", dtype, 13, faces=faces, extra=["--temporal", "3", "--no-monotone-check"])
    assert np.array_equal(T2, want) and h2 == hist
    if dtype == "fp32":  # every residual either way (residual_last_ok)
        assert h == hist


@pytest.mark.parametrize("vr,dec,extra", [(8, (2, 2, 2), ()), (8, (2, 2, 2), ("--no-overlap",)), (4, (4, 1, 1), ()),
                                          (4, (4, 1, 1), ("--no-overlap",)), (1, None, ("--no-graph",)),
                                          (4, (4, 1, 1), ("--no-graph",))])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_solver_decomposition_schedule_graphs(h3d, gpu, cpu_13, dtype, vr, dec, extra):
    """The matrix of test_gpu_convective with the flag on and a source: the
    overlapped sweep schedule, the exchange-then-sweep one, and graphs off."""
    want, _ = cpu_13[("mixed", dtype)]
    s, T, _ = _run(h3d, "hip", dtype, 13, extra=["--temporal", "3", *extra], virtual_ranks=vr, decomp=dec)
    assert s.native.sweeps_active
    overlapped = vr > 1 and "--no-overlap" not in extra
    assert s.native.sweeps_overlapped == overlapped
    pieces = s.native.sweep_pieces(0)
    assert (len(pieces) > 1) == overlapped and s.native.field_buffers == (3 if overlapped else 2)
    assert np.array_equal(T, want), (vr, dec, extra)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_solver_x_slabs_insulated(h3d, gpu, cpu_13, dtype):
    """Insulated walls only on 4 x slabs, overlapped: rank 0's boundary piece is a
    shape the y-marching thin-slab form with walls and a source takes."""
    want, _ = cpu_13[("insulated", dtype)]
    s, T, _ = _run(h3d, "hip", dtype, 13, faces="insulated", extra=["--temporal", "3"], virtual_ranks=4, decomp=(4, 1, 1))
    assert s.native.sweeps_active and s.native.sweeps_overlapped
    (b,) = s.native.sweep_pieces(0)[1:]
    assert lv.thin_slab_form(3, b[1] - b[0], b[3] - b[2]) == (3, 3, 3), b
    assert np.array_equal(T, want)


def test_convergence_and_rollback(h3d, gpu):
    """The heated slab (x, z insulated, y- convective, y+ at 1, a uniform source):
    conv_iter, last residual and field identical to the CPU backend's, with the
    monotone check (a converged sweep replayed with every residual) and without."""
    Ns, q = (17, 17, 17), 8.0
    res = []
    for backend, extra in (("cpu", ()), ("hip", ()), ("hip", ("--no-monotone-check",))):
        s = h3d.HeatSolver(Ns, 200000, 1e-6, backend=backend, insulated="x-,x+,z-,z+", convective={"y-": 0.5},
                           ambient=0.25, wall_source_sweeps=True, extra_args=list(extra))
        s.set_source(np.full(Ns, q))
        assert s.native.sweeps_active == (backend == "hip")
        r = s.run()
        assert r["converged"]
        T = s.gather()
        err = np.abs(T - s.model.convective_slab_source_steady(0.5, 0.25, q))[1:-1, 1:-1, 1:-1].max()
        print(f"heated slab {backend} {extra}: conv_iter {r['conv_iter']} last {r['last_residual']:.3e} err {err:.3e}")
        res.append((r["conv_iter"], r["last_residual"], T))
    for other in res[1:]:
        assert other[0] == res[0][0] and other[1] == res[0][1]
        assert np.array_equal(other[2], res[0][2])
