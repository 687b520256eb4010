"""Every lean sweep variant of csrc/kernels/stencil_tbl_variants.inc that a
kernel spec selects, launched once each (the list is the test matrix,
tests/_lean_variants.py), and the edge role (spec field 9) on the slab and
block paths of a decomposed run: fields, residuals and the untouched rest of
the destination are bitwise those of the CPU's K-single-steps definition."""
import pytest
import torch

import _lean_variants as lv

pytestmark = pytest.mark.gpu

D = (0.06, 0.05, 0.04)
SENTINEL = -5.0
TORCH = {"fp64": torch.float64, "fp32": torch.float32}


def _last_only(kernel):
    parts = kernel.split(":")
    return len(parts) > 7 and bool(int(parts[7]) & lv.LAST_ONLY)


def _depth(kernel):
    return int(kernel.split(":")[0][2])


def _first_diff(got, want):
    """First differing element of two equal-shaped CPU tensors, for the report."""
    bad = (got != want).nonzero()
    if not len(bad):
        return "equal"
    i = tuple(int(v) for v in bad[0])
    return f"{len(bad)} differ, first at {i}: got {got[i].item()!r}, want {want[i].item()!r}"


def _random_field(ops, n, dtype, g, seed):
    gen = torch.Generator().manual_seed(seed)
    f = ops.PaddedField(n, dtype=dtype, gx=g[0], gy=g[1], gz=g[2])
    f.deep3().copy_(torch.rand(f.deep3().shape, generator=gen, dtype=torch.float64).to(dtype))
    return f


_cpu = {}


def _cpu_sweep(ops, dtype, K, n, g, box, u):
    """Input and, by the CPU's K single steps, the whole destination buffer
    (sentinel outside the box) and the K residuals; computed once per case."""
    key = (dtype, K, n, g, box, u)
    if key not in _cpu:
        src = _random_field(ops, n, dtype, g, 7)
        want = ops.PaddedField(n, dtype=dtype, gx=g[0], gy=g[1], gz=g[2])
        want.flat.fill_(SENTINEL)
        st = ops.new_state("cpu")
        ops.sweep3(src, want, D, box, u, kernel=f"tl{K}", state=st)
        _cpu[key] = (src, want, [ops.residual_from_state(st, s) for s in range(K)])
    return _cpu[key]


_NO_U = (0, -1, 0, -1, 0, -1)


def _check(ops, gpu, kernel, dtype, n, g, box, u=_NO_U, step2=False):
    """One GPU sweep of `kernel` against the CPU definition: the stored box,
    every residual the variant computes, and the sentinel everywhere else."""
    K = _depth(kernel)
    src, want, res = _cpu_sweep(ops, dtype, K, tuple(n), tuple(g), tuple(box), tuple(u))
    dsrc = ops.PaddedField(n, dtype=dtype, device=gpu, gx=g[0], gy=g[1], gz=g[2])
    dsrc.flat.copy_(src.flat)
    got = ops.PaddedField(n, dtype=dtype, device=gpu, gx=g[0], gy=g[1], gz=g[2])
    got.flat.fill_(SENTINEL)
    st = ops.new_state(gpu)
    if step2:
        ops.ftcs_step2(dsrc, got, D, kernel=kernel, state=st, slot=0)
    else:
        ops.sweep3(dsrc, got, D, box, u, kernel=kernel, state=st)
    torch.cuda.synchronize()
    what = f"{kernel} {dtype} n={tuple(n)} box={tuple(box)} u={tuple(u)}"
    x0, x1, y0, y1, z0, z1 = box
    a, b = got.owned().cpu()[x0:x1, y0:y1, z0:z1], want.owned()[x0:x1, y0:y1, z0:z1]
    assert torch.equal(a, b), f"{what}: box, {_first_diff(a, b)}"
    a, b = got.flat.cpu(), want.flat
    assert torch.equal(a, b), f"{what}: outside the box (flat index), {_first_diff(a, b)}"
    for s in range(K - 1 if _last_only(kernel) else 0, K):
        assert ops.residual_from_state(st, s) == res[s], f"{what}: residual of step {s}"


def variant_boxes(v):
    """The two smallest boxes that reach every code path of a variant.
    masked: fewer planes than one pipeline fill, a second tile of one row and
    one of one column, every wave in the masked form.  free: three tiles along
    y and z, the middle one mask-free (wfast / efast), 2(K-1) planes of fill
    and drain, one whole unrolled chunk of U mask-free steps and 3 planes."""
    _, YS, zs, U = lv.geometry(v)
    return {"masked": (v.K + 1, YS + 1, zs + 1), "free": (2 * (v.K - 1) + U + 3, 3 * YS, 3 * zs)}


PLAIN = lv.plain()


def test_matrix_is_the_list():
    """The parametrisation below is the list: as many items as the variant
    list has spec-selectable entries without a source."""
    text = lv.list_text()[0]
    thin = sum(1 for v in lv.parse(text) if v.SW)
    assert len(PLAIN) == lv.entry_lines(text) - thin and thin == 6
    assert len({lv.vid(v) for v in PLAIN}) == len(PLAIN)
    print(f"lean variants under test: {len(PLAIN)}")


@pytest.mark.parametrize("v", PLAIN, ids=lv.vid)
def test_listed_variant_bitwise(h3d, gpu, v):
    """One item per spec-selectable entry of stencil_tbl_variants.inc (78 today:
    35 fp64, two of them with the edge role, and 43 fp32), on its masked and
    its mask-free box, through ftcs_step2 with the z stride pinned in spec
    field 8 so that the seams are where the boxes put them."""
    zs = lv.geometry(v)[2]
    for n in variant_boxes(v).values():
        _check(h3d.ops, gpu, lv.spec(v, zs=zs), TORCH[v.dtype], n, (1, 1, 1), (0, n[0], 0, n[1], 0, n[2]), step2=True)


# ---- K = 5 and K = 6 default specs against the PyTorch oracle

def _default_specs(ext):
    out = []
    for dtype in ("fp64", "fp32"):
        for K in (5, 6):
            out.append((dtype, f"tl{K}"))
            r = ext.kernel_spec_resolved(f"tl{K}", dtype).split(":")
            # where the default is one value per lane, the pair form too if it exists
            if r[1] == "1" and ext.lean_supported(dtype, f"tl{K}:2", False):
                out.append((dtype, f"tl{K}:2"))
    return out


@pytest.mark.parametrize("dtype,K", [(d, K) for d in ("fp64", "fp32") for K in (5, 6)])
def test_deep_default_specs_match_oracle(h3d, ext, gpu, dtype, K):
    """tl5 and tl6 as the solver launches them (the shape is the dtype's
    default), on the two boxes of their shape, against K steps of the plain
    PyTorch oracle: the deepest cones are tied to the independent reference as
    K = 2..4 are in test_stencil_k_bitwise."""
    ops = h3d.ops
    specs = [s for d, s in _default_specs(ext) if d == dtype and _depth(s) == K]
    assert f"tl{K}" in specs
    r = [int(f) for f in ext.kernel_spec_resolved(f"tl{K}", dtype).split(":")[1:]]
    assert r[0] == 1, r  # the lean kernel, one value per lane
    shape = lv.Variant(dtype, r[1], r[3], K, r[5], 0, False, 0, False)
    assert shape in [v._replace(NTS=0) for v in PLAIN], shape
    for n in variant_boxes(shape).values():
        gen = torch.Generator().manual_seed(5)
        host = ops.PaddedField(n, dtype=TORCH[dtype])
        host.ghosted().copy_(torch.rand(tuple(e + 2 for e in n), generator=gen, dtype=torch.float64).to(TORCH[dtype]))
        dev = ops.PaddedField(n, dtype=TORCH[dtype], device=gpu)
        dev.flat.copy_(host.flat)
        T, refs = host.ghosted().clone(), []
        for _ in range(K):
            new, res = ops.ftcs_reference(T, D)
            T = T.clone()
            T[1:-1, 1:-1, 1:-1] = new
            refs.append(res)
        want = T[1:-1, 1:-1, 1:-1]
        for spec in specs:
            out = ops.PaddedField(n, dtype=TORCH[dtype], device=gpu)
            out.flat.copy_(dev.flat)
            out.owned().fill_(SENTINEL)
            st = ops.new_state(gpu)
            ops.ftcs_step2(dev, out, D, kernel=spec, state=st, slot=0)
            torch.cuda.synchronize()
            got = out.owned().cpu()
            assert torch.equal(got, want), f"{spec} {dtype} {n}: {_first_diff(got, want)}"
            assert torch.equal(out.ghosted().cpu(), T), f"{spec} {dtype} {n}: ghost shell written"
            assert [ops.residual_from_state(st, s) for s in range(K)] == refs, (spec, n)


# ---- the edge role on the paths of a decomposed run

K4 = 4
# fp64 K = 4, 12 waves of 4 rows, last residual only: the plain 48-row tile
# (the control: same shape, no role), the role with E = 0 and with E = 2 owned
# rows per edge wave (52-row tiles).  spec -> (stored rows YS, E)
EDGE = {"tl4:1:4:1:12:0:3:66": (40, 0), "tl4:1:4:1:12:0:3:66:0:1": (40, 0), "tl4:1:4:1:12:0:3:66:0:3": (44, 2)}


def test_edge_specs_are_listed():
    for spec, (YS, E) in EDGE.items():
        v = [v for v in PLAIN if lv.spec(v) == spec]
        assert len(v) == 1 and lv.geometry(v[0])[1] == YS and max(v[0].EW - 1, 0) == E, spec


@pytest.mark.parametrize("n0,box_x,side", [(4, (0, 4), "both"), (9, (0, 9), "hi"), (12, (4, 8), "both"),
                                            (30, (0, 30), "both")])
@pytest.mark.parametrize("spec", list(EDGE))
def test_edge_sweep_slab_path(h3d, gpu, spec, n0, box_x, side):
    """x slabs: K ghost planes, the x update range widened into them, three
    tiles along y (the middle one's edge waves mask-free), thin, partial and
    whole x boxes."""
    YS, _ = EDGE[spec]
    n = (n0, 3 * YS, 133)
    ux = (-(K4 - 1) if side in ("lo", "both") else 0, n0 + (K4 - 1 if side in ("hi", "both") else 0))
    _check(h3d.ops, gpu, spec, torch.float64, n, (K4, 1, 1), (box_x[0], box_x[1], 0, n[1], 0, n[2]), ux + (0, -1, 0, -1))


def _block_cases(YS, E):
    """(box, sides) on the field (12, 3 YS + 6, 140) with K-deep ghosts on every axis."""
    ny = 3 * YS + 6
    cases = [((0, 12, 0, ny, 0, 140), s) for s in ("lo", "hi", "both")]  # y1 = n_y: the last tile's waves end in the ghosts
    cases += [
        # tile rows off the layout origin (r00 = 3 - K); with y1 = n_y the last full tile's
        # edge wave has its halo rows in the deep ghost, inside the y update range
        ((0, 12, 3, ny, 0, 140), "both"), ((0, 12, 3, ny, 0, 140), "hi"),
        # a last tile of one stored row: its stored rows end inside wave 0's owned rows,
        # and every other wave, the upper edge wave included, lies past the box inside the field
        ((0, 12, 3, 3 + YS + 1, 0, 140), "both"),
        # ... and just past wave 0's owned rows
        ((0, 12, 3, 3 + YS + E + 1, 0, 140), "both"),
        ((3, 9, 0, 4, 0, 140), "both"),             # 4 rows
        ((2, 10, 3, ny - 3, 0, 4), "both"),         # 4 columns
        ((0, 12, ny - 4, ny, 5, 135), "both"),
        ((0, 12, 0, ny, 136, 140), "both"),
        ((2, 10, YS, 2 * YS, 5, 135), "both"),      # an interior piece of one whole tile
    ]
    return list(dict.fromkeys(cases))


def _block_u(n, sides):
    lo, hi = sides in ("lo", "both"), sides in ("hi", "both")
    u = []
    for a in range(3):
        u += [-(K4 - 1) if lo else 0, n[a] + (K4 - 1 if hi else 0)]
    return tuple(u)


_BLOCK = [pytest.param(spec, box, sides, id=f"{spec}-{'_'.join(map(str, box))}-{sides}")
          for spec, (YS, E) in EDGE.items() for box, sides in _block_cases(YS, E)]


@pytest.mark.parametrize("spec,box,sides", _BLOCK)
def test_edge_sweep_block_path(h3d, gpu, spec, box, sides):
    """Block decompositions: deep ghosts and update ranges on every axis, boxes
    that start and end away from 0 and n.  The edge waves' mask-free predicate
    (every row inside the box and the update range), their row masks and the
    clamped row offsets at the ends of the allocation, and owned rows of an
    edge wave cut by the box's end."""
    YS, _ = EDGE[spec]
    n = (12, 3 * YS + 6, 140)
    _check(h3d.ops, gpu, spec, torch.float64, n, (K4, K4, K4), box, _block_u(n, sides))


@pytest.mark.parametrize("spec", list(EDGE))
def test_edge_sweep_block_path_fixed_segments(h3d, gpu, spec):
    """Several pieces per tile (spec field L = 8: x segments of 8 planes, each
    with its own fill and drain) on the block path."""
    YS, _ = EDGE[spec]
    n = (12, 3 * YS + 6, 140)
    parts = spec.split(":")
    parts[5] = "8"
    _check(h3d.ops, gpu, ":".join(parts), torch.float64, n, (K4, K4, K4), (0, 12, 0, n[1], 0, 140), _block_u(n, "both"))
