"""The lean sweep's form dispatch (no GPU): its thin-slab rule against the
tests' copy of it, and the tile every default spec and every listed line runs
as in each of the six forms (source or none x no, insulated or convective
walls) against that form's variant list."""
import itertools
import os
import re

import pytest

import _lean_variants as lv

# (with_source, wall: 0 none / 1 insulated / 2 convective) -> the form's list and its macro
LISTS = {(False, 0): ("stencil_tbl_variants.inc", "H3D_V"), (True, 0): ("stencil_tbl_src_variants.inc", "H3D_VS"),
         (False, 1): ("stencil_tbl_wall_variants.inc", "H3D_VW"), (False, 2): ("stencil_tbl_conv_variants.inc", "H3D_VC"),
         (True, 1): ("stencil_tbl_wall_src_variants.inc", "H3D_VWS"),
         (True, 2): ("stencil_tbl_conv_src_variants.inc", "H3D_VCS")}

# The default shapes that run as another shape, read off the four dispatch
# functions of the wall forms as they stood before they became one (the source
# forms' redirections; every other default runs its own shape):
# (with_source, wall, dtype, K, last residual only) -> (R, WY)
REDIRECTED = {(True, 1, "fp64", 3, False): (4, 12),  # 3 x 16
              (True, 1, "fp64", 2, False): (6, 12),  # 5 x 16 (with the last residual only: itself)
              (True, 1, "fp32", 4, False): (4, 12),  # 4 x 16
              (True, 2, "fp64", 3, False): (4, 12),  # 3 x 16
              (True, 2, "fp64", 4, False): (5, 8),   # 3 x 12
              (True, 2, "fp64", 2, False): (6, 12),  # 5 x 16
              (True, 2, "fp64", 2, True): (6, 12),   # 5 x 16
              (True, 2, "fp32", 4, False): (4, 12)}  # 4 x 16


def _listed(form):
    """(dtype, R, WY, K, Q, NTS, SW) of every line of the form's list (edge-role lines left out)."""
    name, macro = LISTS[form]
    with open(os.path.join(lv.KERNELS, name)) as f:
        text = f.read()
    out = set()
    for m in re.finditer(r"^" + macro + r"\(\s*(double|float)\s*,([^)]*)\)\s*$", text, re.M):
        f = [x.strip() for x in m.group(2).split(",")]
        out.add(("fp64" if m.group(1) == "double" else "fp32", *map(int, f[:5]), f[5] == "true"))
    assert len(out) == len(re.findall(r"^" + macro + r"\(", text, re.M)) and out
    return out


def _edge_listed():
    """(dtype, R, WY, K, Q, NTS, SW, EW) of the edge-role lines (the plain form's list alone has any)."""
    for form, (name, macro) in LISTS.items():
        with open(os.path.join(lv.KERNELS, name)) as f:
            assert (macro + "E(" in f.read()) == (form == (False, 0)), name
    return {(v.dtype, v.R, v.WY, v.K, v.Q, v.NTS, v.SW, v.EW) for v in lv.variants() if v.EW}


def _supported(ext, dtype, spec, src, wall):
    if wall == 0:
        return ext.lean_supported(dtype, spec, src)
    if src:
        return ext.lean_wall_source_supported(dtype, spec, wall == 2)
    return (ext.lean_wall_supported, ext.lean_conv_supported)[wall - 1](dtype, spec)


def test_thin_slab_rule_matches_the_tests_copy(ext):
    for K, ex, ey, dflt in itertools.product(range(2, 6), range(0, 11), (0, 15, 16, 63, 64, 160, 161), (True, False)):
        want = lv.thin_slab_form(K, ex, ey, default_spec=dflt)
        got = ext.lean_thin_slab(K, dflt, ex, ey)
        assert (None if got is None else (*got, K)) == want, (K, ex, ey, dflt, got, want)


# the default tile (R, WY) of the one-value-per-lane lean kernel (KernelSpec::resolved)
DEFAULT = {("fp64", 2): (5, 16), ("fp64", 3): (3, 16), ("fp64", 4): (3, 12),
           ("fp32", 2): (3, 16), ("fp32", 3): (3, 16), ("fp32", 4): (4, 16)}


@pytest.mark.parametrize("src,wall", sorted(LISTS))
def test_default_shapes_of_every_form(ext, src, wall):
    listed = _listed((src, wall))
    for dtype, K, last in itertools.product(("fp64", "fp32"), (2, 3, 4), (False, True)):
        r = ext.kernel_spec_resolved(f"tl{K}:1", dtype).split(":")
        assert (int(r[2]), int(r[4])) == DEFAULT[dtype, K], r
        V = 0
        if not src and wall == 0 and dtype == "fp32":
            # the plain fp32 default is the packed-pair kernel, which has no tile of these
            # lists: no shape; the lean kernel's default tile is asked for with V = 1
            assert ext.kernel_spec_resolved(f"tl{K}", dtype).split(":")[1] == "2"
            assert ext.lean_supported(dtype, f"tl{K}", False) and ext.lean_shape(dtype, f"tl{K}", False, 0) is None
            V = 1
        spec = f"tl{K}:{V}:0:0:0:0:0:{2 | lv.LAST_ONLY}" if last else f"tl{K}:{V}" if V else f"tl{K}"
        got = ext.lean_shape(dtype, spec, src, wall)
        if not _supported(ext, dtype, spec, src, wall):
            assert got is None, (dtype, spec, got)
            assert last, (dtype, spec)  # the defaults themselves exist in every form
            continue
        want = REDIRECTED.get((src, wall, dtype, K, last), DEFAULT[dtype, K])
        assert got == (*want, False), (dtype, spec, got, want)
        nts = 2 | lv.LAST_ONLY if last else 2 if dtype == "fp64" else 0
        assert (dtype, *want, K, 3, nts, False) in listed, (dtype, spec, want, nts)


def test_redirections_name_listed_shapes_only():
    """Every pinned redirection leaves a default shape that its form does not list
    for one that it does."""
    for (src, wall, dtype, K, last), to in REDIRECTED.items():
        shapes = {(d, R, WY, k) for d, R, WY, k, _q, nts, sw in _listed((src, wall))
                  if not sw and bool(nts & lv.LAST_ONLY) == last}
        assert (dtype, *to, K) in shapes, (src, wall, dtype, K, last, to)
        own = {("fp64", 2): (5, 16), ("fp64", 3): (3, 16), ("fp64", 4): (3, 12), ("fp32", 4): (4, 16)}[(dtype, K)]
        assert (dtype, *own, K) not in shapes, (src, wall, dtype, K, last, own)


@pytest.mark.parametrize("src,wall", sorted(LISTS))
def test_a_listed_line_runs_as_itself(ext, src, wall):
    """The spec that names a spec-selectable (non-SW) line of a form's list runs
    that line's tile: a listed line is never redirected (the premise is
    test_redirections_name_listed_shapes_only).  Edge-role lines carry field 9."""
    lines = {(*line, 0) for line in _listed((src, wall))}
    if (src, wall) == (False, 0):
        edge = _edge_listed()
        assert edge and not edge & lines
        lines |= edge
    seen = 0
    for dtype, R, WY, K, Q, NTS, SW, EW in sorted(lines):
        if SW:
            continue
        spec = lv.spec(lv.Variant(dtype, R, WY, K, Q, NTS, SW, EW, src))
        assert len(spec.split(":")) == (10 if EW else 8) and (not EW or spec.endswith(f":{EW}")), spec
        assert _supported(ext, dtype, spec, src, wall), (dtype, spec)
        assert ext.lean_shape(dtype, spec, src, wall) == (R, WY, False), (dtype, spec)
        seen += 1
    assert seen == len(lines) - 6  # three thin-slab (SW) lines per dtype in every list
