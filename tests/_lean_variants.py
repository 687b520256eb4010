"""The lean K-step sweep's variant lists (csrc/kernels/stencil_tbl_variants.inc and
stencil_tbl_src_variants.inc) as the test matrix: every H3D_V / H3D_VE / H3D_VS
line becomes a record, and every record that a kernel spec can select becomes a
spec string.  tests/test_lean_variants_cpu.py ties the table to the dispatch
(stencil_tbl_form.hpp dispatch_tbl_form, which stencil_tbl.hip hands the same
lists), tests/test_gpu_lean_variants.py launches every entry."""
import os
import re
from collections import namedtuple

KERNELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "kernels")
LISTS = ("stencil_tbl_variants.inc", "stencil_tbl_src_variants.inc")

# SW: the y-marching thin-slab forms, picked by box shape and not by spec;
# EW: the edge role (spec field 9); src: the heat-source form
Variant = namedtuple("Variant", "dtype R WY K Q NTS SW EW src")

_INT = r"\s*(\d+)\s*"
_ENTRY = re.compile(r"^H3D_V(E|S|)\(\s*(double|float)\s*," + _INT + "," + _INT + "," + _INT + "," + _INT + "," + _INT +
                    r",\s*(true|false)\s*,(?:" + _INT + ",)?" + _INT + r"\)\s*$", re.M)
LAST_ONLY = 64  # store-field bit: only the last step's residual is computed


def list_text(directory=KERNELS):
    out = []
    for name in LISTS:
        with open(os.path.join(directory, name)) as f:
            out.append(f.read())
    return out


def entry_lines(text):
    """Lines that begin a list entry, counted without the parser's regex."""
    return ("\n" + text).count("\nH3D_V")


def parse(text):
    out = []
    for m in _ENTRY.finditer(text):
        kind, real, R, WY, K, Q, NTS, SW, EW, _part = m.groups()
        if (kind == "E") != (EW is not None):
            raise ValueError(f"malformed entry: {m.group(0)}")
        out.append(Variant("fp64" if real == "double" else "fp32", int(R), int(WY), int(K), int(Q), int(NTS),
                           SW == "true", int(EW or 0), kind == "S"))
    return out


def variants(directory=KERNELS):
    return [v for text in list_text(directory) for v in parse(text)]


def spec(v, zs=0, L=0):
    """The kernel spec that selects v (SW forms have none).  Field 7 is always
    written, so KernelSpec::resolved substitutes no default store policy."""
    assert not v.SW
    s = f"tl{v.K}:1:{v.R}:1:{v.WY}:{L}:{v.Q}:{v.NTS}"
    if v.EW:
        return f"{s}:{zs}:{v.EW}"
    return f"{s}:{zs}" if zs else s


def vid(v):
    return f"{v.dtype}-{spec(v)}"


def geometry(v):
    """Tile rows, stored rows, stored columns and the x unroll of a variant
    (stencil_tbl_kernel.inc: TY, YS, 64 - 2K, U)."""
    TY = v.WY * v.R + 2 * max(v.EW - 1, 0)
    return TY, TY - 2 * v.K, 64 - 2 * v.K, 12 if v.Q == 4 else 6


def plain():
    """Spec-selectable variants without a source: the GPU test matrix."""
    return [v for v in variants() if not v.SW and not v.src]


def thin_slab_form(K, box_extent_x, box_extent_y, default_spec=True):
    """The lean dispatch's choice of a y-marching (SW) form by box shape
    (kernels.hpp lean_thin_slab), as (R, WY, K), or None: the x-marching tile."""
    ex, ey = box_extent_x, box_extent_y
    if not default_spec or ex <= 0 or ey < 16 * ex:
        return None
    if K == 3 and ex == 4:
        return (2, 5, 3)
    if K == 3 and ex <= 2 * K:
        return (3, 3, 3)
    if K == 4 and ex <= K:
        return (3, 4, 4)
    return None
