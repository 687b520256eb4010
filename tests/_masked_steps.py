"""The step forms of the lean K = 4 edge-role sweep (stencil_tbl_kernel.inc):
the shapes test_gpu_masked_steps.py runs, and a transcription of the kernel's
per-wave, per-step classification, so that a test without a GPU can say which
form each listed shape reaches (test_masked_steps_cpu.py)."""
from collections import Counter

K, R, WY, E, U = 4, 4, 12, 2, 6
RB = R + E
TY = WY * R + 2 * E   # 52 tile rows
YS = TY - 2 * K       # 44 stored
ZS = 64 - 2 * K       # 56 stored columns (lean_z_stride: boxes under 500 planes)
SPEC = "tl4:1:4:1:12:0:3:66:0:3"


def spec(L):
    """The edge spec with x segments of L planes (field 5; one piece per tile
    and segment, each with its own pipeline fill)."""
    p = SPEC.split(":")
    p[5] = str(L)
    return ":".join(p)


# name -> ((nx, ny, nz), L).  Whole boxes, one Dirichlet ghost layer, the update
# range the box itself.
SHAPES = {
    # 1 x 2 tiles, the second column overhanging: z-masked interior waves,
    # fully masked y-edge waves
    "z-overhang": ((14, YS, ZS + 5), 16),
    # 2 x 2 tiles, both axes overhanging; the last column stores one lane
    "yz-overhang": ((14, YS + 3, ZS + 1), 16),
    # three tile rows: the edge waves at the seams are y-free, z-masked
    "edge-roles": ((14, 2 * YS + 3, ZS + 5), 16),
    # one tile column of exactly the stride: z-masked by the update range
    # only (the regression guard of zfast)
    "z-exact": ((14, YS + 3, ZS), 16),
    # three tile columns: the middle one is mask-free next to z-masked ones
    "z-middle": ((14, 2 * YS + 3, 2 * ZS + 5), 16),
    # short x segments: seg < 2(K - 1), seg = U, seg just past U; fills that
    # run into the end of the piece, padded chunks left early
    "x1": ((1, YS, ZS + 5), 6),
    "x2": ((2, YS, ZS + 5), 6),
    "x5": ((5, YS, ZS + 5), 2),
    "x6": ((6, YS, ZS + 5), 6),
    "x7": ((7, YS, ZS + 5), 7),
    "x13-6": ((13, YS, ZS + 5), 6),
    "x13-7": ((13, 2 * YS + 3, ZS + 5), 7),
}

ROLES = ("low-edge", "interior", "high-edge")
FORMS = ("free", "z", "masked", "masked-fill", "left")


def classify(n, L, blo=None, bhi=None, u=None):
    """Counter of (role, form) over every (tile, piece, wave, plane step) of one
    sweep of the box [blo, bhi) (default: the whole field) with the update
    ranges u = (xlo, xhi, ylo, yhi, zlo, zhi) (default: the box).  Forms: `free`
    (no mask), `z` (z conditions only), `masked`, `masked-fill` (masked with at
    least one dead stage skipped), `left` (a padded step that is not run)."""
    blo = blo or (0, 0, 0)
    bhi = bhi or tuple(n)
    u = u or (blo[0], bhi[0], blo[1], bhi[1], blo[2], bhi[2])
    ulo, uhi, uylo, uyhi, uzlo, uzhi = u
    nxb = bhi[0] - blo[0]
    nyb = max(1, -(-(bhi[1] - blo[1]) // YS))
    nzb = max(1, -(-(bhi[2] - blo[2]) // ZS))
    seg = max(1, min(L, nxb))      # fixed_xplan
    nxs = -(-nxb // seg)
    c00, r00 = blo[2] - K, blo[1] - K
    out = Counter()
    for ybk in range(nyb):
        for zb in range(nzb):
            c0 = c00 + zb * ZS
            zfast = c0 >= uzlo and c0 + 64 <= uzhi
            for xs in range(nxs):
                xa = blo[0] + xs * seg
                xe = blo[0] + min(xs * seg + seg, nxb)
                x0, xlast = xa - (K - 1), xe + K - 2
                xf_lo = max(x0 + 2 * (K - 1), ulo + K - 1, blo[0] + K - 1)
                xf_hi = min(xlast, uhi - 1, bhi[0] + K - 2)
                for wave in range(WY):
                    tr0 = E + wave * R if wave > 0 else 0
                    yb = r00 + ybk * YS + tr0
                    if wave in (0, WY - 1):
                        role = ROLES[0] if wave == 0 else ROLES[2]
                        yfree = yb >= max(uylo, blo[1]) and yb + RB <= min(uyhi, bhi[1])
                    else:
                        role = ROLES[1]
                        yfree = (tr0 >= K and tr0 + R <= TY - K and yb >= uylo and yb + R <= uyhi
                                 and yb >= blo[1] and yb + R <= bhi[1])
                    for xb in range(x0, xlast + 1, U):
                        for x in range(xb, xb + U):
                            if x > xlast:
                                form = "left"
                            elif yfree and xf_lo <= x <= xf_hi:
                                form = "free" if zfast else "z"
                            elif any(x < x0 + 2 * s for s in range(1, K)):
                                form = "masked-fill"
                            else:
                                form = "masked"
                            out[(role, form)] += 1
    return out
