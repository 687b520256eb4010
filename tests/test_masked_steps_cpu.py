"""Which step form (stencil_tbl_kernel.inc: mask-free, z-masked, masked, masked
with dead fill stages skipped, padded step left) each shape of
test_gpu_masked_steps.py reaches, from a transcription of the kernel's
classification (tests/_masked_steps.py): keeps the GPU list honest without a GPU."""
from collections import Counter

import _masked_steps as ms


def _forms(name):
    n, L = ms.SHAPES[name]
    return ms.classify(n, L)


def _has(c, role, form):
    return c[(role, form)] > 0


def test_every_form_of_every_role_is_reached():
    total = Counter()
    for name in ms.SHAPES:
        total += _forms(name)
    missing = [(r, f) for r in ms.ROLES for f in ms.FORMS if not _has(total, r, f)]
    assert not missing, missing


def test_z_overhang_splits_by_rows():
    """One tile row: the interior waves are z-masked in both tile columns, the
    two edge waves (rows outside the box) fully masked; nothing is mask-free."""
    c = _forms("z-overhang")
    assert _has(c, "interior", "z") and not any(_has(c, r, "free") for r in ms.ROLES)
    for r in ("low-edge", "high-edge"):
        assert not _has(c, r, "z") and _has(c, r, "masked") and _has(c, r, "masked-fill")


def test_edge_roles_reach_the_z_form():
    c = _forms("edge-roles")
    assert all(_has(c, r, "z") for r in ms.ROLES)
    assert all(_has(c, r, "masked") for r in ms.ROLES)  # the box's first and last tile row


def test_exact_stride_is_z_masked_by_the_update_range():
    """nz = the stride: one tile column whose K halo columns on either side are
    outside the update range, so zfast is false and no step is mask-free."""
    n, L = ms.SHAPES["z-exact"]
    assert n[2] == ms.ZS
    c = _forms("z-exact")
    assert _has(c, "interior", "z") and not any(_has(c, r, "free") for r in ms.ROLES)


def test_middle_column_stays_mask_free():
    c = _forms("z-middle")
    assert all(_has(c, r, "free") and _has(c, r, "z") for r in ms.ROLES)


def test_short_segments():
    # seg < 2(K - 1): the fill runs into the end of the piece; nx = 1, 2 have no
    # step inside [xf_lo, xf_hi] (the last stage's planes pass the box's end
    # before the fill is over), and their last chunk is padded
    for name in ("x1", "x2"):
        c = _forms(name)
        assert not any(_has(c, r, f) for r in ms.ROLES for f in ("z", "free")), name
        assert _has(c, "interior", "masked-fill") and _has(c, "interior", "left"), name
    c = _forms("x5")  # pieces of 2, 2 and 1 planes
    assert _has(c, "interior", "z") and _has(c, "interior", "left")
    # seg = U: seg + 2(K - 1) steps are whole chunks, nothing is padded
    c = _forms("x6")
    assert not any(_has(c, r, "left") for r in ms.ROLES) and _has(c, "interior", "z")
    # seg = U + 1: one step past a chunk, U - 1 padded steps
    c = _forms("x7")
    per_wave = 2 * 1  # tiles x pieces
    assert c[("interior", "left")] == (ms.U - 1) * per_wave * (ms.WY - 2)
    for name in ("x13-6", "x13-7"):
        c = _forms(name)
        assert _has(c, "interior", "z") and _has(c, "interior", "masked-fill") and _has(c, "interior", "left"), name


def test_step_counts_add_up():
    """Every piece runs whole chunks of U steps: seg + 2(K - 1) rounded up."""
    for name, (n, L) in ms.SHAPES.items():
        c = ms.classify(n, L)
        seg = min(L, n[0])
        steps = 0
        for xs in range(-(-n[0] // seg)):
            ln = min(seg, n[0] - xs * seg)
            steps += -(-(ln + 2 * (ms.K - 1)) // ms.U) * ms.U
        tiles = -(-n[1] // ms.YS) * -(-n[2] // ms.ZS)
        assert sum(c.values()) == steps * tiles * ms.WY, name
