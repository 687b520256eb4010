"""Value classes for the kernels' inputs and a NaN-aware bit compare.

Every other test feeds the kernels uniform values in [0, 1); the classes here
cover the rest of IEEE's value domain: both signs, a wide exponent range with
heavy cancellation, the subnormal range, overflow into Inf and NaN, signed
zeros, and a single NaN / Inf at a chosen place.  tests/test_value_domain_cpu.py
ties the CPU rows to exact arithmetic on them, tests/test_gpu_value_domain.py
the gfx950 kernels to the CPU rows."""
import torch

INT = {torch.float64: torch.int64, torch.float32: torch.int32}
# exponent of the smallest normal number
EMIN = {torch.float64: -1022, torch.float32: -126}

# Scale exponents, tuned on the CPU rows until their output alone meets
# `conditions` on every box of both test modules (one step on (3, 4, 5) up to
# four steps on (9, 50, 130)); the shares are printed by test_value_domain_cpu.
#   subnormal_edge: 2^(EMIN + 2): a quarter of the inputs and a third or more of the results are subnormal
#   subnormal:      2^(EMIN - 14): every input and every result is subnormal or zero
#   wide:           m 2^e, |e| <= 60 (fp32) / 500 (fp64): no overflow, no underflow in four steps
#   huge:           0.9 of the largest finite value for one step (fma(-2, c, xp) + xm overflows at four
#                   points in five and Inf - Inf follows in the fma chain), 0.45 for two steps and 0.3 for
#                   three and four: a deeper sweep at 0.9 leaves no finite value in the box
SUBNORMAL_EDGE_EXP = {torch.float32: -124, torch.float64: -1020}
SUBNORMAL_EXP = {torch.float32: -140, torch.float64: -1060}
WIDE_EXP = {torch.float32: 60, torch.float64: 500}
HUGE_FACTOR = {1: 0.9, 2: 0.45, 3: 0.3, 4: 0.3}

FINITE_CLASSES = ("signed", "wide", "subnormal_edge", "subnormal")
CLASSES = FINITE_CLASSES + ("huge", "zeros+", "zeros-")
KINDS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


def _describe(t, i):
    v = t[i]
    width = 16 if t.dtype == torch.float64 else 8
    mask = (1 << (4 * width)) - 1
    return f"{v.item()!r} (0x{int(v.view(INT[t.dtype]).item()) & mask:0{width}x})"


def bits_differ(got, want):
    """None if the tensors have the same bits, NaNs taken as equal to each
    other (payload and sign of a NaN are not compared: x86 and gfx950 produce
    different default NaNs); else the report: the count and the first differing
    index with both values and both bit patterns."""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    got, want = got.contiguous(), want.contiguous()
    gn, wn = got.isnan(), want.isnan()
    bad = (gn != wn) | (~gn & ~wn & (got.view(INT[got.dtype]) != want.view(INT[want.dtype])))
    if not bad.any():
        return None
    where = bad.nonzero()
    i = tuple(int(v) for v in where[0])
    return f"{len(where)} of {bad.numel()} differ, first at {i}: got {_describe(got, i)}, want {_describe(want, i)}"


def same_bits(got, want):
    """True if equal in the sense of bits_differ (signed zeros and subnormals
    are distinguished); otherwise an AssertionError with its report."""
    report = bits_differ(got, want)
    if report is not None:
        raise AssertionError(report)
    return True


def scale(cls, dtype, K=1):
    """The magnitude of a class's values: what a source or an ambient
    temperature for a field of that class is scaled by."""
    if cls == "subnormal_edge":
        return 2.0 ** SUBNORMAL_EDGE_EXP[dtype]
    if cls == "subnormal":
        return 2.0 ** SUBNORMAL_EXP[dtype]
    if cls == "huge":
        return HUGE_FACTOR[K] * torch.finfo(dtype).max
    return 0.0 if cls.startswith("zeros") else 1.0


def values(cls, shape, dtype, seed, K=1):
    """A tensor of `shape` of the class `cls`, seeded; drawn in fp64 and
    rounded once to `dtype` (2^e scalings are exact or round into the
    subnormal grid)."""
    gen = torch.Generator().manual_seed(seed)
    signed = 2.0 * torch.rand(shape, generator=gen, dtype=torch.float64) - 1.0
    if cls == "signed" or cls.startswith("spike"):
        v = signed
    elif cls == "wide":
        e = torch.randint(-WIDE_EXP[dtype], WIDE_EXP[dtype] + 1, shape, generator=gen)
        m = 1.0 + torch.rand(shape, generator=gen, dtype=torch.float64)
        v = torch.ldexp(torch.where(signed < 0, -m, m), e)
    elif cls in ("subnormal_edge", "subnormal", "huge"):
        v = signed * scale(cls, dtype, K)
    elif cls == "zeros+":
        v = torch.zeros(shape, dtype=torch.float64)
    elif cls == "zeros-":
        v = -torch.zeros(shape, dtype=torch.float64)
    else:
        raise ValueError(cls)
    return v.to(dtype)


def field(ops, cls, n, dtype, seed, g=(1, 1, 1), K=1, factor=1.0):
    """A host PaddedField of the class on every ghost layer, for K steps
    (`huge` only), times `factor` (a power of two)."""
    f = ops.PaddedField(n, dtype=dtype, gx=g[0], gy=g[1], gz=g[2])
    f.deep3().copy_(values(cls, f.deep3().shape, dtype, seed, K) * factor)
    return f


def source(ops, cls, n, dtype, seed, g=(1, 1, 1), K=1):
    """A heat source S for a field of the class: the class's values at a
    quarter of the field's scale (K <= 4 steps of it stay in the field's range)."""
    return field(ops, "signed" if cls.startswith("spike") else cls, n, dtype, seed, g, K, 0.25)


def spike(ops, kind, pos, n, dtype, seed, g=(1, 1, 1)):
    """A `signed` background with exactly one element set to `kind` (a key of
    KINDS) at the owned coordinates `pos`; ghost positions (-g .. n + g - 1) are
    allowed."""
    f = field(ops, "signed", n, dtype, seed, g)
    at = tuple(p + h for p, h in zip(pos, g))
    assert all(0 <= a < e for a, e in zip(at, f.deep3().shape)), (pos, n, g)
    f.deep3()[at] = KINDS[kind]
    return f


def conductivity(ops, n, dtype, seed, g=(1, 1, 1)):
    """Ch = dtype(0.5 c), c uniform in [0.05, 1]: a material property, the same
    for every value class."""
    gen = torch.Generator().manual_seed(seed)
    f = ops.PaddedField(n, dtype=dtype, gx=g[0], gy=g[1], gz=g[2])
    v = f.deep3()
    v.copy_((0.5 * (0.05 + 0.95 * torch.rand(v.shape, generator=gen, dtype=torch.float64))).to(dtype))
    return f


def negated(ops, f):
    """The field with every sign flipped, signed zeros and ghosts included."""
    out = ops.PaddedField(f.n, dtype=f.dtype, gx=f.gx, gy=f.gy, gz=f.gz)
    out.flat.copy_(-f.flat)
    return out


def shares(stored):
    """Shares of nonzero subnormals, NaNs and Infs among stored values, and
    whether a normal and a finite value are among them."""
    tiny = torch.finfo(stored.dtype).tiny
    mag = stored.abs()
    n = stored.numel()
    return {"subnormal": float(((mag > 0) & (mag < tiny)).sum()) / n, "nan": float(stored.isnan().sum()) / n,
            "inf": float(stored.isinf().sum()) / n, "normal": bool(((mag >= tiny) & stored.isfinite()).any()),
            "finite": bool(stored.isfinite().any()), "nonzero": bool((stored != 0).any())}


def conditions(cls, stored, need_nan=True):
    """Asserts that a class did what it is for, on values the CPU reference
    stored (never on the GPU's, so that no test passes vacuously); returns the
    measured shares.  need_nan=False: one step with a conductivity, which turns
    finite values into Inf but never into NaN (both terms of an axis's flux, and
    the fluxes of all axes, overflow with the sign of -c), so NaN needs a second step."""
    s = shares(stored)
    if cls == "subnormal_edge":
        assert s["subnormal"] >= 0.25 and s["normal"], s
    elif cls == "subnormal":
        assert s["subnormal"] >= 0.5, s
    elif cls == "huge":
        assert (s["nan"] > 0 or not need_nan) and s["inf"] > 0 and s["finite"], s
    elif cls in ("wide", "signed"):
        assert s["nan"] == 0 and s["inf"] == 0 and s["subnormal"] == 0, s
    return s
