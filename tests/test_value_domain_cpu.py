"""The CPU rows over IEEE's whole value domain, tied to exact arithmetic.

The CPU backend is the oracle of every GPU test; utils/fma.py, the oracle of
the CPU backend, is valid for finite operands without overflow and says nothing
about underflow.  Here one step of the CPU rows (uniform, with a source, with a
conductivity, behind six convective walls) is compared bit for bit with an
exact rational evaluation of kernels.hpp's operation order, one
round-to-nearest-even per fma, add and multiply, subnormals, signed zeros, Inf
and NaN included, on the value classes of tests/_value_fields.py; the residual
must be the exact maximum.  Also: the Inf / NaN sets against a numpy evaluation
in a wider format, the negation identity, utils/fma.py against the exact
reference where both are valid, the input conditions of every class, and the
pair kernel's compiled variants against the specs the GPU tests launch."""
import math
import os
import re
import struct
from fractions import Fraction

import numpy as np
import pytest
import torch

import _lean_variants as lv
import _value_fields as vf

D = (0.06, 0.05, 0.04)
N = (3, 4, 5)
DTYPES = [torch.float64, torch.float32]
NP = {torch.float64: np.float64, torch.float32: np.float32}
BETA = (0.5, 0.3, 1.0, 0.125, 0.7, 0.9)  # a coefficient per face (exact in fp32 and not)
FORMS = ("plain", "source", "conductivity", "convective")
DBL_MIN = 2.2250738585072014e-308  # the residual slot's initial value (kResidualInitBits)


# ---- exact arithmetic

def rne(x, p, emin):
    """The positive Fraction x rounded to nearest, ties to even, in the binary
    format of p significand bits and smallest normal exponent emin (subnormals
    included), as a Fraction; math.inf on overflow."""
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1  # 2^e <= x < 2^(e + 1)
    q = Fraction(2) ** (max(e, emin) - (p - 1))  # the spacing of the format at x
    n = x // q
    rem = x - n * q
    if 2 * rem > q or (2 * rem == q and n & 1):
        n += 1
    y = n * q
    return math.inf if y >= Fraction(2) ** (1 - emin + 1) else y


class Exact:
    """fma, add, sub and mul of one dtype on Python floats that hold values of
    that dtype: the exact rational result rounded once; IEEE's rules for
    non-finite operands and for the sign of a zero result."""

    def __init__(self, dtype):
        self.f64 = dtype == torch.float64

    def round(self, x, zero_sign=1.0):
        if x == 0:
            return math.copysign(0.0, zero_sign)
        if self.f64:
            try:
                return float(x)  # correctly rounded, subnormals included
            except OverflowError:
                return math.inf if x > 0 else -math.inf
        y = float(rne(abs(x), 24, -126))  # exact: fp32 values are doubles
        return -y if x < 0 else y

    def fma(self, a, b, c):
        if not (math.isfinite(a) and math.isfinite(b)):
            return (math.nan if a == 0 or b == 0 else a * b) + c
        if not math.isfinite(c):
            return c
        x = Fraction(a) * Fraction(b) + Fraction(c)
        sp = math.copysign(1.0, a) * math.copysign(1.0, b)
        # an exact zero: -0 only as (-0) + (-0), an exact cancellation gives +0
        neg = (a == 0 or b == 0) and c == 0 and sp < 0 and math.copysign(1.0, c) < 0
        return self.round(x, -1.0 if neg else 1.0)

    def add(self, a, b):
        if not (math.isfinite(a) and math.isfinite(b)):
            return a + b
        neg = a == 0 and b == 0 and math.copysign(1.0, a) < 0 and math.copysign(1.0, b) < 0
        return self.round(Fraction(a) + Fraction(b), -1.0 if neg else 1.0)

    def sub(self, a, b):
        return self.add(a, -b)

    def mul(self, a, b):
        if not (math.isfinite(a) and math.isfinite(b)):
            return math.nan if a == 0 or b == 0 else a * b
        return self.round(Fraction(a) * Fraction(b), math.copysign(1.0, a) * math.copysign(1.0, b))


_OFF = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))  # x-, x+, y-, y+, z-, z+


def exact_step(dtype, T, S=None, Ch=None, beta=None, tinf=0.0):
    """One step on the ghosted array T in kernels.hpp's operation order
    (ftcs_update / ftcs_update_src / ftcs_update_var with var_flux;
    convective_ghost behind the walls of `beta`, six coefficients): the new
    interior and the residual as the state slot reports it."""
    A = Exact(dtype)
    npdt = NP[dtype]
    Dr = [float(npdt(d)) for d in D]
    n = tuple(e - 2 for e in T.shape)
    out = np.zeros(n, dtype=npdt)
    res, nan = 0.0, False
    for i in range(1, n[0] + 1):
        for j in range(1, n[1] + 1):
            for k in range(1, n[2] + 1):
                at = (i, j, k)
                c = float(T[at])
                nb = [float(T[i + o[0], j + o[1], k + o[2]]) for o in _OFF]
                if beta is not None:
                    d = A.sub(tinf, c)
                    for f in range(6):
                        a, e = divmod(f, 2)
                        if at[a] == (n[a] if e else 1):
                            nb[f] = A.fma(beta[f], d, c)  # convective_ghost
                acc = c
                for a in range(3):
                    m, p = nb[2 * a], nb[2 * a + 1]
                    if Ch is None:
                        t = A.add(A.fma(-2.0, c, p), m)
                    else:
                        hc = float(Ch[at])
                        hm, hp = (float(Ch[i + o[0], j + o[1], k + o[2]]) for o in _OFF[2 * a:2 * a + 2])
                        t = A.fma(A.add(hc, hp), A.sub(p, c), A.mul(A.add(hc, hm), A.sub(m, c)))  # var_flux
                    acc = A.fma(Dr[a], t, acc)
                if S is not None:
                    acc = A.add(acc, float(S[i - 1, j - 1, k - 1]))
                out[i - 1, j - 1, k - 1] = acc
                r = abs(A.sub(acc, c))
                nan |= r != r
                res = max(res, r) if r == r else res
    return out, (math.nan if nan else max(res, DBL_MIN))


# ---- the CPU backend's single step

def _inputs(ops, cls, dtype, form, T=None):
    T = vf.field(ops, cls, N, dtype, 1) if T is None else T
    cls = "signed" if cls.startswith("spike") else cls
    S = vf.source(ops, cls, N, dtype, 3) if form == "source" else None
    C = vf.conductivity(ops, N, dtype, 2) if form == "conductivity" else None
    beta = [float(NP[dtype](b)) for b in BETA] if form == "convective" else None
    tinf = 0.75 * vf.scale(cls, dtype)
    return T, S, C, beta, tinf


def _cpu_step(ops, T, S, C, beta, tinf):
    out = ops.PaddedField(T.n, dtype=T.dtype)
    st = ops.new_state("cpu")
    kw = {}
    if beta is not None:
        kw = dict(walls=ops.wall_coords(63, T.n), conv=list(BETA), ambient=tinf)
    ops.ftcs_step(T, out, D, state=st, source=S, conductivity=C, **kw)
    return out.owned().clone(), ops.residual_from_state(st, 0)


def _exact(dtype, T, S, C, beta, tinf):
    new, res = exact_step(dtype, T.ghosted().numpy(), S.owned().numpy() if S else None,
                          C.ghosted().numpy() if C else None, beta, float(NP[dtype](tinf)))
    return torch.from_numpy(new), res


def _same_residual(got, want):
    return (got != got and want != want) or struct.pack("<d", got) == struct.pack("<d", want)


# ---- tests

@pytest.mark.parametrize("p,emin,npdt", [(24, -126, np.float32), (53, -1022, np.float64)])
def test_rounding_helper(p, emin, npdt):
    """rne against numpy / struct: exactly representable values stay, the
    halfway cases around the smallest normal and the smallest subnormal go to
    even, and random rationals round as numpy rounds them (fp32 from exact
    doubles; fp64 as float(Fraction))."""
    tiny, sub = Fraction(2) ** emin, Fraction(2) ** (emin - (p - 1))
    for v in (tiny, sub, tiny - sub, tiny + sub, 3 * sub, Fraction(3, 2), Fraction(2) ** (p - 1) + 1, 1 - Fraction(2) ** -p):
        assert rne(v, p, emin) == v and float(npdt(float(v))) == float(v), v
    # halfway cases: ties to even
    assert rne(sub / 2, p, emin) == 0 and rne(3 * sub / 2, p, emin) == 2 * sub and rne(5 * sub / 2, p, emin) == 2 * sub
    assert rne(sub / 2 + sub / 1024, p, emin) == sub and rne(sub / 2 - sub / 1024, p, emin) == 0
    assert rne(tiny - sub / 2, p, emin) == tiny  # the largest subnormal is odd: up to the smallest normal
    assert rne(tiny + sub / 2, p, emin) == tiny and rne(tiny + 3 * sub / 2, p, emin) == tiny + 2 * sub
    assert rne(tiny - 3 * sub / 2, p, emin) == tiny - 2 * sub
    big = (2 - Fraction(2) ** (1 - p)) * Fraction(2) ** (-emin + 1)  # the largest finite value
    assert rne(big, p, emin) == big and rne(big + big / 2 ** (p + 2), p, emin) == big
    assert rne(big + Fraction(2) ** (-emin + 1 - p), p, emin) == math.inf
    rng = np.random.default_rng(0)
    for _ in range(400):
        e = int(rng.integers(emin - p - 2, emin + 8))
        # fp32: 40-bit numerators, exact as doubles, which numpy then rounds once
        x = Fraction(int(rng.integers(1, 2 ** (62 if p == 53 else 40))), 2 ** 39) * Fraction(2) ** e
        want = float(x) if p == 53 else float(np.float32(float(x)))
        assert float(rne(x, p, emin)) == want, x
    if p == 24:  # the fp32 halfway cases through struct as well
        for v, want in ((tiny - sub / 2, tiny), (3 * sub / 2, 2 * sub)):
            assert struct.unpack("<f", struct.pack("<f", float(v)))[0] == float(want)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cls", vf.FINITE_CLASSES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_step_is_exact(h3d, dtype, cls, form):
    """ops.ftcs_step on host fields == the exact reference, field and residual."""
    ops = h3d.ops
    args = _inputs(ops, cls, dtype, form)
    got, res = _cpu_step(ops, *args)
    want, wres = _exact(dtype, *args)
    print(f"{cls} {dtype} {form}: {vf.conditions(cls, got) if form in ('plain', 'source') else vf.shares(got)}")
    assert vf.same_bits(got, want)
    assert _same_residual(res, wres), (res, wres)


SPECIAL = ["huge", "zeros+", "zeros-"] + [f"spike:{kind}:{pos}" for kind in vf.KINDS
                                         for pos in ((1, 2, 2), (0, 0, 0), (2, 3, 4), (-1, 1, 1), (1, 2, 5))]


def _special_field(ops, cls, dtype):
    if not cls.startswith("spike"):
        return vf.field(ops, cls, N, dtype, 1)
    _, kind, pos = cls.split(":")
    return vf.spike(ops, kind, tuple(int(v) for v in pos.strip("()").split(",")), N, dtype, 1)


def _wide_step(dtype, T, S, Ch, beta, tinf):
    """The same operation order in numpy, every operation carried out in the
    next wider format (fp64 for fp32, the 80-bit long double for fp64) and then
    rounded to the dtype: the Inf / NaN rules are numpy's, and no product or
    sum overflows before its single rounding, as in a fused multiply-add."""
    W, dt = (np.longdouble, np.float64) if dtype == torch.float64 else (np.float64, np.float32)
    assert np.finfo(W).maxexp > np.finfo(dt).maxexp and np.finfo(W).nmant > np.finfo(dt).nmant
    r = lambda x: x.astype(dt).astype(W)  # noqa: E731
    fma = lambda a, b, c: r(a * b + c)  # noqa: E731
    T = T.astype(W)
    n = tuple(e - 2 for e in T.shape)
    core = (slice(1, -1),) * 3
    shift = lambda F, o: F[tuple(slice(1 + v, F.shape[a] - 1 + v) for a, v in enumerate(o))]  # noqa: E731
    c = T[core]
    nb = [shift(T, o).copy() for o in _OFF]
    if beta is not None:
        d = r(W(dt(tinf)) - c)
        for f in range(6):
            a, e = divmod(f, 2)
            wall = [slice(None)] * 3
            wall[a] = n[a] - 1 if e else 0
            nb[f][tuple(wall)] = fma(W(dt(BETA[f])), d, c)[tuple(wall)]
    acc = c
    for a in range(3):
        m, p = nb[2 * a], nb[2 * a + 1]
        if Ch is None:
            t = r(fma(W(-2), c, p) + m)
        else:
            h = Ch.astype(W)
            t = fma(r(h[core] + shift(h, _OFF[2 * a + 1])), r(p - c), r(r(h[core] + shift(h, _OFF[2 * a])) * r(m - c)))
        acc = fma(W(dt(D[a])), t, acc)
    if S is not None:
        acc = r(acc + S.astype(W))
    return acc.astype(dt)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cls", SPECIAL)
@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_step_special_values(h3d, dtype, cls, form):
    """Overflow, signed zeros and a single NaN / Inf (centre, corners, ghosts):
    the NaN set and the Inf set of the CPU's output are those of the numpy
    evaluation in a wider format, and every bit is the exact reference's, which
    follows IEEE's rules for non-finite operands and zero signs."""
    ops = h3d.ops
    T, S, C, beta, tinf = _inputs(ops, cls, dtype, form, _special_field(ops, cls, dtype))
    if cls.startswith("zeros"):
        tinf, S = 0.0, (vf.source(ops, cls, N, dtype, 3) if S else None)
    got, res = _cpu_step(ops, T, S, C, beta, tinf)
    with np.errstate(all="ignore"):
        ref = torch.from_numpy(_wide_step(dtype, T.ghosted().numpy(), S.owned().numpy() if S else None,
                                          C.ghosted().numpy() if C else None, beta, tinf))
    assert torch.equal(got.isnan(), ref.isnan()) and torch.equal(got.isinf(), ref.isinf())
    want, wres = _exact(dtype, T, S, C, beta, tinf)
    assert vf.same_bits(got, want)
    assert _same_residual(res, wres), (res, wres)
    s = vf.conditions(cls, got) if form in ("plain", "source") else vf.shares(got)
    if cls == "huge":
        print(f"huge {dtype} {form}: {s}")
    elif cls.startswith("spike"):
        if form == "convective" and T.owned().isfinite().all():
            # a ghost behind a wall is never read: convective_ghost of the first interior point stands for it
            assert s["nan"] == 0 and s["inf"] == 0 and res == res and res < math.inf
        else:
            assert s["nan"] > 0 or s["inf"] > 0  # the bad value reached the stored box
            assert res != res or res == math.inf
    else:
        # zeros in, zeros out: +0 from +0; from -0, fma(-2, -0, -0) = (+0) + (-0) = +0 and so on: +0
        # (behind convective walls too: the ambient is +0)
        assert (got == 0).all() and not torch.signbit(got).any() and res == DBL_MIN
        zero_in = torch.signbit(T.owned()).all() if cls == "zeros-" else not torch.signbit(T.owned()).any()
        assert zero_in


def _deep_case(ops, cls, dtype, K, form, negate=False):
    """A K-step sweep3 of the CPU backend on (5, 6, 7) with K-deep ghosts and
    the update ranges widened into them."""
    n, g = (5, 6, 7), (K, K, K)
    T = vf.field(ops, cls, n, dtype, 4, g)
    S = vf.source(ops, cls, n, dtype, 5, g) if form == "source" else None
    C = vf.conductivity(ops, n, dtype, 6, g) if form == "conductivity" else None
    walls = conv = None
    tinf = 0.75 * vf.scale(cls, dtype)
    u = sum(([-(K - 1), e + K - 1] for e in n), [])
    if form == "convective":
        walls, conv, u = ops.wall_coords(63, n), list(BETA), (0, -1) * 3
    if negate:
        T, S, tinf = vf.negated(ops, T), vf.negated(ops, S) if S else None, -tinf
    out = ops.PaddedField(n, dtype=dtype, gx=K, gy=K, gz=K)
    st = ops.new_state("cpu")
    ops.sweep3(T, out, D, (0, n[0], 0, n[1], 0, n[2]), u, kernel=f"tl{K}", state=st, source=S, conductivity=C,
               walls=walls, conv=conv, ambient=tinf)
    return out.owned().clone(), [ops.residual_from_state(st, s) for s in range(K)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cls", vf.FINITE_CLASSES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_negation_identity(h3d, dtype, cls, form):
    """step(-T, -S) == -step(T, S) bit for bit (round-to-nearest is
    sign-symmetric), K = 1 and a K = 3 sweep3; the ambient is negated with the
    field, Ch and beta are not."""
    ops = h3d.ops
    T, S, C, beta, tinf = _inputs(ops, cls, dtype, form)
    a, ra = _cpu_step(ops, T, S, C, beta, tinf)
    b, rb = _cpu_step(ops, vf.negated(ops, T), vf.negated(ops, S) if S else None, C, beta, -tinf)
    assert vf.same_bits(b, -a) and ra == rb
    a, ra = _deep_case(ops, cls, dtype, 3, form)
    b, rb = _deep_case(ops, cls, dtype, 3, form, negate=True)
    assert vf.same_bits(b, -a) and ra == rb and (a != 0).any()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cls", ["signed", "wide"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_oracles_agree(h3d, dtype, cls, form):
    """Where both are valid, utils/fma.py's ftcs_reference gives the bits and
    the residual of the exact reference."""
    ops = h3d.ops
    T, S, C, beta, tinf = _inputs(ops, cls, dtype, form)
    new, res = ops.ftcs_reference(T.ghosted().clone(), D, src=S.owned() if S else None,
                                  cond=C.ghosted() if C else None, convective=list(BETA) if beta else None, ambient=tinf)
    want, wres = _exact(dtype, T, S, C, beta, tinf)
    assert vf.same_bits(new.contiguous(), want)
    assert max(res, DBL_MIN) == wres


@pytest.mark.parametrize("cls", vf.FINITE_CLASSES + ("huge",))
@pytest.mark.parametrize("dtype", DTYPES)
def test_input_conditions(h3d, dtype, cls):
    """Every class does what it is for on the CPU rows' output alone, on the
    boxes and depths of both test modules, with and without a source; the
    measured shares of subnormal, NaN and Inf values are printed."""
    ops = h3d.ops
    for n, depths in (((3, 4, 5), (1,)), ((5, 3, 64), (1,)), ((9, 13, 130), (1,)), ((9, 50, 130), (2, 3, 4))):
        for K in depths:
            for with_source in (False, True):
                T = vf.field(ops, cls, n, dtype, 1, K=K)
                S = vf.source(ops, cls, n, dtype, 3, K=K) if with_source else None
                out = ops.PaddedField(n, dtype=dtype)
                if K == 1:
                    ops.ftcs_step(T, out, D, source=S)
                else:
                    ops.sweep3(T, out, D, (0, n[0], 0, n[1], 0, n[2]), (0, -1) * 3, kernel=f"tl{K}", source=S)
                s = vf.conditions(cls, out.owned())
                print(f"{cls} {dtype} n={n} K={K} source={with_source}: subnormal {s['subnormal']:.3f} "
                      f"nan {s['nan']:.3f} inf {s['inf']:.3f}")


def test_same_bits_reports():
    a = torch.tensor([0.0, float("nan"), 1.0, 2.0 ** -140], dtype=torch.float32)
    b = a.clone()
    b[1] = -float("nan")
    assert vf.same_bits(a, b)  # payload and sign of a NaN are not compared
    for i, v in ((0, -0.0), (3, 0.0), (2, float("nan")), (1, 1.0)):
        c = a.clone()
        c[i] = v
        with pytest.raises(AssertionError, match=rf"1 of 4 differ, first at \({i},\)"):
            vf.same_bits(c, a)


# ---- the pair kernel's compiled variants

_TBP = re.compile(r"H3D_TBP\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*([^()]*?)\s*\)")


def compiled_pair_variants():
    """(dtype, R, WY, K, Q, store bits) of every H3D_TBP(...) line of
    stencil_tbp.hip, in the order of the dispatch chain."""
    with open(os.path.join(lv.KERNELS, "stencil_tbp.hip")) as f:
        text = f.read()
    body = text[text.index("#define H3D_TBP"):text.index("#undef H3D_TBP")]
    body = body[body.index("if constexpr (sizeof(T) == 4)"):]
    f32, f64 = body.split("} else {")
    out = []
    for dtype, part in (("fp32", f32), ("fp64", f64)):
        for m in _TBP.finditer(part):
            bits = eval(m.group(5), {"__builtins__": {}}, {"kResidualLastOnly": lv.LAST_ONLY})
            out.append((dtype, *(int(m.group(i)) for i in range(1, 5)), bits))
    assert len(out) == body.count("H3D_TBP(") and len(set(out)) == len(out)
    return out


def test_every_compiled_pair_variant_is_launched(ext):
    """Every pair variant that stencil_tbp.hip compiles is selected by a spec
    of test_gpu_temporal's PAIR / PAIR_F64 lists (resolved as the dispatch
    resolves it, first match of the chain), so none goes unlaunched."""
    import test_gpu_temporal as tt

    compiled = compiled_pair_variants()
    launched = set()
    for dtype, lists in (("fp32", tt.PAIR), ("fp64", tt.PAIR_F64)):
        for spec in sum(lists.values(), []):
            r = ext.kernel_spec_resolved(spec, dtype).split(":")
            assert r[1] == "2", (spec, r)
            K, R, WY, Q = int(r[0][2]), int(r[2]), int(r[4]), int(r[6])
            store = int(r[7]) if len(r) > 7 else -1
            hit = next((v for v in compiled if v[:5] == (dtype, R, WY, K, Q)
                        and (v[5] == store or (v[5] == 0 and store <= 0))), None)
            assert hit is not None and ext.lean_supported(dtype, spec, False), (dtype, spec)
            launched.add(hit)
    missing = [v for v in compiled if v not in launched]
    print(f"pair variants compiled: {len(compiled)}, launched: {len(launched)}")
    assert not missing, missing
