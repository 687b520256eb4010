"""Every gfx950 kernel family on IEEE's whole value domain, bit for bit.

The oracle is the CPU backend on host fields through the same ops entry point
(tests/test_value_domain_cpu.py ties it to exact arithmetic on the same value
classes); a sentinel-filled destination, the whole flat buffer compared with
_value_fields.same_bits, no tolerances.  One spec per family (the ones the solver
picks plus the variants with mask logic of their own), two boxes per spec:

a. every value class (both signs, wide exponents, the subnormal range, overflow
   into Inf and NaN, signed zeros), field and residual slots;
b. kernel(-T) == -kernel(T) on the GPU alone;
c. one NaN / +Inf / -Inf at a time, at tile seams, in either half of a pair
   lane, in a masked tail, on a Dirichlet ghost, inside a deep halo: the field,
   the NaN rule of the residual slots and the fault flag of the check;
d. the solver's fault from a NaN at any position, iteration for iteration the
   CPU backend's;
e. a body cooling through convective walls until the whole field is subnormal.

"Fault" is the solver's numerical flag (DeviceState::fault == 1): NaN and Inf
are values in ordinary, in-bounds arrays."""
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

import _lean_variants as lv
import _value_fields as vf

pytestmark = pytest.mark.gpu

D = (0.06, 0.05, 0.04)
SENTINEL = -5.0
TORCH = {"fp64": torch.float64, "fp32": torch.float32}
BETA = (0.5, 0.3, 1.0, 0.125, 0.7, 0.9)  # mixed coefficients, one per face
MASKED = (9, 50, 130)  # a masked z tail, two y tiles for every tile height in use, fewer planes than one chunk
NO_U = (0, -1, 0, -1, 0, -1)

# spec: the kernel string; wall: None, "ins" (mask 63) or "conv" (six faces, BETA); n / g / box / u: a layout of
# its own (the thin-slab forms) instead of the masked and the free box
Case = namedtuple("Case", "id spec dtypes src wall cond layout", defaults=(False, None, False, None))
BOTH = ("fp64", "fp32")

SINGLE = [Case(f"{k}{'-src' if s else ''}", k, BOTH, src=s) for k in ("naive", "tile") for s in (False, True)]
SINGLE += [Case(f"var{'-src' if s else ''}", "tile", BOTH, src=s, cond=True) for s in (False, True)]
SWEEPS = [
    Case("tl2", "tl2", BOTH), Case("tl3", "tl3", BOTH), Case("tl4", "tl4", BOTH),
    Case("lean-last-only", "tl3:1:3:1:16:0:3:66", ("fp64",)),
    Case("lean-edge-role", "tl4:1:4:1:12:0:3:66:0:3", ("fp64",)),
    # the y-marching thin-slab forms, picked by box shape under a default spec
    Case("thin-slab-k3", "tl3", BOTH, layout=((4, 70, 70), (1, 1, 1), (0, 4, 0, 70, 0, 70), NO_U)),
    Case("thin-slab-k4", "tl4", BOTH, layout=((12, 64, 133), (4, 1, 1), (0, 4, 0, 64, 0, 133), (-3, 15, 0, -1, 0, -1))),
    Case("pair-f32", "tl3:2:3:1:16:0:3", ("fp32",)), Case("pair-f32-last-only", "tl3:2:3:1:16:0:3:66", ("fp32",)),
    Case("pair-f32-k4-last-only", "tl4:2:2:1:16:0:3:64", ("fp32",)),
    Case("pair-f64", "tl3:2", ("fp64",)), Case("pair-f64-last-only", "tl3:2:4:1:8:0:3:66", ("fp64",)),
    Case("tl3-src", "tl3", BOTH, src=True), Case("tl3-ins", "tl3", BOTH, wall="ins"),
    Case("tl3-conv", "tl3", BOTH, wall="conv"), Case("tl3-ins-src", "tl3", BOTH, src=True, wall="ins"),
    Case("tl3-conv-src", "tl3", BOTH, src=True, wall="conv"),
]
for _k in ("tv2", "tv3"):
    SWEEPS += [Case(_k, _k, BOTH, cond=True), Case(f"{_k}-ins", _k, BOTH, wall="ins", cond=True),
               Case(f"{_k}-conv", _k, BOTH, wall="conv", cond=True), Case(f"{_k}-src", _k, BOTH, src=True, cond=True)]
CASES = SINGLE + SWEEPS
ITEMS = [pytest.param(c, dt, id=f"{c.id}-{dt}") for c in CASES for dt in c.dtypes]


def _depth(c):
    return int(c.spec.split(":")[0][2]) if c in SWEEPS else 1


def _last_only(c):
    f = c.spec.split(":")
    return len(f) > 7 and bool(int(f[7]) & lv.LAST_ONLY)


def _slots(c):
    """The residual slots the variant computes."""
    K = _depth(c)
    return range(K - 1 if _last_only(c) else 0, K)


def _geometry(ext, c, dt):
    """(stored rows YS, stored columns ZS, x unroll U, pair) of the tile that runs the case."""
    K = _depth(c)
    wall = {None: 0, "ins": 1, "conv": 2}[c.wall]
    if c.cond:
        R, WY = ext.cond_sweep_shape(dt, c.spec, c.src, wall)
        return R * WY - 2 * K, 64 - 2 * K, 6, False
    r = ext.kernel_spec_resolved(c.spec, dt).split(":")
    if r[1] == "2" and not c.wall:  # packed pairs (with walls an unset V means 1)
        return int(r[4]) * int(r[2]) - 2 * K, 128 - 2 * K - 2, 12 if int(r[6]) == 4 else 6, True
    shape = ext.lean_shape(dt, c.spec, c.src, wall)
    assert shape is not None, (c.spec, dt)
    EW = int(r[9]) if len(r) > 9 else 0
    v = lv.Variant(dt, shape[0], shape[1], K, int(r[6]), 0, False, EW, c.src)
    _, YS, ZS, U = lv.geometry(v)
    return YS, ZS, U, False


def _pinned(ext, c, dt, ZS):
    """The spec with the z stride (field 8) pinned where the spec has the
    field, so that seams are where the boxes put them; default specs (which the
    thin-slab rule and the wall forms need) stay as they are."""
    f = c.spec.split(":")
    if len(f) < 7 or c.cond:
        return c.spec
    if len(f) < 8:
        # no store field: the resolved spec names the default store policy
        r = ext.kernel_spec_resolved(c.spec, dt).split(":")
        f = r + (["0"] if len(r) < 8 else [])
    if len(f) == 8:
        f.append(str(ZS))
    else:
        f[8] = str(ZS)
    return ":".join(f)


def _layouts(ext, c, dt):
    """{name: (n, g, box, u)}: the masked and the free box of the case."""
    if c.layout:
        return {"thin": c.layout}
    if c in SINGLE:
        return {"masked": ((9, 13, 130), (1, 1, 1), None, None), "rows": ((5, 3, 64), (1, 1, 1), None, None)}
    K = _depth(c)
    YS, ZS, U, _ = _geometry(ext, c, dt)
    free = (2 * (K - 1) + U + 3, 3 * YS, 3 * ZS)
    whole = lambda n: (0, n[0], 0, n[1], 0, n[2])  # noqa: E731
    return {"masked": (MASKED, (1, 1, 1), whole(MASKED), NO_U), "free": (free, (1, 1, 1), whole(free), NO_U)}


def _to(ops, f, dev):
    if f is None:
        return None
    d = ops.PaddedField(f.n, dtype=f.dtype, device=dev, gx=f.gx, gy=f.gy, gz=f.gz)
    d.flat.copy_(f.flat)
    return d


def _launch(ops, c, spec, T, S, C, out, st, box, u, ambient):
    if c in SINGLE:
        ops.ftcs_step(T, out, D, kernel=spec, state=st, source=S, conductivity=C)
        return
    walls = ops.wall_coords(63, T.n) if c.wall else None
    conv = list(BETA) if c.wall == "conv" else None
    ops.sweep3(T, out, D, box, u, kernel=spec, state=st, source=S, conductivity=C, walls=walls, conv=conv,
               ambient=ambient if conv else 0.0)


def _cpu(ops, c, T, S, C, box, u, ambient):
    """The CPU definition: the whole destination buffer (sentinel outside the
    box), the stored box and the residual slots."""
    want = ops.PaddedField(T.n, dtype=T.dtype, gx=T.gx, gy=T.gy, gz=T.gz)
    want.flat.fill_(SENTINEL)
    st = ops.new_state("cpu")
    _launch(ops, c, c.spec.split(":")[0], T, S, C, want, st, box, u, ambient)
    b = box or (0, T.n[0], 0, T.n[1], 0, T.n[2])
    stored = want.owned()[b[0]:b[1], b[2]:b[3], b[4]:b[5]]
    return want.flat, stored, [ops.residual_from_state(st, s) for s in range(4)]


def _gpu(ops, gpu, c, spec, T, S, C, box, u, ambient):
    got = ops.PaddedField(T.n, dtype=T.dtype, device=gpu, gx=T.gx, gy=T.gy, gz=T.gz)
    got.flat.fill_(SENTINEL)
    st = ops.new_state(gpu)
    _launch(ops, c, spec, _to(ops, T, gpu), _to(ops, S, gpu), _to(ops, C, gpu), got, st, box, u, ambient)
    torch.cuda.synchronize()
    return got.flat.cpu(), [ops.residual_from_state(st, s) for s in range(4)], st


def _bits(x):
    return np.float64(x).view(np.uint64)


def _check_slots(c, stored, rc, rg, what):
    """The residual slots the variant computes.  Without a NaN in the stored
    box a slot is the CPU's bit for bit.  With one, every slot is NaN on the
    GPU (residual_commit_block poisons them all; the CPU's earlier slots may
    still be finite or Inf: the step at which the field blew up is not part of
    the contract, the fault is), and so is the CPU's last."""
    K = _depth(c)
    poisoned = bool(stored.isnan().any())
    assert math.isnan(rc[K - 1]) == poisoned, (what, rc)
    for s in _slots(c):
        if poisoned:
            assert math.isnan(rg[s]), f"{what}: slot {s} is {rg[s]!r} with a NaN in the stored box (CPU {rc[s]!r})"
        else:
            assert not math.isnan(rc[s]) and _bits(rg[s]) == _bits(rc[s]), f"{what}: slot {s}: {rg[s]!r}, CPU {rc[s]!r}"


def _inputs(ops, c, cls, n, dtype, g):
    K = _depth(c)
    T = vf.field(ops, cls, n, dtype, 1, g, K)
    S = vf.source(ops, cls, n, dtype, 3, g, K) if c.src else None
    C = vf.conductivity(ops, n, dtype, 2, g) if c.cond else None
    return T, S, C, 0.75 * vf.scale(cls, dtype, K)


@pytest.mark.parametrize("c,dt", ITEMS)
def test_value_class_bitwise(h3d, ext, gpu, c, dt):
    """a. Each value class on both boxes: the destination buffer (the stored
    box and the untouched sentinel elsewhere) and the residual slots."""
    ops, dtype = h3d.ops, TORCH[dt]
    for name, (n, g, box, u) in _layouts(ext, c, dt).items():
        spec = _pinned(ext, c, dt, _geometry(ext, c, dt)[1]) if c in SWEEPS and not c.layout else c.spec
        for cls in vf.CLASSES:
            T, S, C, ambient = _inputs(ops, c, cls, n, dtype, g)
            want, stored, rc = _cpu(ops, c, T, S, C, box, u, ambient)
            vf.conditions(cls, stored, need_nan=not (c.cond and c in SINGLE))
            got, rg, _ = _gpu(ops, gpu, c, spec, T, S, C, box, u, ambient)
            what = f"{c.id} {dt} {name} {n} {cls}"
            report = vf.bits_differ(got, want)
            assert report is None, f"{what} (flat index): {report}"
            _check_slots(c, stored, rc, rg, what)


@pytest.mark.parametrize("c,dt", ITEMS)
def test_negation_symmetry(h3d, ext, gpu, c, dt):
    """b. run(-T, -S) has the bits of -run(T, S) and equal residual slots, GPU
    against itself (round-to-nearest is sign-symmetric; an operand swap or a
    re-associated add is not).  The ambient is negated, Ch and beta are not."""
    ops, dtype = h3d.ops, TORCH[dt]
    n, g, box, u = next(iter(_layouts(ext, c, dt).values()))
    T, S, C, ambient = _inputs(ops, c, "signed", n, dtype, g)
    a, ra, _ = _gpu(ops, gpu, c, c.spec, T, S, C, box, u, ambient)
    b, rb, _ = _gpu(ops, gpu, c, c.spec, vf.negated(ops, T), vf.negated(ops, S) if S else None, C, box, u, -ambient)
    keep = a == SENTINEL  # the untouched rest of the destination keeps its sign
    assert keep.any() and not keep.all()
    report = vf.bits_differ(b, torch.where(keep, a, -a))
    assert report is None, f"{c.id} {dt}: {report}"
    assert [_bits(ra[s]) for s in _slots(c)] == [_bits(rb[s]) for s in _slots(c)], (ra, rb)


def _positions(ext, c, dt):
    """[(layout name, (n, g, box, u), position in owned coordinates)] for test c."""
    lay = _layouts(ext, c, dt)
    name, L = next(iter(lay.items()))
    n, g, box, u = L
    b = box or (0, n[0], 0, n[1], 0, n[2])
    x, y, z = (b[0] + b[1]) // 2, min(5, n[1] - 1), 7
    pos = [(b[0], 0, 0), (b[1] - 1, n[1] - 1, n[2] - 1),  # the first and the last stored point
           (b[0] - 1, y, z), (x, y, n[2])]                # Dirichlet ghosts (or a deep halo's first plane)
    out = [(name, L, p) for p in pos]
    if c in SINGLE or c.layout:
        return out + [(name, L, (x, n[1] // 2, n[2] // 2)), (name, L, (x, y, n[2] - 2))]
    K = _depth(c)
    YS, ZS, U, pair = _geometry(ext, c, dt)
    more = [(x, y, ZS - 1), (x, y, ZS)]                    # the z seam: last column of tile 0, first of tile 1
    if YS < n[1]:
        more += [(x, YS - 1, z), (x, YS, z)]               # the y seam
    more += [(x, y, n[2] - 3)]                             # the masked tail tile
    if pair:
        more += [(x, y, ZS - 2), (x, y, ZS + 1), (x, y, 0), (x, y, 1)]  # even and odd columns at a tile's ends
    if len(c.spec.split(":")) > 9:
        more += [(x, 1, z), (x, YS - 2, z)]                # rows owned by the edge waves
    out += [(name, L, p) for p in more]
    nf = lay["free"][0]                                    # the mask-free middle tile of the free box
    out.append(("free", lay["free"], (K - 1 + U // 2, YS + YS // 2, ZS + ZS // 2 + 1)))
    if not c.wall:
        # K-deep ghosts on every axis, the update ranges widened into them: a halo point at
        # distance K - 1 (computed, never stored) and one at distance K (read, never updated)
        deep = (n, (K, K, K), box, tuple(v for e in n for v in (-(K - 1), e + K - 1)))
        out += [("deep", deep, (-(K - 1), y, z)), ("deep", deep, (-K, y, z)), ("deep", deep, (x, y, n[2] + K - 2))]
    assert all(-gg <= q < e + gg for _, (nn, gs, _, _), p in out for q, e, gg in zip(p, nn, gs)), (nf, out)
    return out


@pytest.mark.parametrize("c,dt", ITEMS)
def test_one_bad_value_is_seen(h3d, ext, gpu, c, dt):
    """c. The NaN channel: one launch per (kind, position), exactly one bad
    value in the field per launch.  The destination buffer is the CPU's (the NaN
    set spreads exactly as the definition says, everything outside the cone is
    bit-identical); the last slot is NaN exactly when the CPU's is; with a NaN
    in the stored box every slot the variant computes is NaN; and the
    convergence check on that state raises the fault flag and done."""
    ops, dtype = h3d.ops, TORCH[dt]
    K = _depth(c)
    done = ext.STATE_DONE_OFFSET // 4
    for name, (n, g, box, u), pos in _positions(ext, c, dt):
        spec = c.spec
        if c in SWEEPS and not c.layout and name != "deep":
            spec = _pinned(ext, c, dt, _geometry(ext, c, dt)[1])
        _, S, C, ambient = _inputs(ops, c, "signed", n, dtype, g)
        for kind in vf.KINDS:
            T = vf.spike(ops, kind, pos, n, dtype, 1, g)
            assert int((~T.flat.isfinite()).sum()) == 1
            want, stored, rc = _cpu(ops, c, T, S, C, box, u, ambient)
            behind_wall = c.wall and any(q < 0 or q >= e for q, e in zip(pos, n))
            # the bad value reached the stored box (a ghost behind a wall is never read)
            assert bool((~stored.isfinite()).any()) != bool(behind_wall), (c.id, name, pos, kind)
            got, rg, st = _gpu(ops, gpu, c, spec, T, S, C, box, u, ambient)
            what = f"{c.id} {dt} {name} {n} {kind} at {pos}"
            report = vf.bits_differ(got, want)
            assert report is None, f"{what} (flat index): {report}"
            assert math.isnan(rg[K - 1]) == math.isnan(rc[K - 1]), f"{what}: last slot {rg[K - 1]!r}, CPU {rc[K - 1]!r}"
            _check_slots(c, stored, rc, rg, what)
            ext.hip.check_convergence(st.data_ptr(), K - 1, torch.cuda.current_stream(gpu).cuda_stream)
            torch.cuda.synchronize()
            flags = st.cpu().view(torch.int32)[done:done + 2].tolist()
            assert flags == ([0, 0] if behind_wall else [1, 1]), f"{what}: done, fault = {flags}"


# ---- d. the solver

N_SOLVER = (41, 37, 45)
# global vertex indices: owned points are 1 .. N - 2
INJECT = {"interior": (21, 19, 23), "last-plane": (39, 19, 23), "last-row": (21, 35, 23), "last-column": (21, 19, 43),
          "odd-column": (21, 19, 22)}
SETUPS = {
    "fp64": dict(dtype="fp64"),
    "fp32": dict(dtype="fp32"),  # the pair kernel
    "convective": dict(dtype="fp64", insulated="x-,z+", convective={"x+": 0.25, "y-": 0.5, "z-": 1.0}, ambient=0.375),
    "wall-source": dict(dtype="fp64", insulated="x-,z+", convective={"x+": 0.25, "y-": 0.5}, ambient=0.375,
                        wall_source_sweeps=True, source=True),
    "conductivity": dict(dtype="fp64", conductivity_sweeps=True, cond=True),
    "ranks8": dict(dtype="fp64", virtual_ranks=8, decomp=(2, 2, 2)),
}


def _solver(h3d, backend, setup):
    kw = dict(SETUPS[setup])
    cond, source = kw.pop("cond", False), kw.pop("source", False)
    if backend == "cpu":
        for k in ("conductivity_sweeps", "wall_source_sweeps"):
            kw.pop(k, None)
    s = h3d.HeatSolver(N_SOLVER, 400, 1e-9, backend=backend, **kw)
    rng = np.random.default_rng(2)
    if cond:
        s.set_conductivity(rng.uniform(0.05, 1.0, N_SOLVER))
    if source:
        s.set_source(rng.uniform(-50.0, 50.0, N_SOLVER))
    return s


def _owner(s, p):
    """(subdomain index, local owned coordinates) of the global vertex p."""
    for idx in range(s.native.num_local):
        sd = s.native.local_subdomain(idx)
        lo, n = sd["gstart"], sd["n"]
        if all(a <= q < a + e for q, a, e in zip(p, lo, n)):
            return idx, tuple(q - a for q, a in zip(p, lo))
    raise AssertionError(p)


_cpu_faults = {}


def _fault_run(h3d, backend, setup, where):
    s = _solver(h3d, backend, setup)
    s.step(12)
    s.synchronize()
    idx, (i, j, k) = _owner(s, INJECT[where])
    s.native.inject(idx, i, j, k, float("nan"))
    r = s.run()
    return r, s.state()


@pytest.mark.parametrize("where", sorted(INJECT))
@pytest.mark.parametrize("setup", sorted(SETUPS))
def test_solver_fault_from_any_position(h3d, gpu, setup, where):
    """d. 12 steps, a NaN injected, run(): a fault and no convergence, at the
    CPU backend's iteration."""
    key = (setup, where)
    if key not in _cpu_faults:
        _cpu_faults[key] = _fault_run(h3d, "cpu", setup, where)
    rc, sc = _cpu_faults[key]
    assert rc["fault"] and not rc["converged"], rc
    r, st = _fault_run(h3d, "hip", setup, where)
    assert r["fault"] and not r["converged"], r
    assert r["conv_iter"] == rc["conv_iter"] and st["conv_iter"] == sc["conv_iter"], (r, rc)
    assert st["fault"] == sc["fault"] == 1


# ---- e. decay through the subnormal range

N_DECAY = (17, 17, 33)
DECAY_STEPS = {False: 7710, True: 17228}  # uniform, layered: found on the CPU backend


def _decay(h3d, backend, layered):
    s = h3d.HeatSolver(N_DECAY, 10 ** 6, 0.0, dtype="fp32", backend=backend, convective={"all": 1.0}, ambient=0.0,
                       conductivity_sweeps=(layered and backend == "hip"))
    if layered:
        s.set_conductivity(s.model.layered_conductivity(0.25, 1.0))
    s.set_field(vf.values("signed", N_DECAY, torch.float32, 11).double().numpy() * 2.0 ** -100)
    s.step(DECAY_STEPS[layered])
    s.synchronize()
    field = torch.from_numpy(np.ascontiguousarray(s.gather())).to(torch.float32)
    return s, field, list(s.native.residual_history())


@pytest.mark.parametrize("layered", [False, True], ids=["uniform", "layered"])
def test_decay_through_subnormals(h3d, gpu, layered):
    """e. fp32, all six faces convective at beta = 1 towards ambient = 0, from
    signed 2^-100: after DECAY_STEPS steps (the smallest count at which the CPU
    run's interior is entirely subnormal or zero but not all zero) the fields
    have the same bits and the residual histories are equal."""
    _, want, hc = _decay(h3d, "cpu", layered)
    inner = want[1:-1, 1:-1, 1:-1]
    s = vf.shares(inner)
    assert not s["normal"] and s["nonzero"] and s["subnormal"] > 0, s
    solver, got, hg = _decay(h3d, "hip", layered)
    if layered:
        assert solver.native.sweeps_active
    assert vf.same_bits(got, want)
    assert len(hg) == len(hc) and [_bits(a) for a in hg] == [_bits(b) for b in hc]
