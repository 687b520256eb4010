"""The heat balance on the GPU: the gfx950 kernel (heat_balance.hip) against the
CPU definition at kernel level on boxes whose z extents are below a wave, a wave
plus a tail and a block plus an odd tail, in shallow and deep layouts with NaN
everywhere the kernel must not read; the solver across virtual ranks against
the fsum reference; stale wall planes after sweeps; the steady slab; NaN, Inf
and subnormal fields; repeated calls.

Tolerance (derived in tests/test_heat_balance_cpu.py): tol = ulp + n * 2^-100 *
sum|term| against the correctly rounded sum.  Two implementations are held to
the same tol against each other: each differs from the correctly rounded sum
only when the exact sum lies within n * 2^-100 * sum|term| of a rounding
boundary, and then both fall on one of the two values next to that boundary.
Minimum, maximum and the non-finite count are exact."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FACES = ("x-", "x+", "y-", "y+", "z-", "z+")
BOXES = [(7, 6, 5), (9, 8, 70), (6, 7, 261)]
WALLS = {
    "A": dict(insulated="x+,z-", convective={"x-": 0.5, "y+": 0.3}, ambient=1.75),
    "B": dict(insulated="x-,z+", convective={"x+": 0.5, "y-": 0.3}, ambient=1.75),
}
MATERIALS = {"plain": (False, False), "source": (True, False), "conductivity": (False, True), "both": (True, True)}
TORCH = {"fp64": torch.float64, "fp32": torch.float32}
NUMPY = {"fp64": np.float64, "fp32": np.float32}
EPS = {"fp64": 2.0 ** -52, "fp32": 2.0 ** -23}


def tol(ref, key):
    n, sabs = ref["terms"][key]
    value = ref["flow"][key] if key in FACES else ref[key]
    return math.ulp(value) + n * 2.0 ** -100 * sabs


def close(a, b, ref, what):
    """Balance a against b (another implementation, or the reference itself) within tol."""
    slack = 0.0
    for key in ("heat", "source_power") + FACES:
        x = a["flow"][key] if key in FACES else a[key]
        y = b["flow"][key] if key in FACES else b[key]
        print(f"{what} {key}: {x!r} vs {y!r} diff {abs(x - y):.3e} tol {tol(ref, key):.3e}")
        assert abs(x - y) <= tol(ref, key), (what, key)
        slack += tol(ref, key) if key != "heat" else 0.0
    for key in ("t_min", "t_max"):
        assert np.float64(a[key]).tobytes() == np.float64(b[key]).tobytes(), (what, key)
    assert a["nonfinite"] == b["nonfinite"], what
    mag = sum(abs(v) for v in ref["flow"].values()) + abs(ref["source_power"])
    assert abs(a["imbalance"] - b["imbalance"]) <= slack + 7 * math.ulp(mag), (what, "imbalance")


def padded(ops, n, td, depth, G, fill, planes=FACES):
    """A CPU PaddedField, NaN everywhere except the owned block (from the global
    array G of shape n + 2) and the wall vertices behind the owned block of the
    faces in ``planes``."""
    f = ops.PaddedField(n, dtype=td, gx=depth, gy=depth, gz=depth)
    f.flat.fill_(fill)
    Gt = torch.from_numpy(G).to(td)
    f.owned().copy_(Gt[1:-1, 1:-1, 1:-1])
    d = depth
    v = f.deep3()
    for face in planes:
        a, e = divmod(FACES.index(face), 2)
        src = [slice(1, -1)] * 3
        dst = [slice(d, d + n[0]), slice(d, d + n[1]), slice(d, d + n[2])]
        src[a] = -1 if e else 0
        dst[a] = d + n[a] if e else d - 1
        v[tuple(dst)] = Gt[tuple(src)]
    return f


def to_gpu(ops, f, gpu):
    g = ops.PaddedField(f.n, dtype=f.dtype, device=gpu, gx=f.gx, gy=f.gy, gz=f.gz)
    g.flat.copy_(f.flat)
    return g


class Offset:
    """A GPU copy of a PaddedField that starts one element into its allocation:
    no field pointer is 16-byte aligned, and the kernel takes its one-element form."""

    def __init__(self, f, gpu):
        self.n, self.dtype, self.layout, self.gx, self.gy, self.gz, self.dt = f.n, f.dtype, f.layout, f.gx, f.gy, f.gz, f.dt
        self.store = torch.full((f.flat.numel() + 1,), float("nan"), dtype=f.dtype, device=gpu)
        self.flat = self.store[1:]
        self.flat.copy_(f.flat)
        self.device = self.flat.device

    def data_ptr(self):
        return self.flat.data_ptr()


def dirichlet_faces(walls):
    return [f for f in FACES if f not in walls["insulated"] and f not in walls["convective"]]


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("walls", sorted(WALLS))
@pytest.mark.parametrize("n", BOXES, ids=lambda n: "x".join(map(str, n)))
def test_kernel_matches_cpu(h3d, gpu, n, walls, dtype):
    """ops.heat_balance on the GPU against the CPU definition, ghost depth 1 and
    4, the four material cases.  Everything outside the owned box and the
    Dirichlet wall vertices is NaN (in the conductivity: outside the box and the
    wall vertices of the faces that carry a flow), and the result is finite."""
    from heat3d_amd.utils.metrics import heat_balance_reference

    ops, td, ws = h3d.ops, TORCH[dtype], WALLS[walls]
    N = tuple(e + 2 for e in n)
    model = h3d.HeatEquation3D(N)
    rng = np.random.default_rng(sum(n))
    T, q, c = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N), rng.uniform(0.25, 1, N)
    S = (model.dt * q).astype(NUMPY[dtype]).astype(np.float64)  # the stored source, as the reference forms it
    mask = ops.insulated_mask(ws["insulated"]) | ops.convective_mask(ws["convective"])
    wc = ops.wall_coords(mask, n)
    for depth in (1, 4):
        fT = padded(ops, n, td, depth, T, float("nan"), dirichlet_faces(ws))
        fS = padded(ops, n, td, depth, S, float("nan"), ())
        fC = padded(ops, n, td, depth, 0.5 * c, float("nan"), [f for f in FACES if f not in ws["insulated"]])
        gT, gS, gC = (to_gpu(ops, f, gpu) for f in (fT, fS, fC))
        for name, (src, cond) in MATERIALS.items():
            kw = dict(walls=wc, conv=ws["convective"], ambient=ws["ambient"])
            cpu = ops.heat_balance(fT, model, source=fS if src else None, cond=fC if cond else None, **kw)
            got = ops.heat_balance(gT, model, source=gS if src else None, cond=gC if cond else None, **kw)
            ref = heat_balance_reference(T, model, source=q if src else None,
                                         conductivity=c if cond else None, dtype=dtype, **ws)
            what = f"{n} {walls} {dtype} depth {depth} {name}"
            assert got["nonfinite"] == 0 and math.isfinite(got["heat"]) and math.isfinite(got["imbalance"]), what
            assert all(math.isfinite(v) for v in got["flow"].values()), what
            close(got, cpu, ref, what + " gpu vs cpu")
            close(got, ref, ref, what + " gpu vs reference")
            for f in FACES:
                assert (got["flow"][f] == 0.0) == (f in ws["insulated"]), (what, f)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("n", BOXES, ids=lambda n: "x".join(map(str, n)))
def test_kernel_unaligned_fields(h3d, gpu, n, dtype):
    """Fields that are not 16-byte aligned run the kernel's one-element form:
    the same checks as above, wall set A, source and conductivity, deep layout."""
    from heat3d_amd.utils.metrics import heat_balance_reference

    ops, td, ws = h3d.ops, TORCH[dtype], WALLS["A"]
    N = tuple(e + 2 for e in n)
    model = h3d.HeatEquation3D(N)
    rng = np.random.default_rng(sum(n) + 1)
    T, q, c = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N), rng.uniform(0.25, 1, N)
    S = (model.dt * q).astype(NUMPY[dtype]).astype(np.float64)
    mask = ops.insulated_mask(ws["insulated"]) | ops.convective_mask(ws["convective"])
    kw = dict(walls=ops.wall_coords(mask, n), conv=ws["convective"], ambient=ws["ambient"])
    fT = padded(ops, n, td, 4, T, float("nan"), dirichlet_faces(ws))
    fS = padded(ops, n, td, 4, S, float("nan"), ())
    fC = padded(ops, n, td, 4, 0.5 * c, float("nan"), [f for f in FACES if f not in ws["insulated"]])
    gT, gS, gC = (Offset(f, gpu) for f in (fT, fS, fC))
    assert all(g.data_ptr() % 16 != 0 for g in (gT, gS, gC))
    for src, cond in ((False, False), (True, True)):
        cpu = ops.heat_balance(fT, model, source=fS if src else None, cond=fC if cond else None, **kw)
        got = ops.heat_balance(gT, model, source=gS if src else None, cond=gC if cond else None, **kw)
        ref = heat_balance_reference(T, model, source=q if src else None, conductivity=c if cond else None,
                                     dtype=dtype, **ws)
        what = f"unaligned {n} {dtype} src {src} cond {cond}"
        assert got["nonfinite"] == 0 and math.isfinite(got["heat"]) and math.isfinite(got["imbalance"]), what
        close(got, cpu, ref, what + " gpu vs cpu")
        close(got, ref, ref, what + " gpu vs reference")


def hip_solver(h3d, N, dtype, walls, vr=1, **kw):
    return h3d.HeatSolver(N, iter_max=100, eps=0.0, dtype=dtype, backend="hip", device=0, virtual_ranks=vr, **walls, **kw)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_solver_decomposition(h3d, gpu, dtype):
    """1 and 8 virtual ranks (combined on the device in subdomain order) on
    (19, 21, 70), wall set A with a source: both within tol of the reference."""
    from heat3d_amd.utils.metrics import heat_balance_reference

    N = (19, 21, 70)
    rng = np.random.default_rng(19)
    T, q = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N)
    out = []
    for vr in (1, 8):
        s = hip_solver(h3d, N, dtype, WALLS["A"], vr)
        s.set_field(T)
        s.set_source(q)
        out.append(s.heat_balance())
        ref = heat_balance_reference(T, s.model, source=q, dtype=dtype, **WALLS["A"])
        close(out[-1], ref, ref, f"solver {dtype} vr{vr}")
        assert s.heat_balance() == out[-1]  # a repeated call: the same bits
    close(out[0], out[1], ref, f"solver {dtype} vr1 vs vr8")


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("case", ["plain", "conductivity_sweeps"])
def test_stale_walls_after_sweeps(h3d, gpu, case, dtype):
    """step(5) on the sweep path leaves the wall planes stale; the same run in
    single steps refreshes them.  Identical field bits give identical balance bits."""
    N = (19, 21, 70)
    rng = np.random.default_rng(23)
    T, c = rng.uniform(-1, 1, N), rng.uniform(0.25, 1, N)
    out = []
    for temporal in (None, "1"):
        extra = ["--temporal", temporal] if temporal else []
        s = hip_solver(h3d, N, dtype, WALLS["A"], extra_args=extra, conductivity_sweeps=case != "plain")
        s.set_field(T)
        if case != "plain":
            s.set_conductivity(c)
        s.step(5)
        s.synchronize()
        out.append((s.native.sweeps_active, s.gather()[1:-1, 1:-1, 1:-1], s.heat_balance()))
    assert out[0][0] and not out[1][0]
    assert np.array_equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2]
    assert out[0][2]["nonfinite"] == 0 and out[0][2]["flow"]["x+"] == 0.0 and out[0][2]["flow"]["x-"] != 0.0


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_steady_slab_flows(h3d, gpu, dtype):
    """As on the CPU, at (9, 33, 70): beta = 1 and ambient 0 make s = 1/32 and
    every T_j = j/32 exact in both dtypes, so the issue's bound tol + 4 eps |flow|
    applies to the stored field."""
    from heat3d_amd.utils.metrics import heat_balance_reference

    N, beta, ambient = (9, 33, 70), 1.0, 0.0
    walls = dict(insulated="x-,x+,z-,z+", convective={"y-": beta}, ambient=ambient)
    s = hip_solver(h3d, N, dtype, walls)
    T = s.model.convective_slab_steady(beta, ambient)
    assert np.array_equal(T.astype(np.float32).astype(np.float64), T)
    s.set_field(T)
    got = s.heat_balance()
    want = s.model.convective_slab_flows(beta, ambient)
    ref = heat_balance_reference(T, s.model, dtype=dtype, **walls)
    bound = 0.0
    for f in ("y-", "y+"):
        bound = tol(ref, f) + 4 * EPS[dtype] * abs(want[f])
        print(f"slab {dtype} {f}: got {got['flow'][f]!r} exact {want[f]!r} bound {bound:.3e}")
        assert abs(got["flow"][f] - want[f]) <= bound
    for f in ("x-", "x+", "z-", "z+"):
        assert got["flow"][f] == 0.0
    assert want["y-"] < 0 and abs(got["imbalance"]) <= bound


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_value_classes(h3d, gpu, dtype):
    """One Inf, one NaN (each in an interior row and at a wall-adjacent point) and
    a field of subnormals: the non-finite count, the range (NaNs ignored) and the
    NaN-ness of the heat are those of the CPU definition."""
    ops, td = h3d.ops, TORCH[dtype]
    n = (6, 7, 261)
    N = tuple(e + 2 for e in n)
    model = h3d.HeatEquation3D(N)
    rng = np.random.default_rng(29)
    base = rng.uniform(-1, 1, N)
    tiny = float(np.finfo(np.float32 if dtype == "fp32" else np.float64).smallest_subnormal)
    fields = {}
    for name, value in (("inf", float("inf")), ("nan", float("nan"))):
        for where, at in (("interior", (3, 3, 130)), ("wall", (1, 4, 261))):  # global indices: the second is next to x- and z+
            G = base.copy()
            G[at] = value
            fields[f"{name} {where}"] = (G, 1)
    sub = rng.integers(-7, 8, N).astype(np.float64) * tiny
    fields["subnormal"] = (sub, 0)
    for what, (G, bad) in fields.items():
        f = padded(ops, n, td, 1, G, float("nan"))
        cpu = ops.heat_balance(f, model)
        got = ops.heat_balance(to_gpu(ops, f, gpu), model)
        print(what, dtype, got)
        assert got["nonfinite"] == cpu["nonfinite"] == bad, what
        for key in ("t_min", "t_max"):
            assert np.float64(got[key]).tobytes() == np.float64(cpu[key]).tobytes(), (what, key)
        assert math.isnan(got["heat"]) == math.isnan(cpu["heat"]) == bool(bad), what
        if what == "subnormal":
            assert got["heat"] == cpu["heat"] and got["flow"] == cpu["flow"]
            assert got["t_min"] == -7 * tiny and got["t_max"] == 7 * tiny
        if what.startswith("inf"):
            assert got["t_max"] == float("inf")
        if what.startswith("nan"):
            assert got["t_max"] <= 1.0


def test_repeated_call_same_bits(h3d, gpu):
    ops = h3d.ops
    n = (9, 8, 70)
    N = tuple(e + 2 for e in n)
    G = np.random.default_rng(31).uniform(-1, 1, N)
    g = to_gpu(ops, padded(ops, n, torch.float64, 1, G, float("nan")), gpu)
    model = h3d.HeatEquation3D(N)
    a, b = ops.heat_balance(g, model), ops.heat_balance(g, model)
    assert a == b and a["nonfinite"] == 0
