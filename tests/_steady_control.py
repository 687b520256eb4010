"""The steady solve's control flow and its kernels past one pass: helpers and
test bodies shared by tests/test_steady_control_cpu.py (CPU backend) and
tests/test_gpu_steady_control.py (gfx950 against the CPU backend).

A. `Replica` is the loop of csrc/runtime/solver_steady.cpp on one subdomain,
   driven from the host: ops.steady_apply / steady_update / steady_direction for
   the fields and the dot products, `steady_scalars_step` in Python floats for
   alpha, beta, the count and the stop flag.  Reduction shapes depend on the box
   alone and the solver runs the same kernels, so the solver and the replica
   agree bit for bit: no tolerance anywhere in these comparisons.  Between two
   polls the solver enqueues up to seven iterations after the flag is set; the
   replica stops at the flag, so a kernel that ignored the flag, or took alpha /
   beta from the wrong place, shows as a difference.
B. the exits of the outer loop: already solved, non-finite, restarts, twice.
C. the shapes at which steady_cg.hip's loops take a second pass (geometry()
   mirrors the launch arithmetic; each case asserts its premise).
D. the value classes of tests/_value_fields.py through the three operations."""
import math

import numpy as np
import torch

import _steady_cases as sc
import _value_fields as vf

EPS = sc.EPS
DBL_MAX = 1.7976931348623157e308
MAX_RESTARTS = 3  # kMaxRestarts of solver_steady.cpp
KEYS = ("converged", "iterations", "residual", "true_residual", "r0_norm", "restarts", "status")

# ---- A. the replica -------------------------------------------------------------
BOX = (18, 21, 67)  # two z tiles, partial y and z tiles
CAPS = (1, 7, 8, 9, 16, 17)  # around kPoll = 8 and twice that
CAP_TOL = 1e-12
# form -> solver keywords, source, conductivity ("random": uniform in [c_min, 1]; "layered": c_min / 1 in y)
FORMS = {
    "dirichlet": dict(solver={}, source=False, cond=None),
    "mixed": dict(solver=dict(insulated="z-,z+", convective={"x+": 0.5}, ambient=0.25), source=True, cond="random"),
    "layered": dict(solver={}, source=False, cond="layered"),
    "slab": dict(solver=dict(insulated="x-,x+,z-,z+", convective={"y-": 0.5}, ambient=0.25), source=False, cond=None),
    "open_form": dict(solver=dict(convective={"x+": 0.5}, ambient=0.25), source=True, cond="random"),
}
# Uncapped runs: tolerances picked on the CPU backend so that the count is not a
# multiple of kPoll = 8 (the flag is set between two polls) and no restart
# happens; both are asserted as conditions of the case (on the CPU solve).
UNCAPPED_TOL = {"dirichlet": 1e-8, "mixed": 1e-8}

# Restarts, found by a search on the CPU backend over tol in {1e-13, 3e-14, 1e-14,
# 3e-15, 1e-15}, the forms layered / open_form, c_min in {0.25, 1e-1, 1e-2, 1e-3,
# 1e-4} and the boxes (18, 21, 67), (18, 33, 19), (33, 33, 65):
# (form, box, c_min, tol) -> what the CPU backend reported (restarts, iterations).
RESTART_CASES = {
    ("layered", (18, 33, 19), 0.25, 1e-15): (1, 253),
    ("open_form", (18, 21, 67), 0.25, 1e-15): (1, 328),
}
# That search found one restart wherever it found any (33 of 150 runs), never
# kMaxRestarts.  A start at rounding level does end there: the slab's exact
# steady state leaves r0 = 3.6e-16, no iterate has a true residual 1e-10 times
# that, and the CPU backend stops after three restarts, not converged.
EXHAUSTED = ("slab", (17, 33, 19), 1e-10, (3, 124))


def start(h3d, form, backend, N=BOX, c_min=0.25, seed=5, field=None):
    """The solver of a form with a seeded random interior as the initial guess
    (no residual element is exactly zero); returns (solver, source q, conductivity c)."""
    f = FORMS[form]
    kw = dict(f["solver"])
    if backend == "hip":
        kw["device"] = 0
    s = h3d.HeatSolver(N, 100, 1e-5, backend=backend, dtype="fp64", **kw)
    s.initialize()
    m = s.model
    rng = np.random.default_rng(seed)
    q = m.sine_source(0.25) if f["source"] else None
    c = None
    if f["cond"] == "random":
        c = rng.uniform(c_min, 1.0, N)
    elif f["cond"] == "layered":
        c = m.layered_conductivity(c_min, 1.0)
    if q is not None:
        s.set_source(q)
    if c is not None:
        s.set_conductivity(c)
    if field is None:
        field = m.initial_field()
        field[1:-1, 1:-1, 1:-1] = rng.uniform(-1.0, 1.0, [n - 2 for n in N])
    s.set_field(field)
    return s, q, c


class Replica:
    """solve_steady on one subdomain, from the host.  The fields x, p, r, q and
    the form are kept between calls, as the solver keeps them."""

    def __init__(self, h3d, form, s, q, c, device):
        from heat3d_amd import ops

        self.ops = ops
        N = tuple(s.model.n)
        self.N = N
        ph = s.native.physics  # the solver's own bits of D and dt
        self.D = list(ph["D"])
        self.x = sc.padded(h3d, N, s.gather(), device)
        self.p, self.r, self.q = (sc.padded(h3d, N, np.zeros(N), device) for _ in range(3))
        kw = FORMS[form]["solver"]
        mask = ops.insulated_mask(kw.get("insulated"))
        conv = ops.convective_faces(kw.get("convective"))
        self.form = dict(kind=[2 if conv[f] >= 0 else (mask >> f) & 1 for f in range(6)],
                         beta=[max(conv[f], 0.0) for f in range(6)], ambient=float(kw.get("ambient", 0.0)))
        if c is not None:
            self.form["cond"] = sc.padded(h3d, N, 0.5 * c, device)  # Ch = 0.5 c, exact
        self.source = sc.padded(h3d, N, ph["dt"] * q, device) if q is not None else None  # S = dt q, rounded once

    def interior_bits(self):
        return self.x.owned().cpu().numpy().view(np.int64)

    def solve(self, tol, cap=None):
        ops, x, p, r, q, D = self.ops, self.x, self.p, self.r, self.q, self.D
        max_iter = cap if cap else 10 * sum(self.N)
        tol2 = tol * tol
        p.flat.zero_()
        it, rr, rr0, done, status, restarts, first = 0, 0.0, -1.0, False, "running", 0, True
        while True:
            hi, lo = ops.steady_apply(x, r, D, residual=True, source=self.source, **self.form)
            true_rr = hi + lo
            ref = true_rr if first else rr0
            finite = true_rr == true_rr and true_rr <= DBL_MAX
            if not finite:
                status = "breakdown"
                break
            if true_rr <= tol2 * ref:
                if first:
                    status = "converged"
                break
            if not first:
                if status != "converged" or restarts == MAX_RESTARTS:
                    break
                restarts += 1
            # steady_scalars_step, Init (the count goes on across restarts)
            done, status = False, "running"
            rr = true_rr
            if rr0 < 0.0:
                rr0 = rr
            if rr <= tol2 * rr0:
                done, status = True, "converged"
            elif it >= max_iter:
                done, status = True, "max_iter"
            if not done:
                p.owned().copy_(r.owned())  # the direction kernel's copy form
            while not done:
                hi, lo = ops.steady_apply(p, q, D, **self.form)
                pq = hi + lo
                if not pq > 0.0 or pq > DBL_MAX:  # Alpha
                    done, status = True, "breakdown"
                    break
                alpha = rr / pq
                hi, lo = ops.steady_update(x, p, r, q, alpha)
                rn = hi + lo
                it += 1  # Beta
                if rn != rn or rn > DBL_MAX:
                    rr, done, status = rn, True, "breakdown"
                    break
                beta = rn / rr
                rr = rn
                if rn <= tol2 * rr0:
                    done, status = True, "converged"
                elif it >= max_iter:
                    done, status = True, "max_iter"
                if not done:
                    ops.steady_direction(p, r, beta)
            first = False
        ref = rr0 if rr0 >= 0.0 else true_rr
        rec = rr if rr0 >= 0.0 else true_rr
        return dict(converged=finite and true_rr <= tol2 * ref, iterations=it, restarts=restarts, status=status,
                    r0_norm=math.sqrt(ref) if ref == ref else ref,
                    residual=math.sqrt(rec / ref) if ref > 0.0 else 0.0,
                    true_residual=math.sqrt(true_rr / ref) if ref > 0.0 else 0.0)


def report(r):
    return {k: r[k] for k in KEYS}


def device_of(backend):
    return torch.device("cuda", 0) if backend == "hip" else "cpu"


def solver_bits(s):
    return np.ascontiguousarray(s.gather()[1:-1, 1:-1, 1:-1]).view(np.int64)


def assert_same_solve(s, rep, got, want, what):
    print(f"{what}: solver {report(got)}")
    assert report(got) == want, (what, report(got), want)
    assert got["status"] != "running"
    diff = int((solver_bits(s) != rep.interior_bits()).sum())
    assert diff == 0, f"{what}: {diff} interior values differ from the replica's"


def check_replica(h3d, backend, form, calls, N=BOX, c_min=0.25, field=None):
    """solve_steady(tol, cap) for each (tol, cap) of `calls` on one solver and on
    its replica: the report and the interior field equal, bit for bit, after
    every call.  Returns the solver's reports."""
    s, q, c = start(h3d, form, backend, N=N, c_min=c_min, field=field)
    rep = Replica(h3d, form, s, q, c, device_of(backend))
    assert np.array_equal(solver_bits(s), rep.interior_bits())
    out = []
    for tol, cap in calls:
        got = s.solve_steady(tol, cap)
        want = rep.solve(tol, cap)
        assert_same_solve(s, rep, got, want, f"{form} {backend} {N} tol {tol} cap {cap}")
        out.append(got)
    return out


def check_capped(h3d, backend, form, cap):
    (r,) = check_replica(h3d, backend, form, [(CAP_TOL, cap)])
    assert r["status"] == "max_iter" and r["iterations"] == cap and r["converged"] is False, r
    assert r["restarts"] == 0


def check_uncapped(h3d, backend, form):
    tol = UNCAPPED_TOL[form]
    s, _, _ = start(h3d, form, "cpu")
    cpu = s.solve_steady(tol)
    # the premise of the case: the flag is set between two polls, no restart
    assert cpu["iterations"] % 8 != 0 and cpu["restarts"] == 0 and cpu["converged"], cpu
    (r,) = check_replica(h3d, backend, form, [(tol, None)])
    assert r["converged"] and r["status"] == "converged" and r["restarts"] == 0, r


def check_two_calls(h3d, backend, form):
    """A capped solve, then a second one on its result: r, q, the state buffers
    and the direction's buffer are re-used."""
    first, second = check_replica(h3d, backend, form, [(CAP_TOL, 9), (sc.TOL, sc.CAP)])
    assert first["status"] == "max_iter" and second["converged"] and second["status"] == "converged"


# ---- B. the other exits ---------------------------------------------------------
SOLVED = (17, 17, 17)  # h = 2^-4: T = y is the discrete steady state exactly


def same_values(a, b):
    """bitwise, NaNs taken as equal to each other"""
    return vf.bits_differ(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b))) is None


def check_already_solved(h3d, backend):
    s, _, _ = start(h3d, "dirichlet", backend, N=SOLVED, field=h3d.HeatEquation3D(SOLVED).steady_state())
    T0 = s.gather()
    r = s.solve_steady(sc.TOL, sc.CAP)
    print(f"already solved, {backend}: {r}")
    assert r["r0_norm"] == 0.0, r  # the premise
    assert r["converged"] is True and r["iterations"] == 0 and r["status"] == "converged", r
    assert r["residual"] == 0.0 and r["true_residual"] == 0.0 and r["restarts"] == 0, r
    assert same_values(s.gather(), T0)  # (all-Dirichlet: no wall refresh either)


def nonfinite_field(h3d, kind):
    m = h3d.HeatEquation3D(SOLVED)
    if kind == "huge":  # finite, r . r overflows (and the residual's fma chain with it)
        return vf.values("huge", SOLVED, torch.float64, 3).numpy().copy()
    T = m.initial_field()
    T[1:-1, 1:-1, 1:-1] = np.random.default_rng(9).uniform(-1.0, 1.0, [n - 2 for n in SOLVED])
    T[5, 6, 7] = vf.KINDS[kind]
    return T


def check_nonfinite(h3d, backend, kind):
    """One NaN / Inf at an interior point, or a finite field at 0.9 of the
    largest number: breakdown at once, the field left alone, the next solve on
    the same solver unharmed.  (HeatSolver.set_field refuses non-finite arrays;
    the native set_field, the same bounds-checked scatter, takes them.)"""
    T = nonfinite_field(h3d, kind)
    s, _, _ = start(h3d, "dirichlet", backend, N=SOLVED)
    s.native.set_field(np.ascontiguousarray(T))
    bad = int((~np.isfinite(T[1:-1, 1:-1, 1:-1])).sum())
    assert bad == (0 if kind == "huge" else 1)
    r = s.solve_steady(sc.TOL, sc.CAP)
    print(f"{kind}, {backend}: {r}")
    assert r["converged"] is False and r["status"] == "breakdown" and r["iterations"] <= 1, r
    assert r["restarts"] == 0
    assert same_values(s.gather(), T)
    # the count of NaN / Inf among the updated points: the spike is still there
    # (the huge field is finite and stays so: nothing was iterated)
    assert s.heat_balance()["nonfinite"] == bad
    # state and work buffers are not poisoned: the bits of a fresh solver
    good = start(h3d, "dirichlet", backend, N=SOLVED)[0]
    T1 = good.gather()
    want = good.solve_steady(sc.TOL, sc.CAP)
    s.set_field(T1)
    got = s.solve_steady(sc.TOL, sc.CAP)
    assert got["converged"] and got["status"] == "converged", got
    assert report(got) == report(want) and same_values(s.gather(), good.gather())


def check_restart(h3d, backend, case):
    form, N, c_min, tol = case
    (r,) = check_replica(h3d, backend, form, [(tol, None)], N=N, c_min=c_min)
    assert 1 <= r["restarts"] <= MAX_RESTARTS and r["status"] != "running", r
    assert r["converged"] == (r["true_residual"] <= tol), r
    if backend == "cpu":
        assert (r["restarts"], r["iterations"]) == RESTART_CASES[case], r
    return r


def check_restarts_exhausted(h3d, backend):
    form, N, tol, seen = EXHAUSTED
    exact = h3d.HeatEquation3D(N).convective_slab_steady(0.5, 0.25)
    (r,) = check_replica(h3d, backend, form, [(tol, None)], N=N, field=exact)
    assert r["restarts"] <= MAX_RESTARTS and r["status"] != "running", r
    assert r["converged"] == (r["true_residual"] <= tol), r
    if backend == "cpu":
        assert (r["restarts"], r["iterations"]) == seen and r["converged"] is False, r


def check_solving_twice(h3d, backend, name):
    s, exact, c_min = sc.make_solver(h3d, name, backend)
    T0 = s.gather()
    s.solve_steady(sc.TOL, sc.CAP)
    r = s.solve_steady(sc.TOL)  # against the new, tiny r0
    print(f"second solve, {name} {backend}: {r}")
    assert r["iterations"] <= sc.CAP and r["status"] != "running" and r["restarts"] <= MAX_RESTARTS, r
    kappa = 6.0 * (max(s.model.n) - 1) ** 2 / c_min
    err = float(np.linalg.norm(sc._interior(s.gather() - exact)))
    err0 = float(np.linalg.norm(sc._interior(T0 - exact)))
    print(f"  error {err:.3e} bound {kappa * sc.TOL * err0:.3e}")
    assert err <= kappa * sc.TOL * err0


# ---- C. the kernels past one pass ------------------------------------------------
CG_THREADS, CG_WAVES, CG_AHEAD = 256, 4, 4  # kCgThreads, kCgWaves, kCgAhead of steady_cg.hip
LONG_ROWS = (5, 6, 523)
STRIDED = (11, 4102, 69)


def geometry(ext, extent):
    """The launch arithmetic of steady_cg.hip for a box of `extent` points."""
    max_blocks = ext.STEADY_SCRATCH_BYTES // 16  # kCgMaxBlocks double-double partials
    ex, ey, ez = extent
    nzb, nyb = (ez + 63) // 64, (ey + CG_WAVES - 1) // CG_WAVES
    tiles = nzb * nyb
    nxs = max(1, min((max_blocks + tiles - 1) // tiles, (ex + 7) // 8))
    seg = (ex + nxs - 1) // nxs
    nxs = (ex + seg - 1) // seg
    rows = ex * ey
    return dict(max_blocks=max_blocks, nzb=nzb, nyb=nyb, tiles=tiles, nxs=nxs, seg=seg, ntasks=tiles * nxs,
                blocks=min(max_blocks, tiles * nxs), rows=rows, waves=max_blocks * CG_WAVES,
                row_blocks=min(max_blocks, (rows + CG_WAVES - 1) // CG_WAVES), rounds=-(-ez // (64 * CG_AHEAD)))


def past_one_pass_cases(ext):
    """name -> (N, box, wall); every premise is asserted here, so that a
    retuning of the launch constants fails the case instead of un-testing it."""
    no = ext.NO_WALL
    n = [v - 2 for v in LONG_ROWS]
    g = geometry(ext, n)
    # three k0 rounds, the last one partial, every piece u = 0 .. 3 in the full ones
    assert g["rounds"] == 3 and n[2] % (64 * CG_AHEAD) not in (0,) and n[2] > 2 * 64 * CG_AHEAD and g["nzb"] == 9, g
    cases = {"long_rows": (LONG_ROWS, None, None)}
    n = [v - 2 for v in STRIDED]
    g = geometry(ext, n)
    assert g["ntasks"] > g["max_blocks"] and g["rows"] > g["waves"] and g["nxs"] == 2, g
    assert g["blocks"] == g["max_blocks"] > CG_THREADS  # the final kernel's second pass
    assert (g["nzb"], g["nyb"], g["tiles"], g["ntasks"], g["rows"]) == (2, 1025, 2050, 4100, 36900), g
    cases["strided"] = (STRIDED, None, None)
    # an offset box of the same grid sizes: no wall in reach (a subdomain's inner
    # sides), and the x+ and y+ walls only: x+ lies in the second x segment
    box = [0, n[0], 1, n[1], 2, n[2]]
    g = geometry(ext, [n[0], n[1] - 1, n[2] - 2])
    assert g["ntasks"] > g["max_blocks"] and g["rows"] > g["waves"] and g["nxs"] == 2 and n[0] - 1 >= g["seg"], g
    cases["strided_free"] = (STRIDED, box, [no] * 6)
    cases["strided_xplus"] = (STRIDED, box, [no, n[0] - 1, no, n[1] - 1, no, no])
    return cases


def to_device(f, device):
    from heat3d_amd.ops import PaddedField

    if f is None:
        return None
    d = PaddedField(f.n, dtype=f.dtype, device=device, gx=f.gx, gy=f.gy, gz=f.gz)
    d.flat.copy_(f.flat)
    return d


def pair_equal(a, b):
    return all((u != u and v != v) or (u == v and math.copysign(1.0, u) == math.copysign(1.0, v)) for u, v in zip(a, b))


def terms_of(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64)).ravel()


def check_dot(pair, terms, what, exact=True):
    """The fsum bound where every term and the sum of their magnitudes is
    finite; a non-finite term makes the pair's sum non-finite.  exact=False
    (the 2.5 M-point boxes): the magnitudes summed by NumPy and no fsum."""
    v = pair[0] + pair[1]
    with np.errstate(over="ignore"):
        sabs = float(np.abs(terms).sum())
    if not np.isfinite(terms).all():
        assert not math.isfinite(v), (what, pair)
        return None
    if not math.isfinite(sabs):
        return None
    if exact:
        lst = terms.tolist()
        ref, sabs = math.fsum(lst), math.fsum(abs(t) for t in lst)
        print(f"{what}: {v!r} fsum {ref!r} diff {abs(v - ref):.3e} bound {EPS * sabs:.3e}")
        assert abs(v - ref) <= EPS * sabs, (what, v, ref, EPS * sabs)
    return sabs


def both_dots(dc, dg, terms, what, exact=True):
    """CPU and GPU pairs against fsum; without fsum, against each other: each
    is within 2^-52 sum|terms| of the exact sum, so they differ by at most twice
    that (NumPy's pairwise sum of the magnitudes is good to 2^-40 relative)."""
    sabs = check_dot(dc, terms, what + " cpu", exact)
    if dg is None:
        return
    check_dot(dg, terms, what + " gpu", exact)
    if sabs is not None and not exact:
        d = abs((dg[0] + dg[1]) - (dc[0] + dc[1]))
        print(f"{what}: gpu - cpu {d:.3e} bound {2 * EPS * sabs:.3e}")
        assert d <= 2 * EPS * sabs * (1 + 2.0 ** -40)


SENTINEL = -5.0


def apply_both(device, src, D, kw, residual=False, box=None, wall=None, ambient=0.0, source=None, what="", exact=True):
    """steady_apply on the CPU backend and, with a GPU device, on gfx950: the
    written field (whole flat buffer, sentinel-filled) bitwise the same, the
    same pair twice, the dot products as check_dot.  Returns (out, pair) of the CPU."""
    from heat3d_amd import ops

    def run(dev):
        out = to_device(src, dev)
        out.flat.fill_(SENTINEL)
        k = {key: (to_device(v, dev) if key == "cond" else v) for key, v in kw.items()}
        args = (to_device(src, dev), out, D)
        extra = dict(residual=residual, box=box, wall=wall, ambient=ambient, source=to_device(source, dev), **k)
        pair = ops.steady_apply(*args, **extra)
        assert pair_equal(pair, ops.steady_apply(*args, **extra)), what
        return out, pair

    oc, dc = run("cpu")
    dg = None
    if str(device) != "cpu":
        og, dg = run(device)
        assert vf.same_bits(og.flat.cpu(), oc.flat), what
    o = sc.owned_np(oc, box)
    terms = terms_of(o, o) if residual else terms_of(sc.owned_np(src, box), o)
    with np.errstate(invalid="ignore", over="ignore"):
        both_dots(dc, dg, terms, what, exact)
    return oc, dc


def update_both(device, fields, alpha, beta, box=None, what="", exact=True):
    """steady_update, then steady_direction on its p and r, CPU and (with a GPU
    device) gfx950: all four fields bitwise the same, r . r as check_dot, the
    same pair on a second set of the same fields."""
    from heat3d_amd import ops

    def run(dev):
        f = [to_device(v, dev) for v in fields]
        pair = ops.steady_update(*f, alpha, box=box)
        assert pair_equal(pair, ops.steady_update(*[to_device(v, dev) for v in fields], alpha, box=box)), what
        ops.steady_direction(f[1], f[2], beta, box=box)
        return f, pair

    fc, dc = run("cpu")
    dg = None
    if str(device) != "cpu":
        fg, dg = run(device)
        for a, b in zip(fg, fc):
            assert vf.same_bits(a.flat.cpu(), b.flat), what
    r = sc.owned_np(fc[2], box)
    with np.errstate(invalid="ignore", over="ignore"):
        both_dots(dc, dg, terms_of(r, r), what, exact)
    return fc, dc


def host_field(h3d, N, arr):
    return sc.padded(h3d, N, arr, "cpu")


def check_past_one_pass(h3d, device, name, form, residual, exact):
    ext = h3d.native()
    N, box, wall = past_one_pass_cases(ext)[name]
    D = sc.physics_D(h3d, N)
    a, b, c, d = sc.random_fields(N, 11, 4)
    kw = sc.form_fields(h3d, N, form, "cpu")
    src = host_field(h3d, N, a)
    what = f"{name} {form} {'residual' if residual else 'A'}"
    S = host_field(h3d, N, 1e-3 * b) if residual else None
    apply_both(device, src, D, kw, residual=residual, box=box, wall=wall, ambient=0.25, source=S, what=what, exact=exact)
    if form == "uniform" and not residual:
        fields = [host_field(h3d, N, v) for v in (a, b, c, d)]
        update_both(device, fields, 0.3721, 0.8125, box=box, what=f"{name} update", exact=exact)


# ---- D. value domain -------------------------------------------------------------
VALUE_BOXES = ((3, 4, 5), (9, 50, 130))  # owned points
MODES = ("A", "residual", "residual_source")


def value_case(ops, cls, n, form, seed=21):
    T = vf.field(ops, cls, n, torch.float64, seed)
    kw = {k: v for k, v in sc.FORMS[form].items() if k != "cond"}
    if sc.FORMS[form].get("cond"):
        kw["cond"] = vf.conductivity(ops, n, torch.float64, seed + 1)
    return T, kw


def check_value_apply(h3d, device, cls, form):
    from heat3d_amd import ops

    for n in VALUE_BOXES:
        D = sc.physics_D(h3d, [v + 2 for v in n])
        T, kw = value_case(ops, cls, n, form)
        for mode in MODES:
            S = vf.source(ops, cls, n, torch.float64, 33) if mode == "residual_source" else None
            out, _ = apply_both(device, T, D, kw, residual=mode != "A", ambient=0.25 * vf.scale(cls, torch.float64),
                                source=S, what=f"{cls} {form} {n} {mode}")
            # the class did what it is for, on what the CPU stored (a conductivity
            # turns overflow into Inf, never into NaN, in one application)
            stored = out.owned().flatten()
            if cls == "subnormal_edge":
                # the output is an increment, D times differences, a few binades below the field:
                # with a conductivity all of it can be subnormal.  The class is there for normal and
                # subnormal numbers in one call: a quarter of the results subnormal, normals among
                # what the call reads and writes
                assert vf.shares(stored)["subnormal"] >= 0.25
                stored = torch.cat((T.owned().flatten(), stored))
            # huge: Inf - Inf needs two axes that overflow with opposite signs at one point: certain
            # among 58500 points, a matter of chance among 60; never with a conductivity (conditions)
            s = vf.conditions(cls, stored, need_nan=not kw.get("cond") and n == VALUE_BOXES[1])
            print(f"{cls} {form} {n} {mode}: {s}")


def check_value_update(h3d, device, cls, sign):
    from heat3d_amd import ops

    for n in VALUE_BOXES:
        # subnormal_edge at half its scale: a sum of two such values is subnormal less often than one
        # of them, and `conditions` wants a quarter of what is stored subnormal
        factor = 0.5 if cls == "subnormal_edge" else 1.0
        fields = [vf.field(ops, cls, n, torch.float64, 40 + i, factor=factor) for i in range(4)]
        fc, _ = update_both(device, fields, sign * 0.3721, -sign * 0.8125, what=f"{cls} {n} update {sign:+d}")
        if cls in vf.FINITE_CLASSES:
            vf.conditions(cls, fc[0].owned())
            vf.conditions(cls, fc[2].owned())


def wall_shell(n, faces):
    """mask over the ghosted shape (n + 2): the wall vertices of the given faces"""
    m = torch.zeros([v + 2 for v in n], dtype=torch.bool)
    for f in faces:
        idx = [slice(None)] * 3
        idx[f // 2] = 0 if f % 2 == 0 else n[f // 2] + 1
        m[tuple(idx)] = True
    return m


def check_wall_vertices_may_hold_anything(h3d, device, form, residual):
    """NaN at every wall vertex that the operator is documented not to read:
    all six faces in A (a Dirichlet wall counts as 0 there), the insulated and
    convective faces in the residual form.  The output and its dot product are
    bitwise those of zeros there, and free of NaN.  The conductivity stays
    finite: Ch at the wall vertex is part of the face weight."""
    from heat3d_amd import ops

    kinds = sc.FORMS[form]["kind"]
    faces = [f for f in range(6) if not residual or kinds[f] != 0]
    assert len(faces) == (4 if residual else 6)
    for n in VALUE_BOXES:
        D = sc.physics_D(h3d, [v + 2 for v in n])
        T, kw = value_case(ops, "signed", n, form)
        shell = wall_shell(n, faces)
        outs = []
        for fill in (0.0, float("nan")):
            F = to_device(T, "cpu")
            F.ghosted()[shell] = fill
            assert int(F.ghosted().isnan().sum()) == (int(shell.sum()) if fill != fill else 0)
            outs.append(apply_both(device, F, D, kw, residual=residual, ambient=0.25,
                                   what=f"wall vertices {fill} {form} {n} residual {residual}"))
        (o0, d0), (o1, d1) = outs
        assert not o1.owned().isnan().any() and math.isfinite(d1[0] + d1[1])
        assert vf.same_bits(o1.flat, o0.flat) and d0 == d1, (d0, d1)


def check_one_spike(h3d, device, kind, form, residual):
    """One NaN / Inf at the first or the last owned point reaches that point and
    its stencil neighbours inside the box, and nothing else (on the CPU; the
    GPU's field is bitwise the CPU's)."""
    from heat3d_amd import ops

    for n in VALUE_BOXES:
        D = sc.physics_D(h3d, [v + 2 for v in n])
        _, kw = value_case(ops, "signed", n, form)
        for pos in ((0, 0, 0), tuple(v - 1 for v in n)):
            T = vf.spike(ops, kind, pos, n, torch.float64, 21)
            out, pair = apply_both(device, T, D, kw, residual=residual, ambient=0.25,
                                   what=f"spike {kind} {pos} {form} {n} residual {residual}")
            want = torch.zeros(n, dtype=torch.bool)
            want[pos] = True
            for a in range(3):
                for e in (-1, 1):
                    q = list(pos)
                    q[a] += e
                    if 0 <= q[a] < n[a]:
                        want[tuple(q)] = True
            assert torch.equal(~out.owned().isfinite(), want), (kind, pos, n)
            assert not math.isfinite(pair[0] + pair[1])
