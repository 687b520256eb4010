#!/usr/bin/env python3
"""Cost of implicit time steps (HeatSolver.step_implicit) on one GPU, set against
explicit stepping over the same physical time in the same build.

Per size, body, step length m and theta (fp64, tol --tol, from initial_field()):
CG iterations per implicit step, ms per implicit step (the median, with the
smallest and largest, of --reps steps taken one after the other, after one
untimed step of the same case; a case whose untimed step takes longer than
--long seconds gets one timed step, and the untimed one's time is reported
beside it), and ms for m explicit steps,
m times the median of --reps timed chunks of --steps explicit steps after a
warm-up chunk (explicit cost is linear in m).  Bodies: "uniform" (lean K-step
sweeps), "layered" (layered_conductivity(0.25, 1) with layered_capacity(1, 8);
explicit with the capacity sweeps off and on), "capacity" (that capacity
without a conductivity: explicit single steps).  The fields are re-initialised
before every case.  Prints one JSON line per case and a markdown table.

  python tools/bench_implicit.py --sizes 512 --bodies uniform layered capacity
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HEAT3D_RUNTIME", "rocm")


def make(h3d, n, body, **kw):
    s = h3d.HeatSolver((n, n, n), 10 ** 9, 0.0, backend="hip", device=0, dtype="fp64", **kw)
    s.initialize()
    if body == "layered":
        s.set_conductivity(s.model.layered_conductivity(0.25, 1.0))
    if body in ("layered", "capacity"):
        s.set_capacity(s.model.layered_capacity(1.0, 8.0))
    return s


def explicit_ms(h3d, n, body, steps, reps, **kw):
    s = make(h3d, n, body, **kw)
    s.step(steps)
    s.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        s.step(steps)
        s.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / steps)
    return statistics.median(out), s.kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--bodies", nargs="+", default=["uniform", "layered", "capacity"])
    ap.add_argument("--m", type=float, nargs="+", default=[16, 256, 4096, 65536])
    ap.add_argument("--theta", type=float, nargs="+", default=[1.0, 0.5])
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--steps", type=int, default=60, help="explicit steps per timed chunk")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--long", type=float, default=5.0,
                    help="a case whose untimed first step is longer than this (s) gets one timed step")
    a = ap.parse_args()
    import heat3d_amd as h3d

    rows = []
    for n in a.sizes:
        for body in a.bodies:
            ex = {"explicit": explicit_ms(h3d, n, body, a.steps, a.reps)}
            if body == "layered":
                ex["explicit, capacity sweeps"] = explicit_ms(h3d, n, body, a.steps, a.reps, capacity_sweeps=True)
            s = make(h3d, n, body)
            s.step_implicit(1, 16.0, 1.0, tol=a.tol)  # (untimed: first use of the kernels and the work fields)
            for m in a.m:
                for theta in a.theta:
                    s.initialize()
                    warm = s.step_implicit(1, m, theta, tol=a.tol)
                    reps = 1 if warm["seconds"] > a.long else a.reps
                    got = [s.step_implicit(1, m, theta, tol=a.tol) for _ in range(reps)]
                    ms = statistics.median(1e3 * r["seconds"] for r in got)
                    its = [r["iterations"] for r in got]
                    row = {"n": n, "body": body, "m": m, "theta": theta, "tol": a.tol, "timed_steps": reps,
                           "first_step_iterations": warm["iterations"], "first_step_ms": 1e3 * warm["seconds"],
                           "iterations": its, "implicit_ms_min": min(1e3 * r["seconds"] for r in got),
                           "implicit_ms_max": max(1e3 * r["seconds"] for r in got),
                           "converged": all(r["converged"] for r in got), "implicit_ms_per_step": ms,
                           "ms_per_iteration": ms / max(1, statistics.median(its))}
                    for name, (ms1, kernel) in ex.items():
                        row[name + " ms"] = ms1 * m
                        row[name + " ms per step"] = ms1
                        row[name + " kernel"] = kernel
                    print(json.dumps(row), flush=True)
                    rows.append(row)
            del s
    print("\n| N | body | m | theta | CG iterations / step | ms / implicit step | ms / CG iteration | explicit ms for m steps"
          " | ... with capacity sweeps | implicit / best explicit |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        e1, e2 = r["explicit ms"], r.get("explicit, capacity sweeps ms")
        best = min(e1, e2) if e2 is not None else e1
        print(f"| {r['n']} | {r['body']} | {r['m']:g} | {r['theta']:g} | {statistics.median(r['iterations']):g} |"
              f" {r['implicit_ms_per_step']:.1f} | {r['ms_per_iteration']:.3f} | {e1:.1f} |"
              f" {'-' if e2 is None else format(e2, '.1f')} | {r['implicit_ms_per_step'] / best:.2f} |")


if __name__ == "__main__":
    main()
