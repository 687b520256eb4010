#!/usr/bin/env python3
"""Cost of the direct steady-state solve (HeatSolver.solve_steady) on one GPU,
set against the time stepper of the same build.

Per size (default 512 and 1024, fp64, the reference problem from
initial_field()): ms per CG iteration, iterations and seconds to --tol, the
error against T = y at the end; the tile kernel's single step (ms, the median
of --reps timed chunks) and the bound 1.3 x 5.5 x that step; with --converge
also the time stepper's time to converge at --eps and its error.  Prints one
JSON line per size and a markdown table.

  python tools/bench_steady.py --sizes 512 1024 --converge
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


def single_step_ms(h3d, n, steps, reps):
    s = h3d.HeatSolver((n, n, n), 10 ** 9, 0.0, backend="hip", device=0, dtype="fp64",
                       extra_args=["--temporal", "1"])
    s.initialize()
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
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--eps", type=float, default=1e-5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--converge", action="store_true", help="also run the time stepper to --eps")
    ap.add_argument("--converge-max", type=int, default=512, help="largest size the time stepper is run at")
    a = ap.parse_args()
    import heat3d_amd as h3d

    rows = []
    for n in a.sizes:
        step_ms, kernel = single_step_ms(h3d, n, a.steps, a.reps)
        s = h3d.HeatSolver((n, n, n), 10, a.eps, backend="hip", device=0, dtype="fp64")
        s.initialize()
        r = s.solve_steady(a.tol)
        err = s.error_percent()[0]
        row = {"n": n, "tol": a.tol, "converged": r["converged"], "iterations": r["iterations"],
               "seconds": r["seconds"], "ms_per_iteration": 1e3 * r["seconds"] / max(1, r["iterations"]),
               "true_residual": r["true_residual"], "error_percent": err, "single_step_ms": step_ms,
               "single_step_kernel": kernel, "bound_ms": 1.3 * 5.5 * step_ms}
        del s
        if a.converge and n <= a.converge_max:
            t = h3d.HeatSolver((n, n, n), 10 ** 7, a.eps, backend="hip", device=0, dtype="fp64")
            rr = t.run()
            row.update(stepper_seconds=rr["seconds"], stepper_iterations=rr["conv_iter"],
                       stepper_error_percent=rr["error_percent"], stepper_kernel=t.kernel)
            del t
        print(json.dumps(row), flush=True)
        rows.append(row)
    print("\n| N | CG iterations | s to tol | ms / iteration | bound 1.3 x 5.5 x step | single step ms | error % |"
          " stepper s | stepper iterations | stepper error % |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['n']} | {r['iterations']} | {r['seconds']:.3f} | {r['ms_per_iteration']:.3f} | {r['bound_ms']:.3f} |"
              f" {r['single_step_ms']:.4f} | {r['error_percent']:.3e} | {r.get('stepper_seconds', float('nan')):.2f} |"
              f" {r.get('stepper_iterations', '-')} | {r.get('stepper_error_percent', float('nan')):.3f} |")


if __name__ == "__main__":
    main()
