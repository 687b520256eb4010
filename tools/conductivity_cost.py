#!/usr/bin/env python3
"""Cost of a conductivity field: ms per step of a 1024^3 grid, fp64 and fp32,
for the single-step tile kernel plain (--temporal 1), with a conductivity c,
with c and a heat source q, and for the default K-step schedule without c.
Each case replays its hipGraphs: `--steps` steps timed after an untimed
round of the same length, best of `--reps`.  Prints the ratios against the
traffic model (1.5x and 2x the plain single step); --json PATH also writes them.
  python tools/conductivity_cost.py [--grid N] [--steps S] [--dtypes fp64,fp32] [--json PATH]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, default=1024)
ap.add_argument("--steps", type=int, default=24)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--dtypes", default="fp64,fp32")
ap.add_argument("--json", default="")
args = ap.parse_args()
os.environ.setdefault("HEAT3D_RUNTIME", "rocm")
import numpy as np
import heat3d_amd
from heat3d_amd import HeatSolver

N = args.grid
out = {}

def timed(s):
    s.prepare_steps(args.steps)
    s.step(args.steps)
    s.synchronize()
    best = 1e30
    for _ in range(args.reps):
        t0 = time.perf_counter()
        s.step(args.steps)
        s.synchronize()
        best = min(best, time.perf_counter() - t0)
    return 1e3 * best / args.steps

for dt in args.dtypes.split(","):
    r = {}
    s = HeatSolver((N, N, N), 10 ** 9, 0.0, dtype=dt, backend="hip", device=0)
    s.initialize()
    r["sweeps_ms"] = timed(s)
    r["sweeps_kernel"] = s.kernel
    s = None
    s = HeatSolver((N, N, N), 10 ** 9, 0.0, dtype=dt, backend="hip", device=0, extra_args=["--temporal", "1"])
    s.initialize()
    r["single_ms"] = timed(s)
    r["single_kernel"] = s.kernel
    t0 = time.time()
    c = s.model.layered_conductivity(0.25, 1.0)
    s.set_conductivity(c)
    r["set_conductivity_s"] = time.time() - t0
    del c
    r["cond_ms"] = timed(s)
    s.set_source(np.zeros((N, N, N)))
    r["cond_source_ms"] = timed(s)
    s.clear_source()
    s.clear_conductivity()
    r["single_again_ms"] = timed(s)
    s = None
    base = min(r["single_ms"], r["single_again_ms"])
    r["ratio_cond"] = r["cond_ms"] / base          # traffic model: 1.5
    r["ratio_cond_source"] = r["cond_source_ms"] / base  # traffic model: 2.0
    r["ratio_cond_over_sweeps"] = r["cond_ms"] / r["sweeps_ms"]
    out[dt] = r
    print(dt, json.dumps(r), flush=True)
if args.json:
    json.dump(out, open(args.json, "w"), indent=1)
