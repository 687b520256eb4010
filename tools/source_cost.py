#!/usr/bin/env python3
"""Cost of the heat source: the fp64 K-step interior sweep of a 1024^3 grid
(a 1022^3 box) timed by Solver.profile_sweeps without a source, with one
(set_source: the solver re-times its kernels and picks the source forms) and
again after clear_source.  Prints the rates and the time ratio; --json PATH
also writes them.   python tools/source_cost.py [--grid N] [--json PATH]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, default=1024)
ap.add_argument("--json", default="")
args = ap.parse_args()
os.environ.setdefault("HEAT3D_RUNTIME", "rocm")
import numpy as np
import heat3d_amd
from heat3d_amd import HeatSolver

N = args.grid
out = {}
s = HeatSolver((N, N, N), 100000, 0.0, backend="hip", device=0)
s.initialize()
K = s.native.temporal_steps
pts = float(N - 2) ** 3
def measure(tag):
    rows = []
    for rep in range(3):
        p = dict(s.native.profile_sweeps(14))
        s.synchronize()
        rows.append(p["interior_ms"])
    out[tag] = {"kernel": s.kernel, "K": K, "interior_ms": rows, "glups_best": pts * K / (min(rows) * 1e-3) / 1e9,
                "monotone_check": bool(s.native.monotone_check), "sweep_costs": dict(s.native.sweep_costs)}
    print(tag, json.dumps(out[tag]), flush=True)
measure("no_source_a")
t0 = time.time()
q = s.model.sine_source(0.25)
s.set_source(q)
print("set_source seconds", time.time() - t0, flush=True)
del q
measure("source")
s.clear_source()
measure("no_source_b")
a = min(out["no_source_a"]["interior_ms"] + out["no_source_b"]["interior_ms"])
b = min(out["source"]["interior_ms"])
out["ratio_time_source_over_none"] = b / a
print(json.dumps(out))
if args.json:
    json.dump(out, open(args.json, "w"), indent=1)
