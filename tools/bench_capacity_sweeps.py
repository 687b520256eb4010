#!/usr/bin/env python3
"""Step time of a run with a heat capacity and a conductivity field: the
single-step schedule (flag off: the kernels of stencil_cap.hip, behind walls on
refreshed wall planes) against the tc sweeps (--capacity-sweeps) of the same
build, for a composite body with a seeded random relative conductivity c in
[0.05, 1] and a seeded random relative heat capacity rc in [1, 9]:

  walls 0: every face Dirichlet;
  walls 1: x-, x+, z-, z+ insulated, y- convective (0.5, ambient 0.25), y+ Dirichlet;

each with and without a uniform heat source.

For every (size, dtype, walls, source) and each side: a fresh solver, the
fields set, a warm-up, then `--reps` timed windows of step(`--steps`) (graphs
prepared before the window, the device synchronised around it).  The two sides
alternate for `--rounds` rounds so that clock drift shows up as a spread between
rounds instead of a bias of one side.  Prints one JSON line:

  {"results": [{"dtype", "n", "walls", "source", "off": {...}, "on": {...}, "off_over_on"}, ...]}

with, per side, the kernel name and the median / min / max ms per step over all
windows.  off_over_on > 1: the sweeps are faster than the single steps.

  python tools/bench_capacity_sweeps.py [--cases 512:fp64,512:fp32,1024:fp64,1024:fp32] [--walls 0,1] [--sources 0,1]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WALLS = dict(insulated="x-,x+,z-,z+", convective={"y-": 0.5}, ambient=0.25)
Q = 3.0
SEED = 5


def time_config(h3d, n, dtype, flag, walls, c, rc, q, warmup, steps, reps):
    ext = h3d.native()
    s = h3d.HeatSolver((n, n, n), 1 << 40, 0.0, dtype=dtype, backend="hip", device=0, capacity_sweeps=flag,
                       extra_args=["--temporal", "3"], **(WALLS if walls else {}))
    s.initialize()
    s.set_conductivity(c)
    s.set_capacity(rc)
    if q is not None:
        s.set_source(q)
    assert s.native.has_capacity and s.native.sweeps_active == flag
    s.step(warmup)
    s.prepare_steps(steps)
    s.synchronize()
    ext.device_synchronize(0)
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        s.step(steps)
        s.synchronize()
        ext.device_synchronize(0)
        ms.append(1e3 * (time.perf_counter() - t0) / steps)
    st = s.state()
    assert st["iter"] == warmup + reps * steps and not st["fault"], st
    return s.kernel, ms


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="512:fp64,512:fp32,1024:fp64,1024:fp32",
                    help="grid size N (N - 2 interior points per axis) : dtype")
    ap.add_argument("--walls", default="0,1", help="0: every face Dirichlet, 1: the insulated / convective set")
    ap.add_argument("--sources", default="0,1", help="0: without a heat source, 1: with a uniform one")
    ap.add_argument("--steps", type=int, default=60, help="steps per timed window (a multiple of 6: whole sweeps)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5, help="timed windows per solver")
    ap.add_argument("--rounds", type=int, default=2, help="alternations of the two sides per case")
    args = ap.parse_args()
    if "torch" not in sys.modules:
        os.environ.setdefault("HEAT3D_RUNTIME", "rocm")

    import numpy as np

    import heat3d_amd as h3d

    results = []
    c, rc, q, cn = None, None, None, 0
    for case in args.cases.split(","):
        n, dtype = int(case.split(":")[0]), case.split(":")[1]
        if n != cn:  # the global fields, built once per size
            rng = np.random.default_rng(SEED)
            c, rc = rng.uniform(0.05, 1.0, (n, n, n)), rng.uniform(1.0, 9.0, (n, n, n))
            q, cn = np.full((n, n, n), Q), n
        for walls in (int(v) for v in args.walls.split(",")):
            for src in (int(v) for v in args.sources.split(",")):
                side = {k: {"ms": []} for k in ("off", "on")}
                for _ in range(args.rounds):
                    for key in ("off", "on"):
                        kernel, ms = time_config(h3d, n, dtype, key == "on", walls, c, rc, q if src else None,
                                                 args.warmup, args.steps, args.reps)
                        side[key]["kernel"] = kernel
                        side[key]["ms"] += ms
                row = {"dtype": dtype, "n": n, "walls": bool(walls), "source": bool(src), "steps": args.steps}
                for key in ("off", "on"):
                    ms = side[key]["ms"]
                    row[key] = {"kernel": side[key]["kernel"], "ms_per_step_median": round(statistics.median(ms), 5),
                                "ms_per_step_min": round(min(ms), 5), "ms_per_step_max": round(max(ms), 5),
                                "windows": len(ms)}
                row["off_over_on"] = round(row["off"]["ms_per_step_median"] / row["on"]["ms_per_step_median"], 4)
                results.append(row)
                print(f"bench_capacity_sweeps: {json.dumps(row)}", file=sys.stderr, flush=True)
    print(json.dumps({"results": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
