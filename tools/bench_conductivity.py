#!/usr/bin/env python3
"""Step time of a composite-material run (set_conductivity) with the single-step
schedule (flag off) against the K-step tv sweeps (--conductivity-sweeps).

For every dtype and grid size, and for flag off and on: a fresh solver, a seeded
random relative conductivity c in [0.05, 1], a warm-up, then `--reps` timed
windows of step(`--steps`) (graphs prepared before the window, the device
synchronised around it).  The configurations of one (dtype, size) alternate
off / on for `--rounds` rounds so that clock drift shows up as a spread between
rounds instead of a bias of one side.  Prints one JSON line:

  {"results": [{"dtype", "n", "off": {...}, "on": {...}, "ratio_off_over_on"}, ...]}

with, per side, the kernel name, the median / min / max ms per step over all
windows, and GLUPS at the median.  ratio > 1: the sweeps are faster.

  python tools/bench_conductivity.py [--sizes 512,1024] [--dtypes fp64,fp32]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_config(h3d, n, dtype, sweeps, c, warmup, steps, reps):
    ext = h3d.native()
    s = h3d.HeatSolver((n, n, n), 1 << 40, 0.0, dtype=dtype, backend="hip", device=0, conductivity_sweeps=sweeps)
    s.set_conductivity(c)
    assert s.native.sweeps_active == sweeps
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
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--dtypes", default="fp64,fp32")
    ap.add_argument("--steps", type=int, default=60, help="steps per timed window (a multiple of 6: whole sweeps)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5, help="timed windows per solver")
    ap.add_argument("--rounds", type=int, default=2, help="off / on alternations per (dtype, size)")
    ap.add_argument("--seed", type=int, default=5)
    args = ap.parse_args()
    if "torch" not in sys.modules:
        os.environ.setdefault("HEAT3D_RUNTIME", "rocm")
    import numpy as np

    import heat3d_amd as h3d

    results = []
    for n in (int(v) for v in args.sizes.split(",")):
        c = np.random.default_rng(args.seed).uniform(0.05, 1.0, (n, n, n))
        for dtype in args.dtypes.split(","):
            side = {False: {"ms": []}, True: {"ms": []}}
            for _ in range(args.rounds):
                for sweeps in (False, True):
                    kernel, ms = time_config(h3d, n, dtype, sweeps, c, args.warmup, args.steps, args.reps)
                    side[sweeps]["kernel"] = kernel
                    side[sweeps]["ms"] += ms
            row = {"dtype": dtype, "n": n, "steps": args.steps}
            for sweeps, key in ((False, "off"), (True, "on")):
                ms = side[sweeps]["ms"]
                med = statistics.median(ms)
                row[key] = {"kernel": side[sweeps]["kernel"], "ms_per_step_median": round(med, 5),
                            "ms_per_step_min": round(min(ms), 5), "ms_per_step_max": round(max(ms), 5),
                            "windows": len(ms), "glups_median": round((n - 2) ** 3 / med / 1e6, 1)}
            row["ratio_off_over_on"] = round(row["off"]["ms_per_step_median"] / row["on"]["ms_per_step_median"], 4)
            results.append(row)
            print(f"bench_conductivity: {json.dumps(row)}", file=sys.stderr, flush=True)
    print(json.dumps({"results": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
