#!/usr/bin/env python3
"""Step time of a run with a heat source behind walls: the default single-step
schedule (flag off: the tile kernel with a source on refreshed wall planes)
against the K = 3 sweeps of walls and source together (--wall-source-sweeps),
for an insulated-only face set (--insulated all) and a convective one
(--convective all=0.5 --ambient 0.25), with a uniform source.

For every (size, dtype, face set) and each side: a fresh solver, the source set,
a warm-up, then `--reps` timed windows of step(`--steps`) (graphs prepared before
the window, the device synchronised around it).  The two sides alternate for
`--rounds` rounds so that clock drift shows up as a spread between rounds
instead of a bias of one side.  Prints one JSON line:

  {"results": [{"dtype", "n", "faces", "off": {...}, "on": {...}, "off_over_on"}, ...]}

with, per side, the kernel name and the median / min / max ms per step over all
windows.  off_over_on > 1: the sweeps are faster than the single steps.

  python tools/bench_wall_source.py [--cases 1024:fp64,512:fp64,1024:fp32]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (insulated, convective)
FACES = {"insulated": ("all", None), "convective": (None, "all=0.5")}
AMBIENT = 0.25
Q = 3.0


def time_config(h3d, n, dtype, faces, conv, flag, q, warmup, steps, reps):
    ext = h3d.native()
    s = h3d.HeatSolver((n, n, n), 1 << 40, 0.0, dtype=dtype, backend="hip", device=0, insulated=faces, convective=conv,
                       ambient=AMBIENT if conv else 0.0, wall_source_sweeps=flag, extra_args=["--temporal", "3"])
    s.initialize()
    s.set_source(q)
    assert s.native.sweeps_active == flag
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
    ap.add_argument("--cases", default="1024:fp64,512:fp64,1024:fp32", help="grid size N (N - 2 interior points per axis) : dtype")
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
    q, qn = None, 0
    for case in args.cases.split(","):
        n, dtype = int(case.split(":")[0]), case.split(":")[1]
        if n != qn:
            q, qn = np.full((n, n, n), Q), n  # the global source, built once per size
        for name, (faces, conv) in FACES.items():
            side = {k: {"ms": []} for k in ("off", "on")}
            for _ in range(args.rounds):
                for key in ("off", "on"):
                    kernel, ms = time_config(h3d, n, dtype, faces, conv, key == "on", q, args.warmup, args.steps, args.reps)
                    side[key]["kernel"] = kernel
                    side[key]["ms"] += ms
            row = {"dtype": dtype, "n": n, "faces": name, "steps": args.steps}
            for key in ("off", "on"):
                ms = side[key]["ms"]
                row[key] = {"kernel": side[key]["kernel"], "ms_per_step_median": round(statistics.median(ms), 5),
                            "ms_per_step_min": round(min(ms), 5), "ms_per_step_max": round(max(ms), 5), "windows": len(ms)}
            row["off_over_on"] = round(row["off"]["ms_per_step_median"] / row["on"]["ms_per_step_median"], 4)
            results.append(row)
            print(f"bench_wall_source: {json.dumps(row)}", file=sys.stderr, flush=True)
    print(json.dumps({"results": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
