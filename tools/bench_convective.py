#!/usr/bin/env python3
"""Step time of a run with convective walls (--convective all=0.5 --ambient
0.25): the convective-form K = 3 sweeps against the insulated-wall sweeps
(--insulated all) on the same box and against the single-step convective
schedule (--temporal 1: the tile kernel on wall planes refreshed with the ghost
values).

For every (size, dtype) and each of the three configurations: a fresh solver, a
warm-up, then `--reps` timed windows of step(`--steps`) (graphs prepared before
the window, the device synchronised around it).  The configurations alternate
for `--rounds` rounds so that clock drift shows up as a spread between rounds
instead of a bias of one side.  Prints one JSON line:

  {"results": [{"dtype", "n", "insulated": {...}, "convective": {...}, "convective_single": {...},
                "convective_over_insulated", "single_over_convective"}, ...]}

with, per side, the kernel name and the median / min / max ms per step over all
windows.  convective_over_insulated near 1: the ghost's extra FMA runs in
wall-touching waves only.  single_over_convective > 1: the sweeps are faster
than single steps (what makes them the default).

  python tools/bench_convective.py [--cases 1024:fp64,512:fp64,1024:fp32]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (insulated, convective, --temporal)
CONFIGS = {"insulated": ("all", None, 3), "convective": (None, "all=0.5", 3), "convective_single": (None, "all=0.5", 1)}
AMBIENT = 0.25


def time_config(h3d, n, dtype, faces, conv, temporal, warmup, steps, reps):
    ext = h3d.native()
    s = h3d.HeatSolver((n, n, n), 1 << 40, 0.0, dtype=dtype, backend="hip", device=0, insulated=faces, convective=conv,
                       ambient=AMBIENT if conv else 0.0,
                       extra_args=["--temporal", str(temporal)])
    s.initialize()
    assert s.native.sweeps_active == (temporal > 1)
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
    ap.add_argument("--rounds", type=int, default=2, help="alternations of the three configurations per case")
    args = ap.parse_args()
    if "torch" not in sys.modules:
        os.environ.setdefault("HEAT3D_RUNTIME", "rocm")

    import heat3d_amd as h3d

    results = []
    for case in args.cases.split(","):
        n, dtype = int(case.split(":")[0]), case.split(":")[1]
        side = {k: {"ms": []} for k in CONFIGS}
        for _ in range(args.rounds):
            for key, (faces, conv, temporal) in CONFIGS.items():
                kernel, ms = time_config(h3d, n, dtype, faces, conv, temporal, args.warmup, args.steps, args.reps)
                side[key]["kernel"] = kernel
                side[key]["ms"] += ms
        row = {"dtype": dtype, "n": n, "steps": args.steps}
        for key in CONFIGS:
            ms = side[key]["ms"]
            med = statistics.median(ms)
            row[key] = {"kernel": side[key]["kernel"], "ms_per_step_median": round(med, 5),
                        "ms_per_step_min": round(min(ms), 5), "ms_per_step_max": round(max(ms), 5), "windows": len(ms)}
        row["convective_over_insulated"] = round(row["convective"]["ms_per_step_median"] /
                                                 row["insulated"]["ms_per_step_median"], 4)
        row["single_over_convective"] = round(row["convective_single"]["ms_per_step_median"] /
                                              row["convective"]["ms_per_step_median"], 4)
        results.append(row)
        print(f"bench_convective: {json.dumps(row)}", file=sys.stderr, flush=True)
    print(json.dumps({"results": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
