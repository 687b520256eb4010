#!/usr/bin/env python3
"""Step time of a run with a heat capacity (set_capacity) against the
conductivity single step it is modelled on.

For every dtype and grid size three single-step configurations, each a fresh
solver: "cond" (set_conductivity alone: the stencil_var kernels, the yardstick),
"cap" (set_capacity alone: uniform material + capacity, three fields per step
like "cond") and "cond+cap" (both: four fields per step).  A seeded random
relative conductivity c in [0.05, 1], the capacity rc = 1 / c in [1, 20]; a
warm-up, then `--reps` timed chunks of step(`--steps`) (graphs prepared before
the chunk, the device synchronised around it).  The configurations alternate
for `--rounds` rounds so that clock drift shows as a spread between rounds.
Prints one JSON line:

  {"results": [{"dtype", "n", "cond": {...}, "cap": {...}, "cond+cap": {...},
                "cap_over_cond", "condcap_over_cond"}, ...]}

with, per configuration, the kernel name and the median / min / max ms per step
over all chunks.  The traffic model expects cap_over_cond <= 1 and
condcap_over_cond <= 4/3, each with 10 % for the spread between chunks.

  python tools/bench_capacity.py [--sizes 512,1024] [--dtypes fp64,fp32]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = ("cond", "cap", "cond+cap")


def time_config(h3d, n, dtype, config, c, rc, warmup, steps, reps):
    ext = h3d.native()
    s = h3d.HeatSolver((n, n, n), 1 << 40, 0.0, dtype=dtype, backend="hip", device=0)
    if "cond" in config:
        s.set_conductivity(c)
    if "cap" in config:
        s.set_capacity(rc)
    assert not s.native.sweeps_active
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
    ap.add_argument("--steps", type=int, default=20, help="steps per timed chunk")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5, help="timed chunks per solver")
    ap.add_argument("--rounds", type=int, default=1, help="alternations of the configurations per (dtype, size)")
    ap.add_argument("--seed", type=int, default=5)
    args = ap.parse_args()
    if "torch" not in sys.modules:
        os.environ.setdefault("HEAT3D_RUNTIME", "rocm")
    import numpy as np

    import heat3d_amd as h3d

    results = []
    for n in (int(v) for v in args.sizes.split(",")):
        c = np.random.default_rng(args.seed).uniform(0.05, 1.0, (n, n, n))
        rc = 1.0 / c
        for dtype in args.dtypes.split(","):
            side = {k: {"ms": []} for k in CONFIGS}
            for _ in range(args.rounds):
                for config in CONFIGS:
                    kernel, ms = time_config(h3d, n, dtype, config, c, rc, args.warmup, args.steps, args.reps)
                    side[config]["kernel"] = kernel
                    side[config]["ms"] += ms
            row = {"dtype": dtype, "n": n, "steps": args.steps}
            for config in CONFIGS:
                ms = side[config]["ms"]
                med = statistics.median(ms)
                row[config] = {"kernel": side[config]["kernel"], "ms_per_step_median": round(med, 5),
                               "ms_per_step_min": round(min(ms), 5), "ms_per_step_max": round(max(ms), 5),
                               "chunks": len(ms), "glups_median": round((n - 2) ** 3 / med / 1e6, 1)}
            base = row["cond"]["ms_per_step_median"]
            row["cap_over_cond"] = round(row["cap"]["ms_per_step_median"] / base, 4)
            row["condcap_over_cond"] = round(row["cond+cap"]["ms_per_step_median"] / base, 4)
            results.append(row)
            print(f"bench_capacity: {json.dumps(row)}", file=sys.stderr, flush=True)
    print(json.dumps({"results": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
