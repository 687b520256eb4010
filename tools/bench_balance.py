#!/usr/bin/env python3
"""Cost of HeatSolver.heat_balance() on one MI355X (profiles/heat_balance.md).

Per dtype (fp64, fp32) at N^3 (default 1024), plain and with a source and a
conductivity, the median of 20 calls after 3 warm-up calls of
  * heat_balance()            the one-pass double-double reduction,
  * the bandwidth_probe read  kernel (16 B per lane, 2048 blocks) over the bytes
                              the balance reads: one launch per field read,
  * compute_error()           the one-pass reduction the solver already had,
each timed by the host clock around the call and a device synchronise (the two
solver calls synchronise themselves), with the bandwidth the time implies.
One JSON line per case.  Each dtype runs in a child process of its own under
its own time limit, and nothing more is started after a child that failed.

  python tools/bench_balance.py [--n 1024] [--dtypes fp64,fp32] [--json-out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, CALLS = 3, 20


def timed(fn, sync):
    for _ in range(WARMUP):
        fn()
    sync()
    ts = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts)


def child(n: int, dtype: str, backend: str) -> None:
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import heat3d_amd
    from heat3d_amd import HeatSolver

    ext = heat3d_amd.native()
    N = (n, n, n)
    esize = 8 if dtype == "fp64" else 4
    s = HeatSolver(N, iter_max=10, eps=0.0, dtype=dtype, backend=backend, device=0,
                   insulated="x+,z-", convective={"x-": 0.5, "y+": 0.3}, ambient=1.75)
    s.initialize()
    s.step(3)  # a field that is not the initial zeros
    s.synchronize()
    gpu = backend == "hip"
    sync = (lambda: ext.device_synchronize(0)) if gpu else (lambda: None)
    points = s.interior_points
    for case in ("plain", "source+conductivity"):
        if case != "plain":
            s.set_source(np.ones(N))
            s.set_conductivity(s.model.layered_conductivity(0.25, 1.0))
        # T, and S at every point; Ch is read on wall-adjacent rows and planes only
        fields = 1 if case == "plain" else 2
        nbytes = points * esize  # per field read
        bal, bal_min = timed(s.heat_balance, sync)
        err, _ = timed(s.error_percent, sync)
        row = {"n": n, "dtype": dtype, "case": case, "bytes": fields * nbytes, "balance_ms": bal * 1e3,
               "balance_min_ms": bal_min * 1e3, "balance_tbps": fields * nbytes / bal / 1e12,
               "compute_error_ms": err * 1e3, "compute_error_tbps": nbytes / err / 1e12,
               "balance": {k: v for k, v in s.heat_balance().items() if k != "flow"}}
        if gpu:
            buf = torch.zeros(nbytes // 16 * 16, dtype=torch.uint8, device="cuda:0")
            sink = torch.zeros(4, dtype=torch.int32, device="cuda:0")

            def probe():
                for _ in range(fields):
                    ext.hip.bandwidth_probe(1, buf.data_ptr(), sink.data_ptr(), buf.numel(), 2048, 0)

            rd, _ = timed(probe, sync)
            row.update(read_probe_ms=rd * 1e3, read_probe_tbps=fields * nbytes / rd / 1e12,
                       balance_over_read=bal / rd)
            del buf
        print(json.dumps(row), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--dtypes", default="fp64,fp32")
    ap.add_argument("--backend", default="hip", choices=["hip", "cpu"])
    ap.add_argument("--timeout", type=float, default=420.0, help="seconds per dtype (one child process each)")
    ap.add_argument("--json-out", default="")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.n, a.child, a.backend)
        return 0
    rows = []
    for dtype in a.dtypes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--backend", a.backend, "--child", dtype]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"bench_balance: {dtype} ran into its time limit of {a.timeout:g} s; stopping", file=sys.stderr)
            return 124
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            print(f"bench_balance: {dtype} failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
        rows += [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    if a.json_out:
        with open(a.json_out, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
