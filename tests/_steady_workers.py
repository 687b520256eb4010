"""Workers of the multi-process steady-solve tests (gloo bootstrap, socket transport)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)


def _solve(rank, world, port, outdir, name, decomp, backend, comm_name):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method="env://", rank=rank, world_size=world)
    import heat3d_amd

    import _steady_cases as sc

    s, r, T = sc.solve_and_check(heat3d_amd, name, backend, comm="socket", decomp=decomp)
    assert s.native.comm_name == comm_name, s.native.comm_name
    # a repeated solve: the same bits
    s2, r2, T2 = sc.solve_and_check(heat3d_amd, name, backend, comm="socket", decomp=decomp)
    assert r2["iterations"] == r["iterations"] and r2["residual"] == r["residual"]
    if rank == 0:
        assert np.array_equal(T, T2)
    with open(os.path.join(outdir, f"steady{rank}.json"), "w") as f:
        json.dump({k: v for k, v in r.items() if k != "seconds"}, f)
    dist.barrier()
    dist.destroy_process_group()


def steady_cpu_worker(rank, world, port, outdir, name, decomp):
    _solve(rank, world, port, outdir, name, decomp, "cpu", "socket")


def steady_gpu_worker(rank, world, port, outdir, name, decomp):
    """Two processes on the one GPU, halos and the pairs' all-reduce host-staged."""
    _solve(rank, world, port, outdir, name, decomp, "hip", "staged-socket")
