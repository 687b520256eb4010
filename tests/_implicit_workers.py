"""Workers of the multi-process implicit-step tests (gloo bootstrap, socket transport)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)


def _steps(rank, world, port, outdir, name, decomp, backend, comm_name, m, theta):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method="env://", rank=rank, world_size=world)
    import heat3d_amd

    import _implicit_checks as ic

    out = []
    for _ in range(2):  # (a repeated call: the same bits)
        case = ic.make_case(heat3d_amd, name, backend, cap=True, comm="socket", decomp=decomp)
        assert case.s.native.comm_name == comm_name, case.s.native.comm_name
        r = case.s.step_implicit(1, m, theta, tol=ic.TOL)
        out.append((ic.report(r), case.s.gather()))
    assert out[0][0] == out[1][0]
    if rank == 0:
        assert np.array_equal(out[0][1], out[1][1])
        np.save(os.path.join(outdir, "field.npy"), out[0][1])
    with open(os.path.join(outdir, f"implicit{rank}.json"), "w") as f:
        json.dump(out[0][0], f)
    dist.barrier()
    dist.destroy_process_group()


def implicit_cpu_worker(rank, world, port, outdir, name, decomp, m, theta):
    _steps(rank, world, port, outdir, name, decomp, "cpu", "socket", m, theta)


def implicit_gpu_worker(rank, world, port, outdir, name, decomp, m, theta):
    """Two processes on the one GPU, halos and the pairs' all-reduce host-staged."""
    _steps(rank, world, port, outdir, name, decomp, "hip", "staged-socket", m, theta)
