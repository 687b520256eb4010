"""Worker of the multi-process heat-balance test (gloo bootstrap, socket transport, CPU backend)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def balance_worker(rank, world, port, outdir, N, decomp, dtype, walls, seed):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method="env://", rank=rank, world_size=world)
    import heat3d_amd

    rng = np.random.default_rng(seed)
    T, q, c = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N), rng.uniform(0.25, 1, N)
    s = heat3d_amd.HeatSolver(N, 100, 0.0, backend="cpu", decomp=decomp, dtype=dtype, threads=1, **walls)
    assert s.native.comm_name == "socket"
    s.set_field(T)
    s.set_source(q)
    s.set_conductivity(c)
    b = s.heat_balance()
    assert s.heat_balance() == b
    with open(os.path.join(outdir, f"balance{rank}.json"), "w") as f:
        json.dump(b, f)
    dist.barrier()
    dist.destroy_process_group()
