"""The heat balance across processes (socket transport, 2 and 4 ranks): the
(hi, lo) pairs are all-reduced as plain float64 sums, so the result is within
tol + P * 2^-53 * sum|term| of the fsum reference (the issue's bound for the
pair all-reduce); minimum, maximum and the non-finite count are exact; every
rank holds the same dict."""
import json
import math

import numpy as np
import pytest
import torch.multiprocessing as mp

from conftest import free_port
from _heat_balance_workers import balance_worker

FACES = ("x-", "x+", "y-", "y+", "z-", "z+")
WALLS = dict(insulated="x+,z-", convective={"x-": 0.5, "y+": 0.3}, ambient=1.75)


@pytest.mark.parametrize("world,decomp,dtype", [(2, (1, 1, 2), "fp64"), (4, (2, 2, 1), "fp32")])
def test_processes_match_reference(h3d, tmp_path, world, decomp, dtype):
    from heat3d_amd.utils.metrics import heat_balance_reference

    N, seed = (11, 10, 37), 41
    port = free_port()
    mp.start_processes(balance_worker, args=(world, port, str(tmp_path), N, decomp, dtype, WALLS, seed),
                       nprocs=world, join=True, start_method="spawn")
    got = [json.loads((tmp_path / f"balance{r}.json").read_text()) for r in range(world)]
    assert all(g == got[0] for g in got)
    rng = np.random.default_rng(seed)
    T, q, c = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N), rng.uniform(0.25, 1, N)
    ref = heat_balance_reference(T, h3d.HeatEquation3D(N), source=q, conductivity=c, dtype=dtype, **WALLS)
    for key in ("heat", "source_power") + FACES:
        g = got[0]["flow"][key] if key in FACES else got[0][key]
        r = ref["flow"][key] if key in FACES else ref[key]
        n, sabs = ref["terms"][key]
        bound = math.ulp(r) + n * 2.0 ** -100 * sabs + world * 2.0 ** -53 * sabs
        print(f"{world} ranks {dtype} {key}: got {g!r} ref {r!r} diff {abs(g - r):.3e} bound {bound:.3e}")
        assert abs(g - r) <= bound, key
    for key in ("t_min", "t_max", "nonfinite"):
        assert got[0][key] == ref[key], key
    assert got[0]["flow"]["x+"] == 0.0 and got[0]["flow"]["z-"] == 0.0
