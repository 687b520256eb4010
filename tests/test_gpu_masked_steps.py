"""The step forms of the lean K = 4 edge-role sweep beside the mask-free one
(stencil_tbl_kernel.inc): the z-masked step of y-free waves in tiles that have
columns outside the z update range, the dead fill stages the masked step skips,
and padded chunks left early.  Fields and each sweep's residual are bitwise
those of K single steps of the tile kernel.  tests/_masked_steps.py lists the
shapes; test_masked_steps_cpu.py says which form each of them reaches."""
import math

import numpy as np
import pytest
import torch

import _masked_steps as ms
import _value_fields as vf

pytestmark = pytest.mark.gpu

K = ms.K
D = (0.06, 0.05, 0.04)

_oracle = {}


def _reference(ops, gpu, key, host):
    """From the host field, by single steps of the tile kernel: the device copy
    of the input and the fields after K and 2K steps with the residuals of steps
    K and 2K (computed once per key)."""
    if key not in _oracle:
        n = tuple(host.n)
        src = ops.PaddedField(n, dtype=torch.float64, device=gpu)
        src.flat.copy_(host.flat)
        a = ops.PaddedField(n, dtype=torch.float64, device=gpu)
        a.flat.copy_(host.flat)
        b = ops.PaddedField(n, dtype=torch.float64, device=gpu)
        b.flat.copy_(host.flat)  # the same Dirichlet shell in both buffers
        fields, resid = [], []
        cur, nxt = a, b
        for step in range(2 * K):
            st = ops.new_state(gpu)
            ops.ftcs_step(cur, nxt, D, kernel="tile", state=st, slot=0)
            torch.cuda.synchronize()
            cur, nxt = nxt, cur
            if step % K == K - 1:
                fields.append(cur.owned().clone())
                resid.append(ops.residual_from_state(st, 0))
        _oracle[key] = (src, fields, resid)
    return _oracle[key]


def _random(ops, n):
    g = torch.Generator().manual_seed(7)
    host = ops.PaddedField(n, dtype=torch.float64)
    host.ghosted().copy_(torch.rand(tuple(v + 2 for v in n), generator=g, dtype=torch.float64))
    return host


def _sweeps(ops, gpu, key, host, spec):
    """Two sweeps of `spec` against the reference: the stored field bit for bit
    and the residual of each sweep (NaN where the reference's is)."""
    src, fields, resid = _reference(ops, gpu, key, host)
    n = tuple(host.n)
    a = ops.PaddedField(n, dtype=torch.float64, device=gpu)
    b = ops.PaddedField(n, dtype=torch.float64, device=gpu)
    a.flat.copy_(src.flat)
    b.flat.copy_(src.flat)
    b.owned().fill_(-3.0)
    cur, nxt = a, b
    got_resid = []
    for i in range(2):
        st = ops.new_state(gpu)
        ops.ftcs_step2(cur, nxt, D, kernel=spec, state=st, slot=0)
        torch.cuda.synchronize()
        cur, nxt = nxt, cur
        report = vf.bits_differ(cur.owned().cpu(), fields[i].cpu())
        assert report is None, f"{spec} {n} sweep {i + 1}: {report}"
        r = ops.residual_from_state(st, K - 1)
        got_resid.append(r)
        if math.isnan(resid[i]):
            assert math.isnan(r), (spec, n, i, r)
        else:
            assert r == resid[i], (spec, n, i, r, resid[i])
    return got_resid


@pytest.mark.parametrize("name", list(ms.SHAPES))
def test_masked_steps_bitwise(h3d, gpu, name):
    n, L = ms.SHAPES[name]
    _sweeps(h3d.ops, gpu, n, _random(h3d.ops, n), ms.spec(L))


@pytest.mark.parametrize("name", ["z-overhang", "yz-overhang", "z-exact"])
def test_masked_steps_planned_segments(h3d, gpu, name):
    """The spec as the solver passes it (field L = 0: the x plan's segments)."""
    n, _ = ms.SHAPES[name]
    _sweeps(h3d.ops, gpu, n, _random(h3d.ops, n), ms.SPEC)


# one NaN in the second, overhanging tile column, in a row of an interior wave
# and in the first / last updated column of the tile (the z select's two ends)
@pytest.mark.parametrize("z", [ms.ZS, ms.ZS + 4, 2])
def test_nan_through_the_z_masked_step(h3d, gpu, z):
    n, L = ms.SHAPES["z-overhang"]
    pos = (7, 20, z)
    host = vf.spike(h3d.ops, "nan", pos, n, torch.float64, 1)
    assert int(host.flat.isnan().sum()) == 1
    got = _sweeps(h3d.ops, gpu, (n, pos), host, ms.spec(L))
    # the NaN is stored by the first sweep: both residual slots are poisoned
    assert all(math.isnan(r) for r in got), got
    assert all(math.isnan(r) for r in _oracle[(n, pos)][2])


def test_deep_halo_slabs_solver(h3d, gpu):
    """Two x slabs as virtual ranks: K-deep x halos, so the box starts and ends
    inside the update range and the widened count bounds of the fill stages
    are exercised; the solver equals the single-step run bit for bit."""
    n = (24, 47, 61)
    a = h3d.HeatSolver(n, 10 ** 6, 1e-4, backend="hip", virtual_ranks=2, decomp=(2, 1, 1),
                       extra_args=["--kernel2", ms.SPEC])
    b = h3d.HeatSolver(n, 10 ** 6, 1e-4, backend="hip", extra_args=["--temporal", "1"])
    a.initialize()
    assert a.native.temporal_blocking and a.native.temporal_steps == K
    ra, rb = a.run(), b.run()
    assert ra["converged"] and ra["conv_iter"] == rb["conv_iter"], (ra, rb)
    assert ra["last_residual"] == rb["last_residual"]
    assert np.array_equal(a.gather(), b.gather())
