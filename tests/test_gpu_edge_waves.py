"""The edge role of the lean K-step sweep (stencil_tbl_kernel.inc, spec field
9): a tile's two halo waves evaluate only the stages inside the tile's cone
and, with field 9 = 1 + E, own E more rows each.  Fields and the sweep's last
residual are bitwise those of K single steps of the tile kernel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 4
# fp64 K = 4, 12 waves of 4 rows, last residual only: 48-row tiles storing 40
# rows (E = 0) and 52-row tiles storing 44 (E = 2)
SPECS = {"tl4:1:4:1:12:0:3:66:0:1": 40, "tl4:1:4:1:12:0:3:66:0:3": 44}
D = (0.06, 0.05, 0.04)


def _cases(stored):
    # (nx, ny, nz): i one tile on both Dirichlet faces (masked form); ii a seam
    # between two tiles, the second of one row; iii an interior tile, z seams;
    # iv fewer planes than the 2(K-1) + 6 of a pipeline fill and one unrolled chunk
    return {"i": (14, 10, 60), "ii": (20, stored + 3, 60), "iii": (20, 3 * stored, 120),
            "iv": (7, 2 * stored + 3, 60)}


_oracle = {}


def _reference(ops, gpu, n):
    """Input field and, by single steps of the tile kernel, the fields after K
    and 2K steps with the residuals of steps K and 2K (computed once per box)."""
    if n not in _oracle:
        g = torch.Generator().manual_seed(7)
        a = ops.PaddedField(n, dtype=torch.float64, device=gpu)
        host = ops.PaddedField(n, dtype=torch.float64)
        host.ghosted().copy_(torch.rand(tuple(v + 2 for v in n), generator=g, dtype=torch.float64))
        a.flat.copy_(host.flat)
        src = ops.PaddedField(n, dtype=torch.float64, device=gpu)
        src.flat.copy_(a.flat)
        b = ops.PaddedField(n, dtype=torch.float64, device=gpu)
        b.flat.copy_(a.flat)  # the same Dirichlet shell in both buffers
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
        _oracle[n] = (src, fields, resid)
    return _oracle[n]


def _sweeps(ops, gpu, n, spec):
    src, fields, resid = _reference(ops, gpu, n)
    a = ops.PaddedField(n, dtype=torch.float64, device=gpu)
    b = ops.PaddedField(n, dtype=torch.float64, device=gpu)
    a.flat.copy_(src.flat)
    b.flat.copy_(src.flat)
    b.owned().fill_(-3.0)
    cur, nxt = a, b
    for i in range(2):
        st = ops.new_state(gpu)
        ops.ftcs_step2(cur, nxt, D, kernel=spec, state=st, slot=0)
        torch.cuda.synchronize()
        cur, nxt = nxt, cur
        got = cur.owned()
        assert torch.equal(got, fields[i]), \
            f"{spec} {n} sweep {i + 1}: {int((got != fields[i]).sum())} points differ"
        assert ops.residual_from_state(st, K - 1) == resid[i], (spec, n, i)


@pytest.mark.parametrize("case", ["i", "ii", "iii", "iv"])
@pytest.mark.parametrize("spec", list(SPECS))
def test_edge_sweep_bitwise(h3d, gpu, spec, case):
    _sweeps(h3d.ops, gpu, _cases(SPECS[spec])[case], spec)


@pytest.mark.parametrize("spec", list(SPECS))
def test_edge_sweep_fixed_segments(h3d, gpu, spec):
    """Several pieces per tile: x segments of 8 planes (spec field L = 8), each
    with its own pipeline fill and drain around the mask-free steps."""
    parts = spec.split(":")
    parts[5] = "8"
    _sweeps(h3d.ops, gpu, _cases(SPECS[spec])["ii"], ":".join(parts))


@pytest.mark.parametrize("spec", ["tl4:1:4:1:12:0:3:2:0:1", "tl4:1:4:1:12:0:3:2:0:3"])
@pytest.mark.parametrize("eps", [1e-5, 2.9e-4])
def test_edge_solver_monotone_bitwise(h3d, gpu, spec, eps):
    """The shape forced through --kernel2: sweeps after iteration 0 run it (it
    exists as a last-residual form only), the others the depth's default
    shape; stopping iteration, last residual and field equal the run that
    takes every residual."""
    kw = dict(backend="hip", dtype="fp64", extra_args=["--kernel2", spec])
    a = h3d.HeatSolver((33, 33, 33), 10 ** 6, eps, **kw)
    b = h3d.HeatSolver((33, 33, 33), 10 ** 6, eps, **dict(kw, extra_args=kw["extra_args"] + ["--no-monotone-check"]))
    a.initialize()
    b.initialize()
    assert a.native.monotone_check and not b.native.monotone_check
    assert a.native.temporal_steps == K
    ra, rb = a.run(), b.run()
    assert ra["converged"] and ra["conv_iter"] == rb["conv_iter"], (ra, rb)
    assert ra["last_residual"] == rb["last_residual"] and ra["norm"] == rb["norm"]
    assert np.array_equal(a.gather(), b.gather())
