"""Performance metrics for the 7-point stencil."""
from __future__ import annotations

# measured HBM copy bandwidth of one MI355X (MI355X_MICROARCH.md: 6.29 TB/s float4 copy)
HBM_BW_BYTES_PER_S = 6.29e12


def glups(points: int, iterations: int, seconds: float) -> float:
    """Giga lattice-point updates per second."""
    return points * iterations / seconds / 1e9 if seconds > 0 else 0.0


def bytes_per_point(esize: int) -> int:
    """Compulsory HBM traffic per updated point: read once + write once."""
    return 2 * esize


def effective_bandwidth(glups_value: float, esize: int) -> float:
    """Effective HBM bandwidth in TB/s implied by a GLUPS figure."""
    return glups_value * 1e9 * bytes_per_point(esize) / 1e12


def roofline_glups(esize: int, n_gpus: int = 1, bw: float = HBM_BW_BYTES_PER_S) -> float:
    return n_gpus * bw / bytes_per_point(esize) / 1e9


_FACES = ("x-", "x+", "y-", "y+", "z-", "z+")


def heat_balance_reference(T, model, source=None, conductivity=None, insulated=None, convective=None,
                           ambient: float = 0.0, dtype: str = "fp64") -> dict:
    """The heat balance of docs/ARCHITECTURE.md ("Heat balance") in NumPy, the
    tests' reference for ``HeatSolver.heat_balance`` and ``ops.heat_balance``.

    ``T``: the global field (wall vertices included; those of insulated and
    convective faces are not read), ``model`` a ``HeatEquation3D``, ``source`` the
    global q and ``conductivity`` the global c as ``set_source`` /
    ``set_conductivity`` take them, ``insulated`` / ``convective`` / ``ambient`` as
    ``HeatSolver`` takes them, ``dtype`` the solver's.  Every stored value is
    rounded to ``dtype`` as the solver stores it (S = dtype(dt q),
    Ch = dtype(0.5 c)) and widened; every term is a float64 and every sum is
    ``math.fsum``, the correctly rounded sum.

    Returns the keys of ``HeatSolver.heat_balance`` and, for tolerances,
    ``"terms"``: per sum ("heat", "source_power", the face names) the pair
    (number of terms, sum of |term| scaled like the quantity)."""
    import math

    import numpy as np
    import torch

    from ..ops.stencil import convective_faces, insulated_mask
    from .fma import fma

    rt = {"fp64": np.float64, "fp32": np.float32}[dtype]
    Tr = np.asarray(T, dtype=np.float64).astype(rt)
    if Tr.shape != tuple(model.n):
        raise ValueError(f"heat_balance_reference: shape {Tr.shape} != grid {tuple(model.n)}")
    h, dt, alpha = model.h, model.dt, model.alpha
    vol = h[0] * h[1] * h[2]
    inner = (slice(1, -1),) * 3
    U = Tr[inner].astype(np.float64)
    out, terms = {}, {}

    def total(name, t, scale):
        t = np.asarray(t, dtype=np.float64).ravel()
        terms[name] = (int(t.size), scale * math.fsum(np.abs(t).tolist()))
        return math.fsum(t.tolist())

    out["heat"] = vol * total("heat", U, vol)
    finite = U[~np.isnan(U)]
    out["t_min"] = float(finite.min()) if finite.size else float("nan")
    out["t_max"] = float(finite.max()) if finite.size else float("nan")
    out["nonfinite"] = int((~np.isfinite(U)).sum())
    if source is not None:
        S = (dt * np.asarray(source, dtype=np.float64)).astype(rt)
        out["source_power"] = vol / dt * total("source_power", S[inner].astype(np.float64), vol / dt)
    else:
        out["source_power"] = 0.0
        terms["source_power"] = (0, 0.0)
    Ch = None if conductivity is None else (0.5 * np.asarray(conductivity, dtype=np.float64)).astype(rt)
    mask = insulated_mask(insulated)
    beta = convective_faces(convective)
    flow = {}
    for f, name in enumerate(_FACES):
        a, e = divmod(f, 2)
        if (mask >> f) & 1:
            flow[name] = 0.0  # the neighbour is the centre value: no term
            terms[name] = (0, 0.0)
            continue
        first = [slice(1, -1)] * 3
        wall = [slice(1, -1)] * 3
        first[a] = -2 if e else 1
        wall[a] = -1 if e else 0
        c = Tr[tuple(first)]
        if beta[f] >= 0:
            ct = torch.from_numpy(np.ascontiguousarray(c))
            tinf = torch.tensor(float(ambient), dtype=ct.dtype)
            nb = fma(torch.tensor(float(beta[f]), dtype=ct.dtype), tinf - ct, ct).numpy()  # convective_ghost
        else:
            nb = Tr[tuple(wall)]
        t = nb.astype(np.float64) - c.astype(np.float64)
        if Ch is not None:
            w = Ch[tuple(first)] + Ch[tuple(wall)]  # one add in the field dtype: the scheme's face weight
            t = w.astype(np.float64) * t
        b, cc = (a + 1) % 3, (a + 2) % 3
        scale = alpha * h[b] * h[cc] / h[a]
        flow[name] = scale * total(name, t, scale)
    out["flow"] = flow
    tot = 0.0
    for name in _FACES:
        tot += flow[name]
    out["imbalance"] = tot + out["source_power"]
    out["terms"] = terms
    return out
