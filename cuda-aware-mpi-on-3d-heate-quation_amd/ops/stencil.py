"""Kernel-level ops on torch tensors.

The padded field layout of the native engine (csrc/kernels/layout.hpp: owned
block + one-cell ghost shell, z fastest, rows padded so the first owned z
point is 128-byte aligned) is allocated as a flat torch tensor; ``PaddedField``
exposes strided views of it.  ``ftcs_step`` launches the hand-written gfx950
kernel on torch's current HIP stream (or the OpenMP kernel for CPU tensors);
``ftcs_reference`` is the plain-PyTorch oracle of the same arithmetic
(heat3D.cu:128-131 with nvcc's FMA contraction, emulated exactly).
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from .._native import native

_DT = {torch.float64: "fp64", torch.float32: "fp32"}


class PaddedField:
    """One subdomain field in the native padded layout."""

    def __init__(self, n: Sequence[int], dtype=torch.float64, device="cpu", gx: int = 1, gy: int = 1, gz: int = 1):
        if dtype not in _DT:
            raise TypeError(f"unsupported dtype {dtype}")
        self.n = tuple(int(v) for v in n)
        self.dtype = dtype
        self.gx = int(gx)  # ghost planes per x side (deep halos of the K-step slab schedule)
        self.gy, self.gz = int(gy), int(gz)  # ghost rows / columns (deep y / z halos of block splits)
        self.layout = native().layout(list(self.n), torch.tensor([], dtype=dtype).element_size(), self.gx,
                                      self.gy, self.gz)
        self.flat = torch.zeros(self.layout["elems"], dtype=dtype, device=device)

    @property
    def device(self):
        return self.flat.device

    @property
    def dt(self) -> str:
        return _DT[self.dtype]

    def ghosted(self) -> torch.Tensor:
        """View (n0+2, n1+2, n2+2) including the ghost shell."""
        L = self.layout
        off = L["origin"] - L["sx"] - L["sy"] - 1
        shape = tuple(v + 2 for v in self.n)
        return self.flat.as_strided(shape, (L["sx"], L["sy"], 1), off)

    def deep3(self) -> torch.Tensor:
        """View (n0+2gx, n1+2gy, n2+2gz): every ghost layer on every axis."""
        L = self.layout
        off = L["origin"] - self.gx * L["sx"] - self.gy * L["sy"] - self.gz
        shape = (self.n[0] + 2 * self.gx, self.n[1] + 2 * self.gy, self.n[2] + 2 * self.gz)
        return self.flat.as_strided(shape, (L["sx"], L["sy"], 1), off)

    def deep(self) -> torch.Tensor:
        """View (n0+2*gx, n1+2, n2+2): every ghost plane plus the y/z ghost shell."""
        L = self.layout
        off = L["origin"] - self.gx * L["sx"] - L["sy"] - 1
        shape = (self.n[0] + 2 * self.gx, self.n[1] + 2, self.n[2] + 2)
        return self.flat.as_strided(shape, (L["sx"], L["sy"], 1), off)

    def owned(self) -> torch.Tensor:
        L = self.layout
        return self.flat.as_strided(self.n, (L["sx"], L["sy"], 1), L["origin"])

    def data_ptr(self) -> int:
        return self.flat.data_ptr()


def _stream_ptr(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _source_ptr(src: PaddedField, source: Optional[PaddedField]) -> int:
    """Pointer of the heat-source field S = dtype(dt * q) (0: none); it must
    share the field's layout (ghost shells included), dtype and device."""
    if source is None:
        return 0
    if source.layout != src.layout or source.dtype != src.dtype or source.device != src.device:
        raise ValueError("the source field must share the field's layout, dtype and device")
    return source.data_ptr()


def _cond_ptr(src: PaddedField, conductivity: Optional[PaddedField]) -> int:
    """Pointer of the conductivity field Ch = dtype(0.5 * c) (0: uniform
    material); same layout, dtype and device as the field."""
    if conductivity is None:
        return 0
    if conductivity.layout != src.layout or conductivity.dtype != src.dtype or conductivity.device != src.device:
        raise ValueError("the conductivity field must share the field's layout, dtype and device")
    return conductivity.data_ptr()


def _cap_ptr(src: PaddedField, cap: Optional[PaddedField]) -> int:
    """Pointer of the heat-capacity field s = dtype(1 / rc) (0: one capacity
    everywhere); same layout, dtype and device as the field."""
    if cap is None:
        return 0
    if cap.layout != src.layout or cap.dtype != src.dtype or cap.device != src.device:
        raise ValueError("the capacity field must share the field's layout, dtype and device")
    return cap.data_ptr()


FACES = ("x-", "x+", "y-", "y+", "z-", "z+")


def insulated_mask(insulated) -> int:
    """Face mask (bit 2 * axis + side) of ``insulated``: None, an int mask,
    ``"all"``, a comma list or a sequence of the names x-, x+, y-, y+, z-, z+.
    An unknown name is the native UsageError."""
    if insulated is None:
        return 0
    if isinstance(insulated, int):
        if not 0 <= insulated < 64:
            raise ValueError(f"insulated mask {insulated} outside [0, 64)")
        return insulated
    text = insulated if isinstance(insulated, str) else ",".join(str(f) for f in insulated)
    return native().parse_insulated(text) if text else 0


def convective_faces(convective) -> list:
    """Coefficient per face (x-, x+, y-, y+, z-, z+; -1.0 where the face is not
    convective) of ``convective``: None, a mapping ``{"y-": 0.5, "x+": 0.25}``
    (``"all"`` is a key too), a string ``"y-=0.5,x+=0.25"`` or a sequence of six
    numbers.  Unknown faces and coefficients outside [0, 1] are the native
    UsageError."""
    if convective is None:
        return [-1.0] * 6
    if isinstance(convective, str):
        return list(native().parse_convective(convective)) if convective else [-1.0] * 6
    if hasattr(convective, "items"):
        text = ",".join(f"{k}={float(v)!r}" for k, v in convective.items())
        return list(native().parse_convective(text)) if text else [-1.0] * 6
    out = [float(v) for v in convective]
    if len(out) != 6:
        raise ValueError("convective: six coefficients, one per face")
    return out


def convective_mask(convective) -> int:
    """Face mask (bit 2 * axis + side) of the convective faces."""
    return sum(1 << f for f, b in enumerate(convective_faces(convective)) if b >= 0)


def wall_coords(mask: int, n: Sequence[int], gstart: Sequence[int] = (1, 1, 1),
                N: Optional[Sequence[int]] = None) -> list:
    """``walls`` argument of the kernels: per face the local coordinate of the
    updated plane next to the insulated wall (global index 1 or N - 2), NO_WALL
    for a Dirichlet face.  Default: the block is the whole interior of its grid."""
    none = native().NO_WALL
    out = []
    for a in range(3):
        Na = N[a] if N is not None else n[a] + 2
        out.append(1 - gstart[a] if (mask >> (2 * a)) & 1 else none)
        out.append(Na - 2 - gstart[a] if (mask >> (2 * a + 1)) & 1 else none)
    return out


def ftcs_step(src: PaddedField, dst: PaddedField, D: Sequence[float],
              box: Optional[Sequence[int]] = None, kernel: str = "auto",
              state: Optional[torch.Tensor] = None, slot: int = 0,
              source: Optional[PaddedField] = None,
              conductivity: Optional[PaddedField] = None,
              walls: Optional[Sequence[int]] = None, conv=None, ambient: float = 0.0,
              cap: Optional[PaddedField] = None) -> None:
    """dst[box] = FTCS(src) on the owned box (default: all owned points).

    The fields may have deep ghosts (``PaddedField(gx=, gy=, gz=)``): the kernels
    index them with their own ghost depths (one ghost layer, the default, is
    the layout this entry always used).

    ``cap``: optional field s = dtype(1 / rc), rc >= 1 the relative volumetric
    heat capacity, in the same layout (only the centre value of an updated
    point is read): the update becomes kernels.hpp cap_update on the increment
    of the step, T' = fma(s, u, T) (its own gfx950 kernels, stencil_cap.hip),
    with or without ``source`` and ``conductivity``.

    ``walls``: insulated walls as ``wall_coords`` gives them (CPU tensors only,
    with or without a source or a conductivity: the single-step gfx950
    kernels run on wall planes copied from their inward neighbours instead).  ``conv``: the faces
    among them that are convective (``convective_faces`` forms), with the
    ambient temperature ``ambient``.

    ``source``: optional field S = dtype(dt * q) in the same layout, added to
    every updated point (kernels.hpp ftcs_update_src).

    ``conductivity``: optional field Ch = dtype(0.5 * c), c the relative
    conductivity in (0, 1], in the same layout with its ghost shell filled
    (a face weight towards a ghost point reads Ch there): the update becomes
    kernels.hpp ftcs_update_var (its own gfx950 kernels, stencil_var.hip).

    ``state``: optional uint8/int64 tensor of ``DEVICE_STATE_BYTES`` that
    receives the fused max-residual (IEEE bits of a double in its first
    8 bytes for slot 0) and whose ``done`` word turns the kernel into a no-op.
    """
    if src.layout != dst.layout or src.dtype != dst.dtype or src.device != dst.device:
        raise ValueError("src and dst must share layout, dtype and device")
    n = src.n
    b = list(box) if box is not None else [0, n[0], 0, n[1], 0, n[2]]
    for a in range(3):
        if not (0 <= b[2 * a] <= b[2 * a + 1] <= n[a]):
            raise ValueError(f"box {b} outside owned extents {n}")
    sptr = 0
    if state is not None:
        if state.device != src.device or state.numel() * state.element_size() < native().DEVICE_STATE_BYTES:
            raise ValueError("state tensor too small or on the wrong device")
        sptr = state.data_ptr()
    ext = native()
    qptr = _source_ptr(src, source)
    cptr = _cond_ptr(src, conductivity)
    kptr = _cap_ptr(src, cap)
    g = [src.gx, src.gy, src.gz]
    if src.device.type == "cuda":
        if walls is not None:
            raise ValueError("the single-step gfx950 kernels take no walls (copy the wall planes first)")
        ext.hip.stencil(src.dt, src.data_ptr(), dst.data_ptr(), list(n), b, list(D), sptr, slot,
                        kernel, _stream_ptr(src.flat), qptr, cptr, kptr, g)
    else:
        w = list(walls) if walls is not None else [ext.NO_WALL] * 6
        ext.cpu.stencil(src.dt, src.data_ptr(), dst.data_ptr(), list(n), b, list(D), sptr, slot, qptr, cptr, w,
                        convective_faces(conv), float(ambient), kptr, g)


def ftcs_step2(src: PaddedField, dst: PaddedField, D: Sequence[float], kernel: str = "auto",
               state: Optional[torch.Tensor] = None, slot: int = 0) -> None:
    """dst = K FTCS steps of src in ONE temporally blocked sweep (gfx950).

    ``kernel`` picks the depth and variant: ``tl2`` .. ``tl6[:V:R:WZ:WY:L:Q]``
    (the lean K-step kernel, stencil_tbl.hip / stencil_tbp.hip); ``auto`` is
    ``tl2``.  The ghost shell of ``src`` is treated as constant (Dirichlet)
    for every step; the residual of step s lands in ``state`` slot
    ``slot + s``.  Bitwise identical to K ``ftcs_step`` calls.
    """
    if src.layout != dst.layout or src.dtype != dst.dtype or src.device != dst.device:
        raise ValueError("src and dst must share layout, dtype and device")
    if src.device.type != "cuda":
        raise ValueError("ftcs_step2 runs on the GPU")
    sptr = 0
    if state is not None:
        if state.device != src.device or state.numel() * state.element_size() < native().DEVICE_STATE_BYTES:
            raise ValueError("state tensor too small or on the wrong device")
        sptr = state.data_ptr()
    native().hip.stencil2(src.dt, src.data_ptr(), dst.data_ptr(), list(src.n), list(D), sptr, slot,
                          kernel, _stream_ptr(src.flat))


def sweep(src: PaddedField, dst: PaddedField, D: Sequence[float], box: Sequence[int],
          ux: Sequence[int] = (0, -1), kernel: str = "tl3", state: Optional[torch.Tensor] = None,
          slot: int = 0, source: Optional[PaddedField] = None,
          conductivity: Optional[PaddedField] = None, cap: Optional[PaddedField] = None) -> None:
    """One K-step sweep (K from ``kernel``: tl2..tl6) on ``box``
    = (x0, x1, y0, y1, z0, z1) of a deep-ghost field, with the intermediate
    steps computed on the x range ``ux`` (the solver's x-slab schedule).
    GPU tensors run the gfx950 kernel, CPU tensors the K-single-steps
    definition (csrc/kernels/kernels_cpu.cpp).  ``source``: optional heat-source
    field S in the same layout, added at every step.  ``conductivity``: the
    field Ch = dtype(0.5 * c) in the same layout; on the GPU it needs a ``tv2``
    / ``tv3`` kernel (stencil_tbv.hip; the tl kernels have no conductivity form
    and a tv kernel needs one: RuntimeError either way), CPU tensors run the
    K-single-steps definition with it.  ``cap``: the heat-capacity field
    s = dtype(1 / rc) in the same layout: CPU tensors run K single steps with it
    (the definition); on the GPU it needs ``conductivity`` as well and a ``tc2`` /
    ``tc3`` kernel (stencil_tbc.hip), with real 1 / rc values on every ghost layer
    the update ranges reach; any other sweep kernel refuses it (RuntimeError)."""
    if src.layout != dst.layout or src.dtype != dst.dtype or src.device != dst.device:
        raise ValueError("src and dst must share layout, dtype and device")
    sptr = 0
    if state is not None:
        if state.device != src.device or state.numel() * state.element_size() < native().DEVICE_STATE_BYTES:
            raise ValueError("state tensor too small or on the wrong device")
        sptr = state.data_ptr()
    args = (src.dt, src.data_ptr(), dst.data_ptr(), list(src.n), src.gx, list(box), list(ux), list(D), sptr, slot,
            kernel)
    qptr = _source_ptr(src, source)
    cptr = _cond_ptr(src, conductivity)
    if src.device.type == "cuda":
        native().hip.stencil_sweep(*args, _stream_ptr(src.flat), qptr, cptr, _cap_ptr(src, cap))
    else:
        native().cpu.stencil_sweep(*args, qptr, cptr, _cap_ptr(src, cap))


def sweep3(src: PaddedField, dst: PaddedField, D: Sequence[float], box: Sequence[int], u: Sequence[int],
           kernel: str = "tl3", state: Optional[torch.Tensor] = None, slot: int = 0,
           source: Optional[PaddedField] = None, conductivity: Optional[PaddedField] = None,
           walls: Optional[Sequence[int]] = None, conv=None, ambient: float = 0.0,
           cap: Optional[PaddedField] = None) -> None:
    """K-step sweep with deep ghosts on every axis (the block-decomposition
    schedule): ``u`` = (ux0, ux1, uy0, uy1, uz0, uz1) are the update ranges of
    the intermediate steps.  GPU tensors run the lean kernel, CPU tensors the
    K-single-steps definition.  ``source``: optional heat-source field S in the
    same layout (deep ghosts included), added at every step.  ``conductivity``:
    as in ``sweep`` (GPU: ``tv2`` / ``tv3``).  ``walls``: insulated walls as
    ``wall_coords`` gives them; GPU tensors run the wall form of the lean
    kernel (stencil_tbl_wall.hip; a spec without one is a RuntimeError).
    ``conv``: the faces among ``walls`` that are convective (``convective_faces``
    forms: the coefficient per face) with the ambient temperature ``ambient``;
    GPU tensors then run the convective form (stencil_tbl_conv.hip).  ``walls``
    together with ``source``: the wall or convective form with a source
    (stencil_tbl_wall_src.hip / stencil_tbl_conv_src.hip) on GPU tensors, K
    single steps with both on CPU tensors.  ``walls`` together with
    ``conductivity`` (and a ``tv2`` / ``tv3`` kernel): the wall forms of the tv
    sweep (stencil_tbv_wall.hip / stencil_tbv_conv.hip, with or without a source)
    on GPU tensors, K single steps with them on CPU tensors.  ``cap``: as in
    ``sweep`` (CPU tensors only; the gfx950 sweep kernels refuse it)."""
    if src.layout != dst.layout or src.dtype != dst.dtype or src.device != dst.device:
        raise ValueError("src and dst must share layout, dtype and device")
    sptr = 0
    if state is not None:
        if state.device != src.device or state.numel() * state.element_size() < native().DEVICE_STATE_BYTES:
            raise ValueError("state tensor too small or on the wrong device")
        sptr = state.data_ptr()
    args = (src.dt, src.data_ptr(), dst.data_ptr(), list(src.n), [src.gx, src.gy, src.gz], list(box), list(u),
            list(D), sptr, slot, kernel)
    qptr = _source_ptr(src, source)
    cptr = _cond_ptr(src, conductivity)
    w = list(walls) if walls is not None else [native().NO_WALL] * 6
    if src.device.type == "cuda":
        native().hip.stencil_sweep3(*args, _stream_ptr(src.flat), qptr, cptr, w, convective_faces(conv), float(ambient),
                                    _cap_ptr(src, cap))
    else:
        native().cpu.stencil_sweep3(*args, qptr, cptr, w, convective_faces(conv), float(ambient), _cap_ptr(src, cap))


def _face_scale(physics, axis: int) -> float:
    """alpha h_b h_c / h_a, the factor between a face's sum of w (n - c) and its
    heat flow, evaluated left to right with b, c the two axes after ``axis`` in
    cyclic order (the one expression every backend and the reference use)."""
    h, alpha = _physics(physics)[:2]
    b, c = (axis + 1) % 3, (axis + 2) % 3
    return alpha * h[b] * h[c] / h[axis]


def _physics(physics):
    """(h, alpha, dt) of a ``HeatEquation3D``-like object or of a dict with the
    keys "h" and "dt" (``native().physics(...)``, ``Solver.physics``; alpha 1)."""
    if hasattr(physics, "h") and hasattr(physics, "dt"):
        return tuple(physics.h), float(getattr(physics, "alpha", 1.0)), float(physics.dt)
    return tuple(physics["h"]), float(physics.get("alpha", 1.0)), float(physics["dt"])


def _unkey(k: int) -> float:
    """The float64 of an ordered key of the native heat balance (heat_balance.hpp bal_key)."""
    import struct

    if k < 0:
        k ^= 0x7FFFFFFFFFFFFFFF
    return struct.unpack("<d", struct.pack("<q", k))[0]


def heat_balance(field: PaddedField, physics, box: Optional[Sequence[int]] = None,
                 source: Optional[PaddedField] = None, cond: Optional[PaddedField] = None,
                 walls: Optional[Sequence[int]] = None, conv=None, ambient: float = 0.0,
                 cap: Optional[PaddedField] = None) -> dict:
    """Heat balance of ``box`` (default: all owned points) of a field whose block
    is the interior of its grid: every face of the box lies next to a wall.

    ``physics``: the grid's ``HeatEquation3D`` (or a dict with "h" and "dt").
    ``walls``: the insulated and convective faces as ``wall_coords`` gives them
    (the other faces are Dirichlet: the neighbour across them is the stored
    vertex outside the box); ``conv``: the convective ones among them
    (``convective_faces`` forms) with the ambient temperature ``ambient``.
    ``source``: S = dtype(dt q), ``cond``: Ch = dtype(0.5 c), in the field's layout.
    ``cap``: s = dtype(1 / rc) in the field's layout: the stored heat becomes
    hx hy hz sum T / s (each term a float64 quotient); nothing else changes.

    GPU tensors run the gfx950 kernel (heat_balance.hip) on torch's current
    stream, CPU tensors the definition (cpu::heat_balance).  Returns the dict of
    ``HeatSolver.heat_balance``.  The wall vertices of insulated and convective
    faces, and everything else outside the box and its Dirichlet wall vertices,
    are never read from the field."""
    ext = native()
    n = field.n
    b = list(box) if box is not None else [0, n[0], 0, n[1], 0, n[2]]
    w = list(walls) if walls is not None else [ext.NO_WALL] * 6
    beta = convective_faces(conv)
    wall, kind = [], []
    for f in range(6):
        a, e = divmod(f, 2)
        if w[f] != ext.NO_WALL:
            wall.append(int(w[f]))
            kind.append(2 if beta[f] >= 0 else 1)
        else:
            if beta[f] >= 0:
                raise ValueError("a convective face needs its wall coordinate")
            wall.append(b[2 * a + 1] - 1 if e else b[2 * a])
            kind.append(0)
    beta = [max(v, 0.0) for v in beta]
    qptr = _source_ptr(field, source)
    cptr = _cond_ptr(field, cond)
    kptr = _cap_ptr(field, cap)
    out = torch.zeros(ext.BALANCE_SUMS_BYTES // 8, dtype=torch.int64, device=field.device)
    args = (field.dt, field.data_ptr(), list(n), [field.gx, field.gy, field.gz], b, qptr, cptr, wall, kind, beta,
            float(ambient))
    if field.device.type == "cuda":
        scratch = torch.empty(ext.BALANCE_SCRATCH_BYTES // 8, dtype=torch.int64, device=field.device)
        ext.hip.heat_balance(*args, scratch.data_ptr(), out.data_ptr(), False, _stream_ptr(field.flat), kptr)
        raw = out.cpu()
    else:
        ext.cpu.heat_balance(*args, out.data_ptr(), False, kptr)
        raw = out
    hi, lo = raw[:8].view(torch.float64), raw[8:16].view(torch.float64)
    sums = [float(hi[q]) + float(lo[q]) for q in range(8)]  # the final rounding
    h, alpha, dt = _physics(physics)
    vol = h[0] * h[1] * h[2]
    flow = {}
    total = 0.0
    for f, name in enumerate(FACES):
        flow[name] = 0.0 if kind[f] == 1 else _face_scale(physics, f // 2) * sums[2 + f]
        total += flow[name]
    source_power = vol / dt * sums[1] if source is not None else 0.0
    out = {"heat": vol * sums[0], "t_min": _unkey(int(raw[16])), "t_max": _unkey(int(raw[17])),
           "nonfinite": int(raw[18]), "source_power": source_power, "flow": flow,
           "imbalance": total + source_power}
    if cap is not None:  # (as HeatSolver.heat_balance: the key appears with a capacity only)
        out["capacity"] = True
    return out


def _steady_check(*fields: PaddedField) -> PaddedField:
    f0 = fields[0]
    for f in fields:
        if f.dtype != torch.float64:
            raise TypeError("the steady solve's operations take fp64 fields only")
        if f.layout != f0.layout or f.device != f0.device:
            raise ValueError("the fields must share one layout and device")
    return f0


def _steady_dot(f0: PaddedField, launch) -> Tuple[float, float]:
    """Runs ``launch(dot_ptr, *gpu_args)`` and returns the (hi, lo) pair it wrote."""
    ext = native()
    dot = torch.zeros(2, dtype=torch.float64, device=f0.device)
    if f0.device.type == "cuda":
        scratch = torch.empty(ext.STEADY_SCRATCH_BYTES // 8, dtype=torch.int64, device=f0.device)
        launch(dot.data_ptr(), scratch.data_ptr(), _stream_ptr(f0.flat))
        dot = dot.cpu()
    else:
        launch(dot.data_ptr(), None, None)
    return float(dot[0]), float(dot[1])


def steady_apply(src: PaddedField, dst: PaddedField, D: Sequence[float], box: Optional[Sequence[int]] = None,
                 wall: Optional[Sequence[int]] = None, kind: Optional[Sequence[int]] = None,
                 beta: Optional[Sequence[float]] = None, ambient: float = 0.0,
                 source: Optional[PaddedField] = None, cond: Optional[PaddedField] = None,
                 residual: bool = False, shift: Optional[float] = None,
                 cap: Optional[PaddedField] = None) -> Tuple[float, float]:
    """The steady solve's operator on ``box`` (default: all owned points), fp64:
    ``dst = A src`` with the dot product ``src . dst``, or (``residual``)
    ``dst = b - A src`` with ``dst . dst``, returned as the double-double pair
    (hi, lo); the value is ``hi + lo``.

    ``wall``: per face the local coordinate of the updated plane next to that
    wall of the global grid, ``NO_WALL`` where it is out of reach (a subdomain's
    inner sides); default: the owned block is the whole interior of its grid.
    ``kind``: 0 Dirichlet (default), 1 insulated, 2 convective with ``beta``.
    Across a wall the neighbour is: Dirichlet 0 (residual: the stored vertex),
    insulated the centre, convective ``fma(beta, 0 - c, c)`` (residual: towards
    ``ambient``).  ``cond``: Ch = 0.5 c; ``source``: S = dt q (residual only).
    ``shift`` = mu: the shifted operator of an implicit step instead,
    ``dst = (R + mu A) src`` with ``src . dst``, R = diag(1 / s) with ``cap`` = s
    (read at the centre of an updated point only), R = I without ``cap``; not
    with ``residual``, and ``cap`` only with ``shift``.
    GPU tensors run steady_cg.hip on torch's current stream, CPU tensors the
    definition; the field written is bitwise the same."""
    ext = native()
    f0 = _steady_check(src, dst) if cap is None else _steady_check(src, dst, cap)
    if shift is not None and residual:
        raise ValueError("steady_apply: the residual form is not shifted")
    if cap is not None and shift is None:
        raise ValueError("steady_apply: cap goes with shift only")
    n = f0.n
    b = list(box) if box is not None else [0, n[0], 0, n[1], 0, n[2]]
    w = list(wall) if wall is not None else [0, n[0] - 1, 0, n[1] - 1, 0, n[2] - 1]
    kd = [int(v) for v in kind] if kind is not None else [0] * 6
    bt = [float(v) for v in beta] if beta is not None else [0.0] * 6
    args = (src.data_ptr(), dst.data_ptr(), list(n), [f0.gx, f0.gy, f0.gz], b, [float(v) for v in D],
            _source_ptr(src, source), _cond_ptr(src, cond), w, kd, bt, float(ambient), bool(residual),
            shift is not None, 0.0 if shift is None else float(shift), 0 if cap is None else cap.data_ptr())

    def launch(dot, scratch, stream):
        if scratch is None:
            ext.cpu.steady_apply(*args, dot)
        else:
            ext.hip.steady_apply(*args, scratch, dot, stream)

    return _steady_dot(f0, launch)


def steady_update(x: Optional[PaddedField], p: Optional[PaddedField], r: Optional[PaddedField],
                  q: Optional[PaddedField], alpha: float, box: Optional[Sequence[int]] = None) -> Tuple[float, float]:
    """``x += alpha p``, ``r -= alpha q`` on ``box`` (one fused multiply-add
    each) and the new ``r . r`` as the double-double pair (hi, lo).  ``x`` and
    ``p`` both None: only ``r`` is updated (``alpha`` = 1: ``r -= q``, the true
    residual of an implicit step); ``r`` and ``q`` both None: only ``x``
    (``T' = fma(m, d, T)``), and the pair is (0, 0)."""
    ext = native()
    if (x is None) != (p is None) or (r is None) != (q is None) or (x is None and r is None):
        raise ValueError("steady_update: four fields, or x and p alone, or r and q alone")
    f0 = _steady_check(*[f for f in (x, p, r, q) if f is not None])
    n = f0.n
    b = list(box) if box is not None else [0, n[0], 0, n[1], 0, n[2]]
    args = tuple(0 if f is None else f.data_ptr() for f in (x, p, r, q)) + (
        list(n), [f0.gx, f0.gy, f0.gz], b, float(alpha))

    def launch(dot, scratch, stream):
        if scratch is None:
            ext.cpu.steady_update(*args, dot)
        else:
            ext.hip.steady_update(*args, scratch, dot, stream)

    return _steady_dot(f0, launch)


def steady_direction(p: PaddedField, r: PaddedField, beta: float, box: Optional[Sequence[int]] = None) -> None:
    """``p = r + beta p`` on ``box``, one fused multiply-add per point."""
    ext = native()
    f0 = _steady_check(p, r)
    n = f0.n
    b = list(box) if box is not None else [0, n[0], 0, n[1], 0, n[2]]
    args = (p.data_ptr(), r.data_ptr(), list(n), [f0.gx, f0.gy, f0.gz], b, float(beta))
    if f0.device.type == "cuda":
        ext.hip.steady_direction(*args, _stream_ptr(f0.flat))
    else:
        ext.cpu.steady_direction(*args)


def init_field(f: PaddedField, gstart: Sequence[int], N: Sequence[int], h: Sequence[float]) -> None:
    """Analytic IC/BC into the padded field (reference heat3D.cu:408-453)."""
    ext = native()
    if f.device.type == "cuda":
        ext.hip.init_field(f.dt, f.data_ptr(), list(f.n), list(gstart), list(N), list(h), _stream_ptr(f.flat))
    else:
        ext.cpu.init_field(f.dt, f.data_ptr(), list(f.n), list(gstart), list(N), list(h))


def pack_box(f: PaddedField, box: Sequence[int], out: torch.Tensor) -> None:
    """Copy a local box (ghost indices allowed, -1..n) into a contiguous buffer (GPU)."""
    native().hip.pack_box(f.dt, f.data_ptr(), list(f.n), list(box), out.data_ptr(), _stream_ptr(f.flat))


def unpack_box(f: PaddedField, box: Sequence[int], buf: torch.Tensor) -> None:
    native().hip.unpack_box(f.dt, f.data_ptr(), list(f.n), list(box), buf.data_ptr(), _stream_ptr(f.flat))


def ftcs_reference(T: torch.Tensor, D: Sequence[float], src: Optional[torch.Tensor] = None,
                   cond: Optional[torch.Tensor] = None, insulated=None, convective=None,
                   ambient: float = 0.0) -> Tuple[torch.Tensor, float]:
    """Plain-PyTorch FTCS on a ghosted block; returns (new interior, max |dT|).

    ``insulated``: faces of the block that are zero-flux walls (``insulated_mask``
    forms; the block is the whole grid).  The ghost plane of such a face is
    replaced by a copy of the first interior plane before the update, so the
    neighbour across the wall is the centre value.

    ``convective``: faces that are convective walls (``convective_faces`` forms)
    with the ambient temperature ``ambient``: the ghost plane becomes
    fma(beta, T_inf - c, c) of the first interior plane c (kernels.hpp
    convective_ghost), beta and T_inf rounded to the dtype of ``T``.

    ``cond``: optional ghosted block (shape of ``T``) of Ch = dtype(0.5 * c),
    c the relative conductivity: the update of kernels.hpp ftcs_update_var.

    ``src``: optional heat source S = dtype(dt * q) on the interior points
    (shape of the result), added with one rounded addition after the update
    (kernels.hpp ftcs_update_src).

    Same arithmetic as the native backends (exactly rounded FMAs emulated with
    error-free transformations, utils/fma.py), so results compare bitwise."""
    from ..utils.fma import fma, ftcs_update, ftcs_update_var

    def seven(F):
        return (F[1:-1, 1:-1, 1:-1], F[:-2, 1:-1, 1:-1], F[2:, 1:-1, 1:-1], F[1:-1, :-2, 1:-1], F[1:-1, 2:, 1:-1],
                F[1:-1, 1:-1, :-2], F[1:-1, 1:-1, 2:])

    mask = insulated_mask(insulated)
    beta = convective_faces(convective)
    if any(b >= 0 for b in beta):
        T = T.clone()
        tinf = torch.tensor(float(ambient), dtype=T.dtype)
        for f, b in enumerate(beta):
            if b < 0:
                continue
            if (mask >> f) & 1:
                raise ValueError("a face is either insulated or convective")
            a, e = divmod(f, 2)
            c1 = T.select(a, T.shape[a] - 2 if e else 1).clone()
            T.select(a, T.shape[a] - 1 if e else 0).copy_(fma(b, tinf - c1, c1))
    if mask:
        T = T.clone()
        for a in range(3):
            if (mask >> (2 * a)) & 1:
                T.select(a, 0).copy_(T.select(a, 1).clone())
            if (mask >> (2 * a + 1)) & 1:
                T.select(a, T.shape[a] - 1).copy_(T.select(a, T.shape[a] - 2).clone())
    c = T[1:-1, 1:-1, 1:-1]
    if cond is not None:
        if cond.shape != T.shape or cond.dtype != T.dtype:
            raise ValueError("cond must be a ghosted block of the shape and dtype of T")
        new = ftcs_update_var(*seven(T), *seven(cond), D)
    else:
        new = ftcs_update(*seven(T), D)
    if src is not None:
        new = new + src.to(new.dtype)
    # residual in the field's precision (kernels.hpp resid_abs), widened for the max
    res = (new - c).abs().max().double().item() if new.numel() else 0.0
    return new, res


def residual_from_state(state: torch.Tensor, slot: int = 0) -> float:
    """Decode the fused residual (double bits) written by ftcs_step."""
    raw = state.detach().cpu().contiguous().view(torch.uint8)[8 * slot: 8 * slot + 8]
    return float(raw.view(torch.float64).item())


def new_state(device, eps: float = 0.0) -> torch.Tensor:
    """Zeroed DeviceState buffer with the residual slots at their initial value."""
    ext = native()
    st = torch.zeros(ext.DEVICE_STATE_BYTES // 8, dtype=torch.int64)
    init = ext.RESIDUAL_INIT_BITS
    st[: ext.RESIDUAL_SLOTS] = init if init < 2 ** 63 else init - 2 ** 64
    return st.to(device)
