"""The 3D heat equation model and its high-level solver driver.

``HeatEquation3D`` is the problem definition of the reference
(heat3D.cu:1-37 physics header, 331-367 constants, 408-453 IC/BC, 1093-1106
analytic steady state T = y).  ``HeatSolver`` drives the native MI355X engine
(csrc/runtime/solver.cpp) from Python: it picks the backend (gfx950 HIP or
OpenMP CPU), the communicator (RCCL over xGMI for one-process-per-GPU jobs,
sockets for multi-process CPU jobs, LocalComm for virtual ranks) and the
process grid, and exposes run / step / gather / checkpoint.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .._native import native


@dataclass(frozen=True)
class HeatEquation3D:
    """T_t = alpha * lap(T) on [0,1]^3, vertex-centred grid of n[0] x n[1] x n[2]."""

    n: Tuple[int, int, int]
    alpha: float = 1.0
    cfl: float = 0.4

    @property
    def h(self) -> Tuple[float, float, float]:
        return tuple(1.0 / (float(k) - 1.0) for k in self.n)  # type: ignore[return-value]

    @property
    def dt(self) -> float:
        return self.cfl * 1.0 / 6 * min(self.h) ** 2.0 / self.alpha

    @property
    def D(self) -> Tuple[float, float, float]:
        return tuple(self.dt * self.alpha / hh ** 2.0 for hh in self.h)  # type: ignore[return-value]

    @property
    def interior_points(self) -> int:
        return (self.n[0] - 2) * (self.n[1] - 2) * (self.n[2] - 2)

    def boundary_value(self, i: int, j: int, k: int) -> float:
        N = self.n
        if i == 0 or i == N[0] - 1 or k == 0 or k == N[2] - 1:
            return float(j) * self.h[1]
        if j == N[1] - 1:
            return 1.0
        return 0.0

    def initial_field(self, dtype=np.float64) -> np.ndarray:
        """Global initial condition: 0 inside, Dirichlet values on the boundary."""
        N = self.n
        y = np.arange(N[1], dtype=np.float64) * self.h[1]
        T = np.zeros(N, dtype=np.float64)
        T[:, N[1] - 1, :] = 1.0
        T[0, :, :] = y[:, None]
        T[-1, :, :] = y[:, None]
        T[:, :, 0] = y[None, :]
        T[:, :, -1] = y[None, :]
        return T.astype(dtype)

    def steady_state(self) -> np.ndarray:
        """Analytic steady state T = y (heat3D.cu:1096-1102)."""
        y = np.arange(self.n[1], dtype=np.float64) * self.h[1]
        return np.broadcast_to(y[None, :, None], self.n).copy()

    def sine_source(self, amplitude: float) -> np.ndarray:
        """Heat source q = alpha * lam_h * A * sin(pi x) sin(pi y) sin(pi z) on the grid,
        with lam_h = sum_d (4 / h_d^2) sin^2(pi h_d / 2) the eigenvalue of the
        discrete Laplacian for that mode: the discrete steady state of
        T_t = alpha lap(T) + q with the reference's walls is exactly
        y + A sin(pi x) sin(pi y) sin(pi z)."""
        h = self.h
        lam = sum(4.0 / hd ** 2 * np.sin(np.pi * hd / 2.0) ** 2 for hd in h)
        sx, sy, sz = (np.sin(np.pi * np.arange(n, dtype=np.float64) * hd) for n, hd in zip(self.n, h))
        return (self.alpha * lam * float(amplitude)) * sx[:, None, None] * sy[None, :, None] * sz[None, None, :]

    def layered_conductivity(self, c_low: float, c_high: float, split: float = 0.5) -> np.ndarray:
        """Two-layer body: relative conductivity c = ``c_low`` where y_j < ``split``,
        ``c_high`` elsewhere (global array, 0 < c <= 1)."""
        y = np.arange(self.n[1], dtype=np.float64) * self.h[1]
        c = np.where(y < float(split), float(c_low), float(c_high))
        return np.broadcast_to(c[None, :, None], self.n).copy()

    def layered_capacity(self, rc_low: float, rc_high: float, split: float = 0.5) -> np.ndarray:
        """Two-layer body: relative volumetric heat capacity rc = ``rc_low`` where
        y_j < ``split``, ``rc_high`` elsewhere (global array, rc >= 1), the layers
        of ``layered_conductivity``."""
        y = np.arange(self.n[1], dtype=np.float64) * self.h[1]
        rc = np.where(y < float(split), float(rc_low), float(rc_high))
        return np.broadcast_to(rc[None, :, None], self.n).copy()

    def dirichlet_mode(self, m: Sequence[int], s: float = 1.0) -> Tuple[np.ndarray, float]:
        """Discrete eigenmode of the update between Dirichlet walls at 0: the
        product of sin(pi m_a i_a / (N_a - 1)) over the three axes (global array,
        0 on every wall vertex).  One step of a body with the uniform capacity
        factor ``s`` = 1 / rc multiplies it by the returned factor
        g = 1 - s * 4 sum_a D_a sin^2(pi m_a / (2 (N_a - 1))); ``s`` = 1 is the
        body without a heat capacity."""
        v = []
        lam = 0.0
        for a in range(3):
            N = self.n[a]
            i = np.arange(N, dtype=np.float64)
            va = np.sin(np.pi * m[a] * i / (N - 1))
            va[0] = va[-1] = 0.0
            v.append(va)
            lam += self.D[a] * np.sin(np.pi * m[a] / (2.0 * (N - 1))) ** 2
        T = v[0][:, None, None] * v[1][None, :, None] * v[2][None, None, :]
        return T, float(1.0 - float(s) * 4.0 * lam)

    def implicit_factor(self, m_vec: Sequence[int], m: float, theta: float, s: float = 1.0) -> float:
        """Exact factor by which one implicit step (``HeatSolver.step_implicit``)
        of length ``m`` explicit steps with ``theta`` multiplies the mode
        ``dirichlet_mode(m_vec)`` in a body with the uniform capacity factor
        ``s`` = 1 / rc: (1 - (1 - theta) m s lam) / (1 + theta m s lam) with
        lam = 4 sum_a D_a sin^2(pi m_a / (2 (N_a - 1)))."""
        lam = 0.0
        for a in range(3):
            lam += self.D[a] * np.sin(np.pi * m_vec[a] / (2.0 * (self.n[a] - 1))) ** 2
        lam *= 4.0
        msl = float(m) * float(s) * lam
        return float((1.0 - (1.0 - float(theta)) * msl) / (1.0 + float(theta) * msl))

    def layered_steady(self, c: np.ndarray) -> np.ndarray:
        """Exact steady state of the discrete scheme for a conductivity that
        varies in y only, between the walls T(y=0) = 0 and T(y=1) = 1: a
        constant flux w_m (p_{m+1} - p_m) through every y face, w_m the face
        mean 0.5 (c_m + c_{m+1}), so p_0 = 0 and
        p_j = (sum_{m<j} 1/w_m) / (sum_{m<N-1} 1/w_m); constant in x and z."""
        c = np.asarray(c, dtype=np.float64)
        if c.shape != tuple(self.n):
            raise ValueError(f"layered_steady: shape {c.shape} != grid {tuple(self.n)}")
        cy = c[0, :, 0]
        if not np.array_equal(c, np.broadcast_to(cy[None, :, None], self.n)):
            raise ValueError("layered_steady: the conductivity must vary in y only")
        w = 0.5 * (cy[:-1] + cy[1:])
        r = np.concatenate(([0.0], np.cumsum(1.0 / w)))
        p = r / r[-1]
        return np.broadcast_to(p[None, :, None], self.n).copy()

    def neumann_mode(self, axis: int, m: int) -> Tuple[np.ndarray, float]:
        """Discrete eigenmode of the update between two insulated walls of
        ``axis``: cos(pi m (j - 1/2) / M) at the interior vertices j = 1..M,
        M = N - 2, constant along the other axes (global array; the wall
        vertices hold copies of their inward neighbours).  With every face
        insulated one step multiplies it by the returned factor
        g = 1 - 4 D_axis sin^2(pi m / (2 M))."""
        N = self.n[axis]
        M = N - 2
        j = np.arange(1, M + 1, dtype=np.float64)
        v = np.empty(N, dtype=np.float64)
        v[1:-1] = np.cos(np.pi * m * (j - 0.5) / M)
        v[0], v[-1] = v[1], v[-2]
        shape = [1, 1, 1]
        shape[axis] = N
        T = np.broadcast_to(v.reshape(shape), self.n).copy()
        g = 1.0 - 4.0 * self.D[axis] * np.sin(np.pi * m / (2.0 * M)) ** 2
        return T, float(g)

    def wall_coefficient(self, h: float, axis: int, k: float = 1.0) -> float:
        """Coefficient beta of a convective wall of ``axis`` for a surface
        coefficient ``h`` (-k dT/dn = h (T - T_inf)) and a conductivity ``k``:
        beta = 2 Bi / (2 + Bi) with Bi = h * h_axis / k, the surface acting at
        the face midway between the wall vertex and the first interior vertex.
        The update stays a convex combination only for beta <= 1 (Bi <= 2): a
        larger one raises ValueError (refine the grid along ``axis``)."""
        if not (h >= 0.0 and k > 0.0 and np.isfinite(h) and np.isfinite(k)):
            raise ValueError(f"wall_coefficient: need h >= 0 and k > 0, got h = {h}, k = {k}")
        bi = float(h) * self.h[axis] / float(k)
        beta = 2.0 * bi / (2.0 + bi)
        if beta > 1.0:
            raise ValueError(f"wall_coefficient: Bi = {bi:g} gives beta = {beta:g} > 1 (need Bi <= 2)")
        return beta

    def convective_slab_steady(self, beta: float, ambient: float = 0.0) -> np.ndarray:
        """Exact steady state of the discrete scheme for the slab problem: x-, x+,
        z-, z+ insulated, y- convective with coefficient ``beta`` > 0 and ambient
        ``ambient``, y+ Dirichlet at 1.  Constant in x and z and linear in y,
        T_j = T_inf + s (1 / beta + j - 1) for j = 1 .. Ny - 2 with
        s = (1 - T_inf) / (1 / beta + Ny - 2); the y- wall vertices hold the
        ghost T_1 + beta (T_inf - T_1) (global array)."""
        if not 0.0 < beta <= 1.0:
            raise ValueError(f"convective_slab_steady: beta {beta} outside (0, 1]")
        Ny = self.n[1]
        s = (1.0 - ambient) / (1.0 / beta + Ny - 2)
        j = np.arange(Ny, dtype=np.float64)
        v = ambient + s * (1.0 / beta + j - 1.0)
        v[0] = v[1] + beta * (ambient - v[1])
        v[-1] = 1.0
        return np.broadcast_to(v[None, :, None], self.n).copy()

    def convective_slab_flows(self, beta: float, ambient: float = 0.0) -> Dict[str, float]:
        """Exact heat flows (``HeatSolver.heat_balance()["flow"]``, positive into the
        body) of the slab steady state ``convective_slab_steady``: the constant
        flux s per face passes every y face, so -alpha hx hz / hy * s per point
        of a y plane, (Nx - 2)(Nz - 2) of them, leaves through y- and the opposite
        value enters through y+; the four insulated faces carry none."""
        if not 0.0 < beta <= 1.0:
            raise ValueError(f"convective_slab_flows: beta {beta} outside (0, 1]")
        Nx, Ny, Nz = self.n
        h = self.h
        s = (1.0 - ambient) / (1.0 / beta + Ny - 2)
        out = -self.alpha * h[0] * h[2] / h[1] * s * ((Nx - 2) * (Nz - 2))
        return {"x-": 0.0, "x+": 0.0, "y-": out, "y+": -out, "z-": 0.0, "z+": 0.0}

    def convective_slab_source_steady(self, beta: float, ambient: float, q: float) -> np.ndarray:
        """Exact steady state of the discrete scheme for the slab problem of
        ``convective_slab_steady`` with a uniform heat source ``q``.  With
        sigma = dt q / D_y and M = Ny - 2, T_j = A + B j - sigma j^2 / 2 on
        j = 1 .. M, where A and B solve
        beta A = (1 - beta) (B - sigma / 2) + beta T_inf (the y- wall) and
        A + B (M + 1) - sigma (M + 1)^2 / 2 = 1 (y+ Dirichlet at 1).  Constant in
        x and z; the y- wall vertices hold the ghost T_1 + beta (T_inf - T_1), y+
        holds 1 (global array)."""
        if not 0.0 < beta <= 1.0:
            raise ValueError(f"convective_slab_source_steady: beta {beta} outside (0, 1]")
        Ny = self.n[1]
        M = Ny - 2
        sigma = self.dt * float(q) / self.D[1]
        # A = ((1 - beta) (B - sigma / 2) + beta T_inf) / beta in the y+ condition
        r = (1.0 - beta) / beta
        B = (1.0 + sigma * (M + 1) ** 2 / 2.0 + r * sigma / 2.0 - ambient) / (r + M + 1)
        A = r * (B - sigma / 2.0) + ambient
        j = np.arange(Ny, dtype=np.float64)
        v = A + B * j - sigma * j * j / 2.0
        v[0] = v[1] + beta * (ambient - v[1])
        v[-1] = 1.0
        return np.broadcast_to(v[None, :, None], self.n).copy()

    def layered_convective_slab_steady(self, c: np.ndarray, beta: float, ambient: float = 0.0) -> np.ndarray:
        """Exact steady state of the discrete scheme for a composite wall cooled
        by a fluid: a conductivity ``c`` that varies in y only (as for
        ``layered_steady``), x-, x+, z-, z+ insulated, y- convective with
        coefficient ``beta`` > 0 and ambient ``ambient``, y+ Dirichlet at 1.  With
        the face weights w_{j+1/2} = 0.5 (c_j + c_{j+1}) a constant flux F passes
        every y face: beta w_{1/2} (T_1 - T_inf) = F at the wall (its ghost is
        T_1 + beta (T_inf - T_1), the weight still reads c at the wall vertex),
        w_{j+1/2} (T_{j+1} - T_j) = F inside, and T_{Ny-1} = 1 fixes F.  Constant
        in x and z; the y- wall vertices hold the ghost (global array, float64)."""
        if not 0.0 < beta <= 1.0:
            raise ValueError(f"layered_convective_slab_steady: beta {beta} outside (0, 1]")
        c = np.asarray(c, dtype=np.float64)
        if c.shape != tuple(self.n):
            raise ValueError(f"layered_convective_slab_steady: shape {c.shape} != grid {tuple(self.n)}")
        cy = c[0, :, 0]
        if not np.array_equal(c, np.broadcast_to(cy[None, :, None], self.n)):
            raise ValueError("layered_convective_slab_steady: the conductivity must vary in y only")
        w = 0.5 * (cy[:-1] + cy[1:])  # w[j] = w_{j+1/2}
        # resistances from T_inf up to vertex j = 1 .. Ny - 1
        r = np.concatenate(([1.0 / (float(beta) * w[0])], 1.0 / w[1:]))
        R = np.cumsum(r)
        F = (1.0 - float(ambient)) / R[-1]
        v = np.empty(self.n[1], dtype=np.float64)
        v[1:] = float(ambient) + F * R
        v[0] = v[1] + float(beta) * (float(ambient) - v[1])
        v[-1] = 1.0
        return np.broadcast_to(v[None, :, None], self.n).copy()

    def error_percent(self, T: np.ndarray) -> float:
        """100 * mean |T - y| over interior points (the reference's 'L2-norm error')."""
        y = self.steady_state()
        d = np.abs(T[1:-1, 1:-1, 1:-1] - y[1:-1, 1:-1, 1:-1])
        return 100.0 * float(d.mean())


def _fmt(x) -> str:
    return repr(float(x)) if isinstance(x, float) else str(x)


class HeatSolver:
    """Python driver of the native engine.

    Parameters mirror the CLI (``heat3d NX NY NZ ITER_MAX EPS --flags``).  In a
    torch.distributed job (``WORLD_SIZE > 1``) the native communicator is
    bootstrapped through torch.distributed: RCCL for the HIP backend,
    sockets for the CPU backend.
    """

    def __init__(self, n: Sequence[int], iter_max: int = 1000, eps: float = 1e-5, *,
                 dtype: str = "fp64", backend: str = "auto", comm: str = "auto",
                 decomp: Optional[Sequence[int]] = None, virtual_ranks: int = 1,
                 kernel: str = "auto", graph: bool = True, overlap: bool = True,
                 check_every: int = 64, graph_chunk: int = 0, device: Optional[int] = None,
                 threads: int = 0, extra_args: Sequence[str] = (), group=None,
                 phantom: Optional[Sequence[int]] = None, conductivity_sweeps: bool = False,
                 insulated=None, convective=None, ambient: float = 0.0, wall_source_sweeps: bool = False,
                 capacity_sweeps: bool = False):
        ext = native()
        self.model = HeatEquation3D(tuple(int(v) for v in n))  # type: ignore[arg-type]
        args: List[str] = [str(int(v)) for v in n] + [str(int(iter_max)), _fmt(eps)]
        args += ["--dtype", dtype, "--kernel", kernel, "--check-every", str(check_every),
                 "--graph-chunk", str(graph_chunk)]
        if backend != "auto":
            args += ["--backend", backend]
        if decomp:
            args += ["--decomp", "x".join(str(int(d)) for d in decomp)]
        if virtual_ranks > 1:
            args += ["--virtual-ranks", str(virtual_ranks)]
        if not graph:
            args.append("--no-graph")
        if not overlap:
            args.append("--no-overlap")
        if threads:
            args += ["--threads", str(threads)]
        if conductivity_sweeps:
            # with a conductivity field: K-step sweeps of the tv kernels instead of single steps
            args.append("--conductivity-sweeps")
        if capacity_sweeps:
            # with a heat capacity and a conductivity field: K-step sweeps of the tc kernels instead of single steps
            args.append("--capacity-sweeps")
        if wall_source_sweeps:
            # with insulated / convective walls and a heat source: K-step sweeps instead of single steps
            args.append("--wall-source-sweeps")
        if insulated:
            # zero-flux walls: names of x-, x+, y-, y+, z-, z+ (a sequence or a comma list) or "all";
            # the native parser validates them (UsageError)
            args += ["--insulated", insulated if isinstance(insulated, str) else ",".join(str(f) for f in insulated)]
        if convective:
            # convective (Robin) walls: {"y-": 0.5, "x+": 0.25} (or "all"), a string "y-=0.5,x+=0.25";
            # the native parser validates faces and coefficients (UsageError)
            text = convective if isinstance(convective, str) else ",".join(
                f"{f}={float(b)!r}" for f, b in dict(convective).items())
            args += ["--convective", text]
        if ambient != 0.0 or convective:
            args += ["--ambient", repr(float(ambient))]
        args += list(extra_args)
        self.args = args

        from ..parallel.distributed import env_info, native_comm_args

        info = env_info()
        use_gpu = backend == "hip" or (backend == "auto" and ext.device_count() > 0)
        if comm == "auto":
            if info.world_size > 1:
                comm = "rccl" if use_gpu else "socket"
            else:
                comm = "local"
        if phantom is not None:
            comm = "phantom"
        dev = -1 if device is None else int(device)
        if use_gpu and device is None and info.world_size > 1:
            dev = info.local_rank % max(1, ext.device_count())
        self.comm_kind = comm

        def make(extra=()):
            from ..parallel.distributed import NativeCommArgs

            if phantom is not None:
                # performance proxy: rank phantom[0] of a phantom[1]-rank job, peers emulated
                cargs = NativeCommArgs(int(phantom[0]), int(phantom[1]), "phantom")
            elif comm in ("rccl", "socket", "staged"):
                cargs = native_comm_args(comm, group=group)  # collective: every rank calls it
            else:
                cargs = NativeCommArgs()
            return ext.Solver(args + list(extra), device=dev, **cargs.kwargs())

        self._make = make
        self._s = make()
        self._initialized = False
        self.stream_graphs_retried = False

    # -- lifecycle -------------------------------------------------------------
    def initialize(self) -> "HeatSolver":
        """(Re)initialise the fields.  If the start-up canary of the
        overlapped schedule's per-stream hipGraphs deadlocks (the solver aborts
        its communicators and raises; every rank alike), the native solver is
        rebuilt once with the graphs off — a new communicator — and
        initialised again: the run continues eagerly in this process."""
        try:
            self._s.initialize()
        except RuntimeError as e:
            if "stream-graph canary deadlock" not in str(e) or self.stream_graphs_retried:
                raise
            import sys

            print(f"heat3d: {e}; rebuilding the solver with --stream-graphs off", file=sys.stderr, flush=True)
            self.stream_graphs_retried = True
            self._s = None
            self._s = self._make(["--stream-graphs", "off"])
            self._s.initialize()
        self._initialized = True
        return self

    def _ensure(self):
        if not self._initialized:
            self.initialize()

    def run(self) -> Dict:
        """Iterate until converged or ITER_MAX; returns the run report."""
        self._ensure()
        r = dict(self._s.run())
        g, loc = self._s.compute_error()
        r["error_percent"] = 100.0 * g
        r["error_percent_local"] = 100.0 * loc
        return r

    def step(self, n: int) -> None:
        """Enqueue exactly ``n`` iterations (asynchronous on the GPU)."""
        self._ensure()
        self._s.step(int(n))

    def synchronize(self) -> None:
        self._s.synchronize()

    # -- problem definition ----------------------------------------------------
    def _global_array(self, a, what: str) -> np.ndarray:
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
        if a.shape != tuple(self.model.n):
            raise ValueError(f"{what}: shape {a.shape} != grid {tuple(self.model.n)}")
        if not np.isfinite(a).all():
            raise ValueError(f"{what}: non-finite values")
        return a

    def set_source(self, q) -> None:
        """Volumetric heat source: T_t = alpha lap(T) + q, ``q`` an array of the
        global shape (every rank of a multi-process job passes the same array;
        each keeps its own box).  The update adds S = dtype(dt * q) to every
        updated point.  Keeps the field, restarts the iteration count and the
        convergence state at 0.  Collective."""
        q = self._global_array(q, "set_source")
        self._ensure()
        self._s.set_source(q)

    def clear_source(self) -> None:
        self._s.clear_source()

    def set_conductivity(self, c) -> None:
        """Spatially varying conductivity: T_t = div(alpha c grad T) + q, ``c`` the
        relative conductivity on the global vertex grid, 0 < c <= 1 (alpha is the
        diffusivity of the best-conducting material, so the time step stays
        stable).  A value outside (0, 1] or not finite is the native
        ``UsageError`` (a RuntimeError), raised on every rank.  While set, every
        iteration runs as a single step, or, with ``conductivity_sweeps=True``,
        in K-step sweeps of the tv kernels (same bits; behind insulated or
        convective walls their wall forms).  Keeps the field, restarts the iteration count and
        the convergence state at 0.  Collective."""
        c = np.ascontiguousarray(np.asarray(c, dtype=np.float64))
        if c.shape != tuple(self.model.n):
            raise ValueError(f"set_conductivity: shape {c.shape} != grid {tuple(self.model.n)}")
        self._ensure()
        self._s.set_conductivity(c)

    def clear_conductivity(self) -> None:
        """Back to the uniform material (and the K-step sweeps)."""
        self._s.clear_conductivity()

    def set_capacity(self, rc) -> None:
        """Spatially varying heat capacity: rc T_t = div(alpha c grad T) + q, ``rc``
        the relative volumetric heat capacity rho c_p on the global vertex grid,
        rc >= 1 (the reference material is the one with the smallest capacity, so
        the time step stays stable).  A value below 1 or not finite is the native
        ``UsageError`` (a RuntimeError) naming the first offending index, raised
        on every rank.  While set, every iteration runs as a single step
        (``conductivity_sweeps`` and ``wall_source_sweeps`` mean nothing) unless a
        conductivity is set too and ``capacity_sweeps=True`` asks for the K-step
        sweeps of the tc kernels (same bits; without a conductivity that flag
        does nothing), the stored heat of ``heat_balance()`` is weighted with rc, the steady
        state (``solve_steady``) is the one without a capacity, and ``step_implicit`` honours it.  A body with
        rc == 1 everywhere agrees with one without a capacity to rounding, not
        bitwise.  Keeps the field, restarts the iteration count and the
        convergence state at 0.  Collective."""
        rc = np.ascontiguousarray(np.asarray(rc, dtype=np.float64))
        if rc.shape != tuple(self.model.n):
            raise ValueError(f"set_capacity: shape {rc.shape} != grid {tuple(self.model.n)}")
        self._ensure()
        self._s.set_capacity(rc)

    def clear_capacity(self) -> None:
        """Back to one capacity everywhere: the schedule and the bits of a run
        that never had one."""
        self._s.clear_capacity()

    def set_field(self, T) -> None:
        """User initial condition with its Dirichlet data: the boundary vertices
        of ``T`` (global shape) become the fixed wall values, its interior T^0;
        iteration 0 follows.  ``error_percent`` keeps measuring against T = y,
        which is only meaningful for the reference problem.  Collective."""
        T = self._global_array(T, "set_field")
        self._ensure()
        self._s.set_field(T)

    def prepare_steps(self, n: int) -> None:
        """Capture (untimed) the hipGraph that ``step(n)`` will replay."""
        self._ensure()
        self._s.prepare_steps(int(n))

    def state(self) -> Dict:
        """Convergence state (iter, conv_iter, done, fault, norm, last_residual, ...).

        With the monotone check (Solver::resolve_coarse) the first call after a
        multi-rank run converged inside a sweep that computed only its last
        residual replays that sweep and all-reduces its residuals: call it on
        every rank then (``run()`` already does)."""
        return dict(self._s.state())

    # -- data ------------------------------------------------------------------
    def gather(self) -> Optional[np.ndarray]:
        """Global field (N0, N1, N2) as float64 on the root process, else None."""
        return self._s.gather_global()

    def local_field(self, idx: int = 0, ghosts: bool = False) -> np.ndarray:
        return self._s.local_field(idx, ghosts)

    def error_percent(self) -> Tuple[float, float]:
        g, loc = self._s.compute_error()
        return 100.0 * g, 100.0 * loc

    def heat_balance(self) -> Dict:
        """Where the heat is and where it goes, summed on the device over the
        updated points (global indices 1 .. N - 2) of the current field: ``heat``
        (hx hy hz sum T; with a heat capacity hx hy hz sum rc T, and the dict then has ``capacity``: True), ``t_min`` / ``t_max`` (NaNs ignored), ``nonfinite`` (the
        count of NaN / Inf values), ``flow`` per face ``{"x-": ..., ...}`` (positive:
        into the body; exactly 0.0 on an insulated face), ``source_power`` and
        ``imbalance``, the sum of the flows and the source power: the rate of
        change of ``heat`` that the scheme applies at this instant.  Every sum is
        accumulated in double-double on a fixed reduction shape: a repeated
        call returns the same bits, and decompositions of one process agree to
        the last rounding (docs/ARCHITECTURE.md, "Heat balance").  Synchronises;
        collective; the same dict on every rank."""
        self._ensure()
        return dict(self._s.heat_balance())

    def solve_steady(self, tol: float = 1e-8, max_iter: Optional[int] = None) -> Dict:
        """Solve for the steady state directly: unpreconditioned conjugate
        gradients on the device, from the current field (``set_field`` gives the
        initial guess and the Dirichlet wall values), on the symmetric positive
        definite system ``G(T) - T = 0`` of the current mode (conductivity,
        source, insulated and convective faces), until the residual's 2-norm is
        ``tol`` times the initial one or ``max_iter`` iterations (default
        ``10 (Nx + Ny + Nz)``).  The solution becomes the current field and the
        time-step state restarts at iteration 0, as after ``set_field``.

        Returns ``converged`` (judged on the recomputed residual ``b - A x``),
        ``iterations``, ``residual`` (relative, from the recurrence),
        ``true_residual`` (relative, recomputed), ``r0_norm``, ``seconds``,
        ``restarts`` (from the true residual, when the recurrence met ``tol``
        and ``b - A x`` did not) and ``status``.  A repeated solve from the same
        field returns the same bits; decompositions agree to the tolerance, not
        bitwise.  fp64 only; not with ``compat``; a system with neither a
        Dirichlet face nor a convective face with a positive coefficient is
        singular: each a ``UsageError``.  Synchronises; collective."""
        self._ensure()
        return dict(self._s.solve_steady(float(tol), 0 if max_iter is None else int(max_iter)))

    def step_implicit(self, steps: int, m: float, theta: float = 1.0, tol: float = 1e-8,
                      max_iter: Optional[int] = None) -> Dict:
        """Implicit time steps: ``steps`` steps, each ``m`` > 0 explicit time steps
        long, with ``theta`` in [0.5, 1] (1 backward Euler, 0.5 Crank-Nicolson).
        One step solves ``R (T' - T) = m [theta r(T') + (1 - theta) r(T)]`` with
        ``r(T) = G(T) - T`` the explicit increment of the current mode without
        the capacity and ``R = diag(rc)`` (the heat capacity is honoured here),
        as ``(R + theta m A) d = r(T)``, ``T' = T + m d``, by the conjugate
        gradients of ``solve_steady`` from ``d = 0`` until the residual's 2-norm
        is ``tol`` times ``||r(T)||`` or ``max_iter`` iterations per step
        (default ``10 (Nx + Ny + Nz)``).  Every mode of ``solve_steady`` works,
        and so do a capacity and a body with every face insulated.  The result
        becomes the current field and the time-step state restarts at
        iteration 0, as after ``set_field``.

        Returns ``steps_done``, ``time_advanced`` (``steps_done * m``),
        ``iterations`` (total) and ``step_iterations`` (per step), ``residual``,
        ``true_residual`` and ``r0_norm`` of the last step, ``restarts``,
        ``status``, ``seconds`` and ``converged`` (every step's recomputed
        residual within ``tol``).  A step whose ``r(T)`` is zero takes no
        iteration and leaves the field's bits alone.  A non-finite ``r . r``
        gives ``"breakdown"``: the field stays as it was before that step and
        the call returns.  A step that stops at ``max_iter`` is applied and ends
        the call.  Same call, same bits; decompositions agree to the tolerance.
        fp64 only; not with ``compat``; ``m``, ``theta``, ``tol`` or ``steps``
        out of range: each a ``UsageError``.  Synchronises; collective."""
        self._ensure()
        return dict(self._s.step_implicit(int(steps), float(m), float(theta), float(tol),
                                          0 if max_iter is None else int(max_iter)))

    def write_tecplot(self, path: str = "output/out.dat", layout: str = "auto") -> None:
        self._s.write_tecplot(path, layout)

    def save_checkpoint(self, path: str) -> None:
        self._s.save_checkpoint(path)

    def load_checkpoint(self, path: str) -> None:
        self._s.load_checkpoint(path)

    # -- introspection -----------------------------------------------------------
    @property
    def native(self):
        return self._s

    @property
    def dims(self):
        return tuple(self._s.dims)

    @property
    def backend(self) -> str:
        return self._s.backend_name

    @property
    def kernel(self) -> str:
        return self._s.kernel_name

    @property
    def is_root(self) -> bool:
        return self._s.is_root

    @property
    def interior_points(self) -> int:
        return self._s.interior_points
