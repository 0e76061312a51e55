"""Python host over the libpucfem C ABI: contexts, the reference's step loops, solve().

The reference scripts are module-level programs (StokesColor.py:436-602, StokesFood.py:356-541,
heatEq.py:218-335, poisson.py:218-296).  This module performs the same setup (pairs, Dirichlet
sets, squirmer boundary values, Poisson load) on the host with the reference's numpy semantics and
hands the hot path -- assembly, every solve, div/grad, BCs, advection, tracers -- to the HIP library.
"""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .mesh import Mesh, boundary_sets, filter_wall_pairs, find_boundary_pairs, INNER_BOUNDARY_MARKER

SCHEMES = {"color": _lib.STOKES_COLOR, "food": _lib.STOKES_FOOD, "heat": _lib.HEAT, "poisson": _lib.POISSON}
# fields of pucfem_sample_points / pucfem_raster by name: (enum, components)
SAMPLE_FIELDS = {"u": (_lib.F_U, 2), "u_star": (_lib.F_USTAR, 2), "p": (_lib.F_P, 1), "p2": (_lib.F_P2, 1),
                 "div_star": (_lib.F_DIV_STAR, 1), "div_u": (_lib.F_DIV_U, 1), "final_div": (_lib.F_FINAL_DIV, 1),
                 "c": (_lib.F_C, 1), "vorticity": (_lib.F_VORTICITY, 1)}
FLOW_KEYS = ("max_vorticity", "enstrophy", "kinetic_energy", "max_speed")
_SAMPLE_NCOMP = {f: n for f, n in SAMPLE_FIELDS.values()}
LOADS_KEYS = _lib.LOADS_KEYS  # pucfem_swimmer_loads' ten values, in order
LOADS_SUMS = (("force_x", 0, 2), ("force_y", 1, 3), ("torque", 4, 5), ("power", 6, 7))


def loads_dict(v):
    """The ten values of pucfem_swimmer_loads (last axis of v) by name, with the pressure and viscous parts' sums
    force_x, force_y, torque and power.  The parts stay separate: the splitting scheme's pressure is its own."""
    v = np.asarray(v, dtype=np.float64)
    d = {k: (float(v[q]) if v.ndim == 1 else v[..., q].copy()) for q, k in enumerate(LOADS_KEYS)}
    for name, a, b in LOADS_SUMS:
        d[name] = d[LOADS_KEYS[a]] + d[LOADS_KEYS[b]]
    return d


ADVECTION_NAMES = ("sl", "maccormack")  # pucfem_set_advection's schemes, by PUCFEM_ADV_SL / PUCFEM_ADV_MACCORMACK


def advection_scheme(name):
    """The PUCFEM_ADV_* scheme of advection='sl' | 'maccormack' (an int passes through)."""
    if isinstance(name, str):
        if name not in ADVECTION_NAMES:
            raise ValueError(f"advection must be one of {ADVECTION_NAMES}, got {name!r}")
        return ADVECTION_NAMES.index(name)
    if int(name) not in (0, 1):
        raise ValueError(f"advection must be one of {ADVECTION_NAMES}, got {name!r}")
    return int(name)


TRAJECTORY_NAMES = ("euler", "midpoint")  # pucfem_set_trajectory's orders, PUCFEM_TRJ_EULER / PUCFEM_TRJ_MIDPOINT


def _stretch_flag(on):
    """tracer_stretch= as a bool (a bool or numpy bool only: a name or a number is a mistake)."""
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError(f"tracer_stretch must be True or False, got {on!r}")
    return bool(on)


def trajectory_order(name):
    """The PUCFEM_TRJ_* order of trajectory='euler' | 'midpoint' (an int 1 | 2 passes through)."""
    if isinstance(name, str):
        if name not in TRAJECTORY_NAMES:
            raise ValueError(f"trajectory must be one of {TRAJECTORY_NAMES}, got {name!r}")
        return TRAJECTORY_NAMES.index(name) + 1
    if isinstance(name, bool) or int(name) not in (_lib.TRJ_EULER, _lib.TRJ_MIDPOINT):
        raise ValueError(f"trajectory must be one of {TRAJECTORY_NAMES}, got {name!r}")
    return int(name)


def dye_field(name):
    """The pucfem_field value of a dye channel's name "dye0" .. "dye15" (PUCFEM_F_DYE0 + k); None for a name that is
    not of that form at all, ValueError for "dye" followed by anything but a channel index below 16."""
    if not (isinstance(name, str) and name.startswith("dye")):
        return None
    k = name[3:]
    if not (k.isascii() and k.isdigit() and str(int(k)) == k and int(k) < _lib.MAX_DYES):
        raise ValueError(f"unknown field {name!r}: the dye channels are 'dye0' .. 'dye{_lib.MAX_DYES - 1}'")
    return _lib.F_DYE0 + int(k)


class Buoyancy:
    """Boussinesq buoyancy of the dye: f = g * sum_t beta_t * (s_t - ref_t), with s_t the dye c ("c") or a dye
    channel ("dye0" .. "dye15") at the start of the step.  terms: {name: (beta, ref)}, summed in the order given."""

    def __init__(self, g=(0.0, -1.0), terms=None):
        self.g = tuple(float(v) for v in np.asarray(g, dtype=np.float64).reshape(-1))
        if len(self.g) != 2:
            raise ValueError("buoyancy: g is a pair")
        terms = {"c": (1.0, 0.0)} if terms is None else dict(terms)
        if not 1 <= len(terms) <= 1 + _lib.MAX_DYES:
            raise ValueError(f"buoyancy: 1 .. {1 + _lib.MAX_DYES} terms, got {len(terms)}")
        self.terms = {}
        for name, br in terms.items():
            if name != "c" and dye_field(name) is None:
                raise ValueError(f"buoyancy: unknown field {name!r}: 'c' or 'dye0' .. 'dye{_lib.MAX_DYES - 1}'")
            beta, ref = br
            self.terms[name] = (float(beta), float(ref))
        vals = list(self.g) + [v for br in self.terms.values() for v in br]
        if not np.all(np.isfinite(vals)):
            raise ValueError("buoyancy: g, beta and ref must be finite")

    def arrays(self):
        """(g (2,), fields int32, beta, ref) as pucfem_set_buoyancy takes them."""
        fields = np.array([_lib.F_C if n == "c" else dye_field(n) for n in self.terms], dtype=np.int32)
        beta = np.array([b for b, _ in self.terms.values()], dtype=np.float64)
        ref = np.array([r for _, r in self.terms.values()], dtype=np.float64)
        return np.array(self.g, dtype=np.float64), fields, beta, ref

    def __repr__(self):
        return f"Buoyancy(g={self.g}, terms={self.terms})"


def _force_args(force, N):
    """force= as (constant, field): None, a pair, or an (N, 2) array."""
    if force is None:
        return None, None
    a = np.asarray(force, dtype=np.float64)
    if a.shape == (2,):
        return a, None
    if a.shape == (N, 2):
        return None, a
    raise ValueError(f"force must be a pair, an ({N}, 2) array or None, got shape {a.shape}")


def _sample_spec(fields):
    """(names, enum array, components) of a field list given by name ("u", "c", "dye3", ...) or pucfem_field
    value."""
    if isinstance(fields, (str, int, np.integer)):
        fields = (fields,)
    names, ids, ncomp = [], [], []
    for f in fields:
        if isinstance(f, str):
            if f not in SAMPLE_FIELDS and dye_field(f) is not None:
                e, n = dye_field(f), 1
            elif f not in SAMPLE_FIELDS:
                raise ValueError(f"unknown field {f!r}: one of {sorted(SAMPLE_FIELDS)} or 'dye0' .. 'dye15'")
            else:
                e, n = SAMPLE_FIELDS[f]
        else:
            e = int(f)
            n = _SAMPLE_NCOMP.get(e, 1)  # (a field the library refuses: it reports the error)
        names.append(f)
        ids.append(e)
        ncomp.append(n)
    return names, np.array(ids, dtype=np.int32), ncomp


def _window(window):
    if window is None:
        return None, None
    w = np.ascontiguousarray(window, dtype=np.float64).reshape(4)
    return w, _lib.dptr(w)


def pixel_centres(width, height, window=None):
    """The (height * width, 2) points a raster samples, row j = 0 (the lowest y) first: pixel (i, j) of the window
    (x0, y0, x1, y1) (None: the unit square) at x0 + (i + 0.5) (x1 - x0) / width, y0 + (j + 0.5) (y1 - y0) / height,
    in the library's operation order (pucfem_raster)."""
    x0, y0, x1, y1 = (0.0, 0.0, 1.0, 1.0) if window is None else [float(v) for v in window]
    x = x0 + (np.arange(width, dtype=np.float64) + 0.5) * (x1 - x0) / float(width)
    y = y0 + (np.arange(height, dtype=np.float64) + 0.5) * (y1 - y0) / float(height)
    X, Y = np.meshgrid(x, y)
    return np.ascontiguousarray(np.stack([X.ravel(), Y.ravel()], 1))


def _streamline_args(seeds, h, nsteps, unit, order, both, vmin):
    """(seeds (n, 2), flags) of a streamline call; order 2: midpoint, 1: Euler."""
    if order not in (1, 2):
        raise ValueError("order is 2 (midpoint) or 1 (Euler)")
    P = np.ascontiguousarray(seeds, dtype=np.float64).reshape(-1, 2)
    flags = (_lib.SLN_UNIT if unit else 0) | (_lib.SLN_EULER if order == 1 else 0) | (_lib.SLN_BOTH if both else 0)
    return P, flags


@dataclass
class Streamlines:
    """Lines of Context.streamlines: `points` (lines, nsteps + 1, 2), NaN past a line's end; `status` (lines,) 0
    complete, 1 left the fluid, 2 stagnant, 3 seed outside; `npts` (lines,) the points stored; `values` {field:
    (lines, nsteps + 1) or (lines, nsteps + 1, 2)} at the stored points.  With both=True the first half of the lines
    runs along the flow and the second half against it.  An ensemble's arrays carry a leading member axis."""
    points: np.ndarray
    status: np.ndarray
    npts: np.ndarray
    values: dict = field(default_factory=dict)

    def segments(self):
        """streamline_segments(self.points)"""
        return streamline_segments(self.points)


def streamline_segments(points):
    """Cut lines (..., npoints, 2) for plotting: a list of (k, 2) arrays, k >= 2.  A line's trailing NaNs are
    dropped and it is split where consecutive x differ by more than 0.5 -- a periodic wrap, which would otherwise be
    drawn as a stroke across the whole picture."""
    P = np.asarray(points, dtype=np.float64)
    out = []
    for line in P.reshape((-1,) + P.shape[-2:]):
        ok = ~np.isnan(line).any(axis=1)
        n = int(np.argmin(ok)) if not ok.all() else len(line)
        line = line[:n]
        if n < 2:
            continue
        cuts = np.where(np.abs(np.diff(line[:, 0])) > 0.5)[0] + 1
        out += [seg for seg in np.split(line, cuts) if len(seg) >= 2]
    return out


def _split_images(names, ncomp, img):
    """{name: (..., H, W) or (..., 2, H, W)} from an image stack whose component axis is -3."""
    out, k = {}, 0
    for f, n in zip(names, ncomp):
        out[f] = img[..., k, :, :] if n == 1 else img[..., k:k + n, :, :]
        k += n
    return out


@dataclass
class SquirmerBC:
    """Squirmer boundary condition and physics of the Stokes scripts.

    Defaults are StokesColor.py:28-44 (B1=-2, B2=0, v=0.1); StokesFood.py uses v=1.0, DT=0.01
    and B2 in {0, -5, +5} (neutral / pusher / puller, README.md:43-45)."""

    B1: float = -2.0
    B2: float = 0.0
    nu: float = 0.1
    center: tuple = (0.5, 0.5)
    outer_value: tuple = (0.0, 0.0)
    capture_radius: float = 0.28  # SQUIRMER_RADIUS + 0.03 (StokesFood.py:50-51)
    squirmer_radius: float = 0.25


def squirmer_values(coords, inner, B1, B2, center=(0.5, 0.5)):
    """makeDirBCU inner-body values (StokesColor.py:410-427), evaluated with numpy as the
    reference does (np.arctan2 / np.sin / np.cos, float64)."""
    X = np.asarray(coords, dtype=np.float64)
    rx = X[inner, 0] - center[0]
    ry = X[inner, 1] - center[1]
    th = np.arctan2(ry, rx)
    vt = B1 * np.sin(th) + B2 * np.sin(2 * th)
    return np.stack([vt * -np.sin(th), vt * np.cos(th)], 1)


def stroke_geometry(coords, inner, K, center=(0.5, 0.5)):
    """(shape (n, K), dir (n, 2)) of a stroke's driven nodes `inner`: shape[:, j] = sin((j + 1) theta) and
    dir = (-sin theta, cos theta), formed with the numpy lines of squirmer_values, so that a table row (B1, B2) gives
    that function's bits."""
    X = np.asarray(coords, dtype=np.float64)
    rx = X[inner, 0] - center[0]
    ry = X[inner, 1] - center[1]
    th = np.arctan2(ry, rx)
    shape = np.stack([np.sin((j + 1) * th) for j in range(K)], 1)
    return np.ascontiguousarray(shape), np.ascontiguousarray(np.stack([-np.sin(th), np.cos(th)], 1))


class Stroke:
    """A time-dependent stroke of the squirmer: a periodic table of mode amplitudes, one row per step.  table is
    (P, K) float64, 1 <= P <= 65536 rows and 1 <= K <= 8 modes; column j drives sin((j + 1) theta), so columns 0 and 1
    are B1 and B2 of SquirmerBC.  The k-th step after the stroke was set (k = 0 the first) imposes row
    (start + k) mod P: v_t = sum_j table[row, j] sin((j + 1) theta) along the tangent, the products summed in the
    order of j."""

    def __init__(self, table, start=0):
        t = np.array(table, dtype=np.float64)
        if t.ndim != 2:
            raise ValueError(f"stroke: the table is (P, K), got shape {t.shape}")
        P, K = t.shape
        if not 1 <= K <= _lib.STROKE_MAX_MODES:
            raise ValueError(f"stroke: 1 .. {_lib.STROKE_MAX_MODES} modes, got K = {K}")
        if not 1 <= P <= _lib.STROKE_MAX_PERIOD:
            raise ValueError(f"stroke: 1 .. {_lib.STROKE_MAX_PERIOD} rows, got P = {P}")
        if not np.all(np.isfinite(t)):
            raise ValueError("stroke: the table must be finite")
        if int(start) != start or int(start) < 0:
            raise ValueError("stroke: start is a row count >= 0")
        self.table = np.ascontiguousarray(t)
        self.table.setflags(write=False)
        self.start = int(start)

    @property
    def P(self):
        return self.table.shape[0]

    @property
    def K(self):
        return self.table.shape[1]

    def row(self, k):
        """The table row the k-th step imposes."""
        return (self.start + int(k)) % self.P

    def amplitudes(self, k):
        """The amplitudes (K,) the k-th step imposes."""
        return self.table[self.row(k)].copy()

    @classmethod
    def constant(cls, B1, B2):
        """The steady squirmer SquirmerBC(B1, B2) as a stroke: the same boundary bits at every step."""
        return cls([[B1, B2]])

    @classmethod
    def harmonic(cls, period, B1=(0.0, 0.0, 0.0), B2=(0.0, 0.0, 0.0), *modes, start=0):
        """Each mode a (mean, amp, phase): row k holds mean + amp * np.sin(2 * np.pi * (k + 1) / period + phase)."""
        if int(period) != period or period < 1:
            raise ValueError("stroke: period is a row count >= 1")
        k = np.arange(int(period), dtype=np.float64)
        cols = []
        for mode in (B1, B2) + tuple(modes):
            mean, amp, phase = (float(v) for v in mode)
            cols.append(mean + amp * np.sin(2 * np.pi * (k + 1) / period + phase))
        return cls(np.stack(cols, 1), start)

    @classmethod
    def blinking(cls, period, a, b, duty=0.5, start=0):
        """Piecewise constant: the first round(duty * period) rows hold the amplitudes a, the others b (a pusher /
        puller alternation: a = (B1, -B2), b = (B1, +B2))."""
        if int(period) != period or period < 1:
            raise ValueError("stroke: period is a row count >= 1")
        a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
        if a.shape != b.shape:
            raise ValueError("stroke: the two amplitude tuples have one length")
        if not 0.0 <= duty <= 1.0:
            raise ValueError("stroke: duty is in [0, 1]")
        na = int(round(duty * int(period)))
        return cls(np.stack([a] * na + [b] * (int(period) - na), 0), start)

    def __repr__(self):
        return f"Stroke(P={self.P}, K={self.K}, start={self.start})"


def _check_stroke(stroke):
    if stroke is not None and not isinstance(stroke, Stroke):
        raise ValueError("stroke must be a Stroke or None")
    return stroke


@dataclass
class Tolerances:
    rtol_visc: float = 1e-13
    rtol_pres: float = 1e-12
    rtol_lin: float = 1e-14
    maxit_visc: int = 500
    maxit_pres: int = 200000
    maxit_lin: int = 20000
    warm_start: bool = True
    precond: str = "auto"  # pressure: "jacobi", "mg" (geometric multigrid, needs a refined mesh) or "auto"
    mg_degree: int = 2
    mg_ratio: float = 10.0
    mg_post: int = 0
    mg_rep_nodes: int = 0  # multi-rank: replicate coarse levels up to this size (0: library default)
    mg_single: bool = True  # fp32 V-cycle inside the fp64 CG (same iteration counts, ~30% fewer bytes)
    # fp32 cycle: level operators stored in fp16 (fp32 arithmetic); "coarse": all but the finest.  Off by
    # default: at L7 it saves ~10% of the smoother's bytes but costs ~1 extra CG iteration per solve
    mg_f16_vals: bool | str = False
    index16: bool = True  # int16 column deltas where the operator band fits
    mg_kind: int = 1  # smoother: 1 = Chebyshev on [lmax/mg_ratio, lmax], 4 = fourth-kind Chebyshev
    proj_k: int = 24  # pressure initial guess: A-projection onto up to proj_k solution directions (0: warm start)
    proj_k_visc: int = 0  # the same for the viscous solve's two components (measured: no net gain at L7)
    proj_shared: bool = False  # both pressure solves of a step project onto one shared basis
    # "auto": small meshes (<= 1500 nodes, one rank) solve with precomputed dense inverses and meshes of
    # <= 4096 nodes with a one-workgroup CG; "iterative": the large-mesh multi-kernel CG path on every mesh
    solver_path: str = "auto"
    # "auto": on multigrid hierarchies (>= 2 levels) the rows of the nodes inside the coarse triangles are
    # matrix-free lattice stencils; "assembled": stored SELL rows everywhere
    operators: str = "auto"
    # StokesColor dye update: "semilagrange" (StokesColor.py:347-389) or "implicit" (the FEM advection-
    # diffusion variant of scripts/good_visualization.py:700-718, diffusivity dye_diffusivity; one rank)
    dye: str = "semilagrange"
    dye_diffusivity: float = 1e-3
    # operator assembly: "auto" = on the device when the context has one (bit-identical to the host's), "host"
    assembly: str = "auto"

    @classmethod
    def production(cls, **kw):
        """The settings bench.py measures (and the production-path parity tests check): multigrid-
        preconditioned pressure CG with the fp32 V-cycle, the pressure guess projected onto one basis of
        up to 32 directions shared by both pressure solves,
        int16 column deltas, the extrapolated viscous start, pressure rtol PRODUCTION_RTOL_PRES."""
        # V(3,3) Chebyshev smoothing on [lmax / 15, lmax]: measured at L7 against V(2,2) / ratio 10 and the
        # neighbouring choices (driver command 90.7 -> 97.6 steps/s)
        base = dict(rtol_visc=1e-12, rtol_pres=PRODUCTION_RTOL_PRES, precond="mg", mg_single=True,
                    mg_f16_vals=False, index16=True, mg_degree=3, mg_post=3, mg_ratio=15.0, mg_kind=1,
                    proj_k=32, proj_shared=True, proj_k_visc=0)
        # separate bases per solve (r8d, one box, twice each): 24 -> 106.8 / 107.0, 16 -> 107.1 / 108.5,
        # 12 -> 105.6 / 105.6, 8 -> 99.8 / 100.0 steps/s, pressure iterations 72 / 72 / 76 / 83 (saturated
        # at 16); ONE basis shared by both solves keeps improving with its size (r8l): 16 -> 105.1 / 105.4
        # (73 iterations), 24 -> 106.9 / 107.1 (68), 32 -> 109.5 / 110.1 (63) against separate 16: 107.6 / 107.8
        base.update(kw)
        return cls(**base)


# pressure CG tolerance of the measured configuration (bench.py); tests/test_gpu_production.py checks
# that it keeps every step within 1e-6 of the oracle's exact solves.  tools/rtol_probe.py (48 steps
# on mesh_fine x3, worst deviation from the oracle along the trajectory, r2q):
#   rtol_pres 1e-8: |u| 6.1e-10, |c| 1.1e-8;  1e-7: |u| 6.5e-9, |c| 6.6e-8;  1e-6: |u| 3.0e-8, |c| 5.4e-7
# 1e-7 saves ~20 % of the pressure iterations.  Its margin to the 1e-6 bar depends on the mesh (a
# relative-residual stop bounds the error through the condition number, ~h^-2): 15x at L3 (above), 2.1x
# over the driver window on L7 (worst |dc| 4.7e-7, profiles/r8m_scale_parity.txt); the per-step error past
# the transient on L7 is tests/test_gpu_scale_parity.py::test_production_rtol_L7_per_step_past_transient.
PRODUCTION_RTOL_PRES = 1e-7


class Context:
    """One libpucfem context (one GPU, or host-only with device=-1)."""

    def __init__(self, device=0, dist=None):
        self.h = None  # close() (and __del__) must work when creation fails below
        L = _lib.lib()
        p = ct.c_void_p()
        if dist is None:
            _lib.check(L.pucfem_ctx_create(int(device), ct.byref(p)))
        else:
            rank, world, uid = dist
            buf = (ct.c_uint8 * 128).from_buffer_copy(bytes(uid))
            _lib.check(L.pucfem_ctx_create_dist(int(device), int(rank), int(world), buf, ct.byref(p)))
        self.h = p
        self.L = L
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.L.pucfem_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def _c(self, rc):
        _lib.check(rc, self.h)

    # ---------------------------------------------------------------- setup
    def upload(self, mesh: Mesh, coord_fp32=False):
        X = np.ascontiguousarray(mesh.coords, dtype=np.float64)
        mk = np.ascontiguousarray(mesh.markers, dtype=np.int32)
        T = np.ascontiguousarray(mesh.triangles, dtype=np.int32)
        self._c(self.L.pucfem_mesh_upload(self.h, X.shape[0], _lib.dptr(X), _lib.iptr(mk), T.shape[0],
                                          _lib.iptr(T), int(coord_fp32)))
        self.N = X.shape[0]
        self.T = T.shape[0]
        self.coords = X  # (surface_traction's edge midpoints and lengths)

    def set_pairs(self, kind, pairs):
        P = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
        self._c(self.L.pucfem_set_pairs(self.h, kind, P.shape[0], _lib.lptr(P)))

    def set_dirichlet(self, nodes, values):
        n = np.ascontiguousarray(nodes, dtype=np.int32)
        v = np.ascontiguousarray(values, dtype=np.float64)
        ncomp = 1 if v.ndim == 1 else v.shape[1]
        self._c(self.L.pucfem_set_dirichlet(self.h, len(n), _lib.iptr(n), _lib.dptr(v), ncomp))

    def set_source(self, g_tri):
        g = np.ascontiguousarray(g_tri, dtype=np.float32)
        self._c(self.L.pucfem_set_source(self.h, len(g), _lib.fptr(g)))

    def set_hierarchy(self, base: Mesh, levels: int):
        X = np.ascontiguousarray(base.coords, dtype=np.float64)
        mk = np.ascontiguousarray(base.markers, dtype=np.int32)
        T = np.ascontiguousarray(base.triangles, dtype=np.int32)
        self._c(self.L.pucfem_set_hierarchy(self.h, X.shape[0], _lib.dptr(X), _lib.iptr(mk), T.shape[0],
                                            _lib.iptr(T), int(levels)))
        self.has_hierarchy = levels > 0

    def build(self, scheme, dt, nu=0.0, tol: Tolerances | None = None, capture=0.28, center=(0.5, 0.5), nstrips=0):
        tol = tol or Tolerances()
        mg = tol.precond == "mg" or (tol.precond == "auto" and getattr(self, "has_hierarchy", False))
        p = _lib.Params(scheme=SCHEMES.get(scheme, scheme), nstrips=nstrips, dt=dt, nu=nu, rtol_visc=tol.rtol_visc,
                        rtol_pres=tol.rtol_pres, rtol_lin=tol.rtol_lin, maxit_visc=tol.maxit_visc,
                        maxit_pres=tol.maxit_pres, maxit_lin=tol.maxit_lin, warm_start=int(tol.warm_start),
                        sl_k=10, capture_radius=capture, center_x=center[0], center_y=center[1],
                        precond=int(mg), mg_degree=tol.mg_degree, mg_ratio=tol.mg_ratio, mg_post=tol.mg_post,
                        mg_single=int(tol.mg_single), mg_rep_nodes=tol.mg_rep_nodes,
                        mg_f32_vals=2 if tol.mg_f16_vals == "coarse" else int(not tol.mg_f16_vals),
                        idx32=int(not tol.index16), proj_k=tol.proj_k, proj_k_visc=tol.proj_k_visc,
                        mg_kind=tol.mg_kind, solver_path={"auto": 0, "iterative": 1}[tol.solver_path],
                        assembled={"auto": 0, "assembled": 1}[tol.operators],
                        dye_scheme={"semilagrange": 0, "implicit": 1}[tol.dye], dye_diffusivity=tol.dye_diffusivity,
                        assembly={"auto": 0, "device": 0, "host": 1}[tol.assembly], proj_shared=int(tol.proj_shared))
        self.precond = "mg" if mg else "jacobi"
        self.center = (float(center[0]), float(center[1]))
        self._c(self.L.pucfem_build_operators(self.h, ct.byref(p)))

    # ---------------------------------------------------------------- fields / steps
    def set_field(self, f, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        self._c(self.L.pucfem_set_field(self.h, f, _lib.dptr(a), a.size))

    def get_field(self, f, shape):
        out = np.zeros(shape)
        self._c(self.L.pucfem_get_field(self.h, f, _lib.dptr(out), out.size))
        return out

    def step(self, n=1):
        st = (_lib.StepStats * max(n, 1))()
        self._c(self.L.pucfem_step(self.h, n, st))
        return [st[i] for i in range(n)]

    def sample(self, fields, points):
        """Fields at arbitrary points on the device (pucfem_sample_points; StokesFood.py:482-487's locate and
        interpolate): ({field: (n,) or (n, 2) float64}, triangle ids (n,) int32, -1 where no triangle holds the
        point and the values are NaN).  fields: names ("u", "u_star", "p", "p2", "div_star", "div_u", "final_div",
        "c", "vorticity") or pucfem_field values; points (n, 2), taken as given (no periodic wrap)."""
        names, ids, ncomp = _sample_spec(fields)
        P = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
        n = P.shape[0]
        out = np.zeros((sum(ncomp), n))
        tri = np.zeros(n, dtype=np.int32)
        self._c(self.L.pucfem_sample_points(self.h, len(ids), _lib.iptr(ids), n, _lib.dptr(P), _lib.dptr(out),
                                            _lib.iptr(tri)))
        vals, k = {}, 0
        for f, nc in zip(names, ncomp):
            vals[f] = out[k].copy() if nc == 1 else np.ascontiguousarray(out[k:k + nc].T)
            k += nc
        return vals, tri

    def raster(self, fields, width, height, window=None):
        """Fields as width x height images of `window` = (x0, y0, x1, y1) (None: the unit square), rasterised on
        the device (pucfem_raster; the frames of scripts/good_visualization2.py:536-571 without a copy of the
        fields): {field: float32 (height, width) or (2, height, width)}, row 0 the lowest y, NaN where no triangle
        holds the pixel centre (outside the mesh, inside the swimmer)."""
        names, ids, ncomp = _sample_spec(fields)
        w, wp = _window(window)
        # (a non-positive size: an empty buffer, and the library reports the error)
        img = np.zeros((sum(ncomp), max(int(height), 0), max(int(width), 0)), dtype=np.float32)
        self._c(self.L.pucfem_raster(self.h, len(ids), _lib.iptr(ids), int(width), int(height), wp, _lib.fptr(img)))
        return _split_images(names, ncomp, img)

    def streamlines(self, seeds, h, nsteps, unit=True, order=2, both=False, vmin=0.0, fields=()):
        """The frozen velocity integrated from `seeds` (n, 2) on the device (pucfem_streamlines; the reference's
        ax.streamplot): a Streamlines.  h: the signed step (negative: against the flow) -- an arc length in the max
        norm with unit=True, a time otherwise; order 2 midpoint, 1 Euler; both=True: every seed forwards (lines
        [0, n)) and backwards (lines [n, 2 n)); vmin: a line ends (status 2) where both |u_x| and |u_y| are <= vmin;
        fields: names as for sample(), read at every stored point."""
        P, flags = _streamline_args(seeds, h, nsteps, unit, order, both, vmin)
        names, ids, ncomp = _sample_spec(fields)
        n, lines, ns = P.shape[0], P.shape[0] * (2 if both else 1), max(int(nsteps), 0) + 1
        # (arguments the library refuses: small buffers, and it reports the error)
        big = n < 1 or ns * lines > (1 << 26)
        pts = np.zeros((1, 1, 2) if big else (ns, lines, 2))
        st = np.zeros(1 if big else lines, dtype=np.int32)
        npts = np.zeros(1 if big else lines, dtype=np.int32)
        val = np.zeros((sum(ncomp), 1, 1) if big else (sum(ncomp), ns, lines)) if ids.size else None
        self._c(self.L.pucfem_streamlines(self.h, n, _lib.dptr(P), float(h), int(nsteps), flags, float(vmin), len(ids),
                                          _lib.iptr(ids) if ids.size else None, _lib.dptr(pts), _lib.iptr(st),
                                          _lib.iptr(npts), _lib.dptr(val) if val is not None else None))
        vals, k = {}, 0
        for f, nc in zip(names, ncomp):
            vals[f] = val[k].T if nc == 1 else val[k:k + nc].transpose(2, 1, 0)
            k += nc
        return Streamlines(pts.transpose(1, 0, 2), st, npts, vals)

    def streamlines_probe(self, seeds, h, nsteps, unit=True, order=2, both=False, vmin=0.0, iters=5):
        """Kernel time of streamlines() without fields (pucfem_streamlines_probe; tools/streamline_bench.py)."""
        P, flags = _streamline_args(seeds, h, nsteps, unit, order, both, vmin)
        o = (ct.c_double * 2)()
        self._c(self.L.pucfem_streamlines_probe(self.h, P.shape[0], _lib.dptr(P), float(h), int(nsteps), flags,
                                                float(vmin), int(iters), o))
        return dict(kernel_ms=o[0], output_bytes=int(o[1]))

    def raster_probe(self, fields, width, height, window=None, iters=10):
        """Kernel time and pixel bookkeeping of raster() (pucfem_raster_probe; tools/raster_bench.py)."""
        _, ids, _ = _sample_spec(fields)
        w, wp = _window(window)
        o = (ct.c_double * 4)()
        self._c(self.L.pucfem_raster_probe(self.h, len(ids), _lib.iptr(ids), int(width), int(height), wp, int(iters), o))
        return dict(kernel_ms=o[0], not_found=int(o[1]), first_face=int(o[2]), image_bytes=int(o[3]))

    def apply(self, op, x, out_shape):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros(out_shape)
        self._c(self.L.pucfem_apply(self.h, op, _lib.dptr(x), _lib.dptr(y)))
        return y

    def solve(self, op, b, x0=None, rtol=1e-13, maxit=100000):
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.zeros_like(b) if x0 is None else np.ascontiguousarray(x0, dtype=np.float64).copy()
        it = ct.c_int32()
        self._c(self.L.pucfem_solve(self.h, op, _lib.dptr(b), _lib.dptr(x), rtol, maxit, ct.byref(it)))
        return x, it.value

    def info(self):
        o = (ct.c_int64 * 12)()
        self._c(self.L.pucfem_info(self.h, o))
        keys = ["N", "T", "nnz_P", "nnz_Pp", "n_own", "n_ghost", "sell_P", "sell_Pp", "n_pairs", "n_dirichlet"]
        d = dict(zip(keys, list(o)))
        d["index16_P"], d["index16_Pp"], d["mg_f16_vals"] = bool(o[10] & 1), bool(o[10] & 2), bool(o[10] & 4)
        d["mg_levels"] = o[11]
        return d

    def path_info(self):
        """The code path of the step (pucfem_path_info)."""
        o = (ct.c_int64 * 8)()
        self._c(self.L.pucfem_path_info(self.h, o))
        visc = {0: "dense", 1: "block", 2: "multi-kernel"}
        pres = {0: "dense", 1: "block", 2: "jacobi-cg", 3: "mg-pcg"}
        return dict(viscous=visc[o[0]], pressure=pres[o[1]], reseeds=o[2], basis_p=o[3], basis_p2=o[4],
                    visc_extrap_order=o[5], proj_k=o[6], lattice=bool(o[7] & 1),
                    sl_locator="lattice" if o[7] & 2 else "records",
                    viscous_iteration="chebyshev" if o[7] & 4 else "cg",
                    visc_check_failed=bool(o[7] & 8),
                    visc_step_pairs=bool(o[7] & 16),
                    mg_step_pairs=bool(o[7] & 32),
                    pending_pressure_directions=bool(o[7] & 64),
                    single_reduction_pcg=bool(o[7] & 128))

    def proj_probe(self, iters=20):
        """The pressure projection's two basis passes timed outside the step (pucfem_proj_probe); the state stays."""
        o = (ct.c_double * 6)()
        self._c(self.L.pucfem_proj_probe(self.h, int(iters), o))
        return dict(mdot2_ms=o[0], pcomb_ms=o[1], mdot2_bytes=o[2], pcomb_bytes=o[3], m=int(o[4]), m_pcomb=int(o[5]))

    def visc_interval(self):
        """[lo, hi] of the viscous Chebyshev iteration (pucfem_visc_interval)."""
        o = (ct.c_double * 2)()
        self._c(self.L.pucfem_visc_interval(self.h, o))
        return float(o[0]), float(o[1])

    def mg_lmax(self, level):
        """The multigrid smoothing interval's top on `level` (pucfem_mg_lmax): lmax in use, the device power
        iteration's quotient (0: host), the host fp64 power iteration's quotient, the Gershgorin bound."""
        o = (ct.c_double * 4)()
        self._c(self.L.pucfem_mg_lmax(self.h, int(level), o))
        return dict(lmax=o[0], lam_device=o[1], lam_host=o[2], gershgorin=o[3])

    MG_PIECES = ("resid", "smooth0", "smoothx", "restrict", "prolong", "coarse", "cycle", "precondition")

    def mg_level_size(self, level):
        """Nodes of multigrid level `level` (0 = coarsest)."""
        n, nnz = ct.c_int64(), ct.c_int64()
        self._c(self.L.pucfem_host_get_csr(self.h, 100 + 3 * int(level), ct.byref(n), ct.byref(nnz), None, None, None))
        return n.value

    def mg_probe(self, piece, level, b=None, x=None):
        """One piece of the pressure V-cycle on caller-numbered fp64 vectors (pucfem_mg_probe; test
        infrastructure).  piece: a name of MG_PIECES.  b, x: the piece's inputs as include/pucfem.h lists them
        (b lives on level - 1 for "prolong", the output on level - 1 for "restrict").  Returns the output vector,
        and for "precondition" the pair (z, <r, z>)."""
        k = self.MG_PIECES.index(piece)
        level = int(level)
        # (sizes: the library reads and writes whole level vectors; a level that does not exist is its error)
        lv = {"restrict": (None, level, level - 1), "prolong": (level - 1, level, level)}.get(piece, (level, level, level))
        if piece == "coarse":
            lv = (0, None, 0)
        need = [None if q is None or q < 0 else self.mg_level_size(q) for q in lv]
        b = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
        x = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
        for name, v, n in (("b", b, need[0]), ("x", x, need[1])):
            if v is not None and n is not None and v.shape != (n,):
                raise ValueError(f"mg_probe {piece}: {name} has shape {v.shape}, level vector is ({n},)")
        out = np.zeros(need[2] if need[2] is not None else 1)
        rz = ct.c_double(0.0)
        self._c(self.L.pucfem_mg_probe(self.h, k, int(level), None if b is None else _lib.dptr(b),
                                       None if x is None else _lib.dptr(x), _lib.dptr(out),
                                       ct.cast(ct.byref(rz), ct.POINTER(ct.c_double))))
        return (out, rz.value) if piece == "precondition" else out

    def proj_info(self):
        """Projected pressure guesses (pucfem_proj_info): re-seeds, monitor restarts, last guess residuals."""
        o = (ct.c_double * 4)()
        self._c(self.L.pucfem_proj_info(self.h, o))
        return dict(reseeds=int(o[0]), restarts=int(o[1]), guess_rel=(o[2], o[3]))

    def tracer_info(self, member=None):
        """The context's tracer set, or that of ensemble member `member` (pucfem_tracer_info): tracers, eaten and
        lost (non-finite position) counts reduced on the device, tracer steps since the set was set, and the last
        tracer launch's blocks (1: the one-block kernel) and threads per block."""
        o = (ct.c_int64 * 6)()
        self._c(self.L.pucfem_tracer_info(self.h, -1 if member is None else int(member), o))
        return dict(tracers=o[0], eaten=o[1], nonfinite=o[2], steps=o[3], blocks=o[4], threads=o[5])

    def dyes_info(self):
        """The context's dye channels (pucfem_dyes_info): their number, the channel steps since they were set, the
        not-found rows of the last channel launch and the device bytes held for them."""
        o = (ct.c_int64 * 4)()
        self._c(self.L.pucfem_dyes_info(self.h, o))
        return dict(channels=o[0], steps=o[1], notfound=o[2], bytes=o[3])

    def dyes_mixing(self):
        """(K, 3): (I, mu, var) of every dye channel over marker == 0 (pucfem_dyes_mixing)."""
        K = self.dyes_info()["channels"]
        out = np.zeros((K, 3))
        self._c(self.L.pucfem_dyes_mixing(self.h, _lib.dptr(out) if K else None))
        return out

    def dyes_probe(self, nch, iters=10):
        """Kernel time of one channel launch with nch channels (pucfem_dyes_probe; tools/dye_bench.py)."""
        o = (ct.c_double * 2)()
        self._c(self.L.pucfem_dyes_probe(self.h, int(nch), int(iters), o))
        return dict(kernel_ms=o[0], algo_bytes=o[1])

    def set_inertia(self, on):
        """Switch the inertial term on or off (pucfem_set_inertia): with it on, every step advects the velocity by
        itself, u_a = SL(u; u, dt), in front of the viscous solve."""
        self._c(self.L.pucfem_set_inertia(self.h, 1 if on else 0))

    def inertia_info(self):
        """The context's inertial term (pucfem_inertia_info): whether it is on, the inertial steps since it was
        switched on, the not-found rows of the last inertial launch and the device bytes held for it."""
        o = (ct.c_int64 * 4)()
        self._c(self.L.pucfem_inertia_info(self.h, o))
        return dict(on=bool(o[0]), steps=o[1], notfound=o[2], bytes=o[3])

    def set_tracer_diffusion(self, D, seed=0):
        """Brownian tracers (pucfem_set_tracer_diffusion): every free tracer also takes a random-walk increment of
        diffusivity D per tracer step, reproducible from the 64-bit seed; D = 0 is the plain step."""
        self._c(self.L.pucfem_set_tracer_diffusion(self.h, float(D), int(seed) & 0xFFFFFFFFFFFFFFFF))

    def tracer_diffusion(self, member=-1):
        """(D, seed) of the context (member = -1) or of an ensemble member (pucfem_get_tracer_diffusion)."""
        d, s = ct.c_double(0.0), ct.c_uint64(0)
        self._c(self.L.pucfem_get_tracer_diffusion(self.h, int(member), ct.byref(d), ct.byref(s)))
        return d.value, int(s.value)

    def tracer_probe(self, dt, iters=20):
        """Kernel time of one tracer launch on the current u, tracers and diffusion setting (pucfem_tracer_probe;
        tools/brownian_bench.py).  The tracers move."""
        o = (ct.c_double * 2)()
        self._c(self.L.pucfem_tracer_probe(self.h, float(dt), int(iters), o))
        return dict(kernel_ms=o[0], tracers=int(o[1]))

    # ---- tracer stretching (pucfem_set_tracer_stretch)
    def set_tracer_stretch(self, on, member=None):
        """Tracer stretching of the context (member=None; pucfem_set_tracer_stretch) or of ensemble member `member`
        (-1: every member; pucfem_ens_set_tracer_stretch): the tracers carry the deformation gradient F of the flow
        map along their paths."""
        if member is None:
            self._c(self.L.pucfem_set_tracer_stretch(self.h, int(_stretch_flag(on))))
        else:
            self._c(self.L.pucfem_ens_set_tracer_stretch(self.h, int(member), int(_stretch_flag(on))))

    def stretch_info(self, member=None, T=None):
        """pucfem_tracer_stretch_info of the context (member=None) or of an ensemble member: the flag, the tracer steps
        taken with it on since F was last reset, the tracers with finite F, of those the ones with det F <= 0, the
        largest and smallest Cauchy-Green eigenvalue lam, the sum of log(lam) and the number of its terms, reduced on
        the device.  T: the elapsed time; adds ftle_mean = sum_log / (2 T terms) and ftle_max = log(lam_max) / (2 T)."""
        o = (ct.c_double * 8)()
        self._c(self.L.pucfem_tracer_stretch_info(self.h, -1 if member is None else int(member), o))
        d = dict(on=bool(o[0]), steps=int(o[1]), finite=int(o[2]), folded=int(o[3]), lam_max=o[4], lam_min=o[5],
                 sum_log=o[6], terms=int(o[7]))
        if T is not None:
            T = float(T)
            with np.errstate(divide="ignore", invalid="ignore"):
                d["ftle_mean"] = float(np.float64(d["sum_log"]) / np.float64(2.0 * T * d["terms"]))
                d["ftle_max"] = float(np.log(np.float64(d["lam_max"])) / np.float64(2.0 * T))
        return d

    def inertia_probe(self, iters=10):
        """Kernel time of one inertial launch on the current u (pucfem_inertia_probe; tools/inertia_bench.py)."""
        o = (ct.c_double * 2)()
        self._c(self.L.pucfem_inertia_probe(self.h, int(iters), o))
        return dict(kernel_ms=o[0], algo_bytes=o[1])

    # ---- body forces (pucfem_set_force, pucfem_set_buoyancy)
    def set_force(self, constant=None, field=None):
        """The uniform force (a pair or None) and the nodal force field ((N, 2) or None) of the steps' right-hand
        side r = base + dt * f (pucfem_set_force); both None switches that part off."""
        F = None if constant is None else np.ascontiguousarray(constant, dtype=np.float64)
        if F is not None and F.shape != (2,):
            raise ValueError(f"force: the uniform force is a pair, got shape {F.shape}")
        fn = None if field is None else np.ascontiguousarray(field, dtype=np.float64)
        self._c(self.L.pucfem_set_force(self.h, None if F is None else _lib.dptr(F),
                                        None if fn is None else _lib.dptr(fn)))

    def set_buoyancy(self, buoyancy=None):
        """Boussinesq buoyancy of the dye (pucfem_set_buoyancy): a Buoyancy, or None for off."""
        if buoyancy is None:
            self._c(self.L.pucfem_set_buoyancy(self.h, None, 0, None, None, None))
            return
        if not isinstance(buoyancy, Buoyancy):
            raise ValueError("buoyancy must be a Buoyancy or None")
        g, fields, beta, ref = buoyancy.arrays()
        self._c(self.L.pucfem_set_buoyancy(self.h, _lib.dptr(g), len(fields), _lib.iptr(fields), _lib.dptr(beta),
                                           _lib.dptr(ref)))

    def force_info(self):
        """The context's body force (pucfem_force_info): which terms are present, the forced steps since the setting
        last changed, the buoyancy terms and the device bytes held."""
        o = (ct.c_int64 * 4)()
        self._c(self.L.pucfem_force_info(self.h, -1, o))
        return dict(mask=int(o[0]), uniform=bool(o[0] & _lib.FORCE_UNIFORM), nodal=bool(o[0] & _lib.FORCE_NODAL),
                    buoyancy=bool(o[0] & _lib.FORCE_BUOYANCY), steps=o[1], terms=o[2], bytes=o[3])

    def force_apply(self, base, dt):
        """r = base + dt * f (N, 2) from the context's current force setting and dye fields, through the step's
        kernel on scratch buffers (pucfem_force_apply); the step's state is not touched."""
        b = np.ascontiguousarray(base, dtype=np.float64)
        if b.shape != (self.N, 2):
            raise ValueError(f"force_apply: base must be ({self.N}, 2), got {b.shape}")
        out = np.zeros_like(b)
        self._c(self.L.pucfem_force_apply(self.h, _lib.dptr(b), float(dt), _lib.dptr(out)))
        return out

    def force_probe(self, iters=10):
        """Kernel time of one k_force_rhs launch with the current setting (pucfem_force_probe; tools/force_bench.py)."""
        o = (ct.c_double * 2)()
        self._c(self.L.pucfem_force_probe(self.h, int(iters), o))
        return dict(kernel_ms=o[0], algo_bytes=o[1])

    # ---- time-dependent strokes (pucfem_set_stroke)
    def set_stroke(self, stroke, nodes=None, shape=None, dirs=None, member=None):
        """The stroke of the context's steps (member=None, pucfem_set_stroke) or of ensemble member `member` (-1: all;
        pucfem_ens_set_stroke): a Stroke with the driven nodes (caller numbering), their shapes (n, K) and directions
        (n, 2), or None to clear it."""
        if stroke is None:
            if member is None:
                self._c(self.L.pucfem_set_stroke(self.h, 0, 0, None, 0, None, None, None, 0))
            else:
                self._c(self.L.pucfem_ens_set_stroke(self.h, int(member), 0, 0, None, 0, None, None, None, 0))
            return
        nd = np.ascontiguousarray(nodes, dtype=np.int32)
        sh = np.ascontiguousarray(shape, dtype=np.float64)
        dr = np.ascontiguousarray(dirs, dtype=np.float64)
        if sh.shape != (len(nd), stroke.K) or dr.shape != (len(nd), 2):
            raise ValueError(f"stroke: shapes ({len(nd)}, {stroke.K}) and directions ({len(nd)}, 2), got {sh.shape} "
                             f"and {dr.shape}")
        args = (stroke.K, stroke.P, _lib.dptr(stroke.table), len(nd), _lib.iptr(nd), _lib.dptr(sh), _lib.dptr(dr),
                stroke.start)
        if member is None:
            self._c(self.L.pucfem_set_stroke(self.h, *args))
        else:
            self._c(self.L.pucfem_ens_set_stroke(self.h, int(member), *args))

    def stroke_info(self, member=-1):
        """pucfem_stroke_info of the context (member=-1) or an ensemble member: modes K (0: off), period P, start row,
        steps taken since the stroke was set, the row the next step imposes, driven nodes."""
        o = (ct.c_int64 * 6)()
        self._c(self.L.pucfem_stroke_info(self.h, int(member), o))
        return dict(K=int(o[0]), P=int(o[1]), start=int(o[2]), steps=int(o[3]), row=int(o[4]), nodes=int(o[5]))

    def get_dirichlet(self, count, ncomp=2, member=-1):
        """The Dirichlet values the device holds now, (count, ncomp) in the order of the list given to set_dirichlet
        (pucfem_get_dirichlet)."""
        out = np.zeros((int(count), ncomp) if ncomp > 1 else (int(count),))
        self._c(self.L.pucfem_get_dirichlet(self.h, int(member), _lib.dptr(out)))
        return out

    def stroke_apply(self, row, count, member=-1):
        """Row `row` of the stroke through the step's kernel on a scratch copy of the Dirichlet values
        (pucfem_stroke_apply), (count, 2) in the list's order; nothing of the step's state is touched."""
        out = np.zeros((int(count), 2))
        self._c(self.L.pucfem_stroke_apply(self.h, int(member), int(row), _lib.dptr(out)))
        return out

    def stroke_probe(self, iters=10):
        """Kernel time of one k_stroke_bc launch with the current stroke (pucfem_stroke_probe; tools/stroke_bench.py)."""
        o = (ct.c_double * 2)()
        self._c(self.L.pucfem_stroke_probe(self.h, int(iters), o))
        return dict(kernel_ms=o[0], algo_bytes=o[1])

    def set_advection(self, what, scheme):
        """The advection scheme (pucfem_set_advection) of the dye (what = ADV_DYE), of the inertial step's velocity
        (ADV_VELOCITY) or of both (their sum): 'sl' the reference's first-order step, 'maccormack' two of them and
        a clamp (second order)."""
        self._c(self.L.pucfem_set_advection(self.h, int(what), advection_scheme(scheme)))

    def advection_info(self):
        """pucfem_advection_info: the two schemes, the MacCormack steps since each was switched on, the counts of
        the last launch of each (rows whose back-trace / forward trace found no triangle, clamped values) and the
        device bytes held."""
        o = (ct.c_int64 * 11)()
        self._c(self.L.pucfem_advection_info(self.h, o))
        return dict(dye=ADVECTION_NAMES[o[0]], velocity=ADVECTION_NAMES[o[1]], dye_steps=o[2], velocity_steps=o[3],
                    dye_counts=(o[4], o[5], o[6]), velocity_counts=(o[7], o[8], o[9]), bytes=o[10])

    def advection_probe(self, what, nch=1, iters=10):
        """Kernel times of the two MacCormack passes (pucfem_advection_probe; tools/maccormack_bench.py)."""
        o = (ct.c_double * 4)()
        self._c(self.L.pucfem_advection_probe(self.h, int(what), int(nch), int(iters), o))
        return dict(pass1_ms=o[0], pass2_ms=o[1], pass1_bytes=o[2], pass2_bytes=o[3])

    def set_trajectory(self, what, order):
        """The trajectory order (pucfem_set_trajectory) of the dye (what = TRJ_DYE), of the inertial step's velocity
        (TRJ_VELOCITY), of the tracers (TRJ_TRACERS) or of several (their sum): 'euler' one straight step of the
        velocity at the starting point, 'midpoint' a step with the velocity read half a step along it."""
        self._c(self.L.pucfem_set_trajectory(self.h, int(what), trajectory_order(order)))

    def trajectory_info(self):
        """pucfem_trajectory_info: the three orders, the steps each part has taken while on, the rows of the last dye
        and velocity launch whose midpoint was not found, the tracers of the last launch that fell back to their
        Euler step, and the device bytes held."""
        o = (ct.c_int64 * 10)()
        self._c(self.L.pucfem_trajectory_info(self.h, o))
        return dict(dye=TRAJECTORY_NAMES[o[0] - 1], velocity=TRAJECTORY_NAMES[o[1] - 1],
                    tracers=TRAJECTORY_NAMES[o[2] - 1], dye_steps=o[3], velocity_steps=o[4], tracer_steps=o[5],
                    dye_mid_notfound=o[6], velocity_mid_notfound=o[7], tracers_fell_back=o[8], bytes=o[9])

    def trajectory_probe(self, what, scheme="sl", nch=1, iters=10):
        """Kernel times of the fused midpoint launches (pucfem_trajectory_probe; tools/trajectory_bench.py)."""
        o = (ct.c_double * 4)()
        self._c(self.L.pucfem_trajectory_probe(self.h, int(what), advection_scheme(scheme), int(nch), int(iters), o))
        return dict(pass1_ms=o[0], pass2_ms=o[1], pass1_bytes=o[2], pass2_bytes=o[3])

    def flow_info(self, member=None):
        """Flow summaries of the current u, reduced on the device (pucfem_flow_info; one launch, four doubles
        copied): max |vorticity|, the enstrophy 1/2 sum w vorticity^2, the kinetic energy 1/2 sum w |u|^2 and the
        peak speed, with w = area_sum + 1e-12 per node.  member: that member of the context's ensemble."""
        o = (ct.c_double * 4)()
        self._c(self.L.pucfem_flow_info(self.h, -1 if member is None else int(member), o))
        return dict(zip(FLOW_KEYS, (float(v) for v in o)))

    # ---------------------------------------------------------------- swimmer loads
    def surface_edges(self):
        """The swimmer surface's edge list (pucfem_host_surface_edges; works host-only): int32 arrays tri, a, b, opp
        in the caller's numbering, in ascending (triangle, local edge) order."""
        n = ct.c_int64(0)
        self._c(self.L.pucfem_host_surface_edges(self.h, ct.byref(n), None, None, None, None))
        out = [np.zeros(n.value, dtype=np.int32) for _ in range(4)]
        self._c(self.L.pucfem_host_surface_edges(self.h, ct.byref(n), *(_lib.iptr(a) for a in out)))
        return dict(zip(("tri", "a", "b", "opp"), out))

    def swimmer_loads(self, member=None):
        """Force and torque of the fluid on the swimmer, the power it delivers to the fluid and the viscous
        dissipation, reduced on the device from the current u and the last step's p + p2 (pucfem_swimmer_loads; one
        launch, ten doubles copied): the ten LOADS_KEYS values and, as their sums, force_x, force_y, torque and
        power.  member: that member of the context's ensemble."""
        o = (ct.c_double * 10)()
        self._c(self.L.pucfem_swimmer_loads(self.h, -1 if member is None else int(member), o))
        return loads_dict(np.array(o[:]))

    def surface_traction(self, member=None):
        """The per-edge parts of swimmer_loads around the body (pucfem_surface_traction): {name: (E,)} for the first
        eight LOADS_KEYS, with `theta`, the angle of the edge midpoints about the centre, and `length`."""
        E = self.surface_edges()
        out = np.zeros((len(E["tri"]), 8))
        self._c(self.L.pucfem_surface_traction(self.h, -1 if member is None else int(member), _lib.dptr(out)))
        d = {k: out[:, q].copy() for q, k in enumerate(LOADS_KEYS[:8])}
        X, c = self.coords, getattr(self, "center", (0.5, 0.5))
        mid = 0.5 * (X[E["a"]] + X[E["b"]])
        d["theta"] = np.arctan2(mid[:, 1] - c[1], mid[:, 0] - c[0])
        d["length"] = np.hypot(*(X[E["b"]] - X[E["a"]]).T)
        return d

    def loads_apply(self, u, p, edges=False):
        """The unit operation (pucfem_loads_apply): the ten values of the caller's u (N, 2) and pressure p (N), with
        edges=True also the (E, 8) per-edge values."""
        u = np.ascontiguousarray(u, dtype=np.float64)
        p = np.ascontiguousarray(p, dtype=np.float64)
        if u.shape != (self.N, 2) or p.shape != (self.N,):
            raise ValueError("u is (N, 2) and p is (N,)")
        o = np.zeros(10)
        e = np.zeros((len(self.surface_edges()["tri"]), 8)) if edges else None
        self._c(self.L.pucfem_loads_apply(self.h, _lib.dptr(u), _lib.dptr(p), _lib.dptr(o),
                                          _lib.dptr(e) if edges else None))
        return (o, e) if edges else o

    def record_loads(self, capacity):
        """Switch the loads record on (a device ring of `capacity` rows, one per step and per ensemble member) or,
        with 0, off (pucfem_set_loads_record).  Every call starts from zero rows."""
        self._c(self.L.pucfem_set_loads_record(self.h, int(capacity)))

    def loads_info(self, member=None):
        o = (ct.c_int64 * 4)()
        self._c(self.L.pucfem_loads_info(self.h, -1 if member is None else int(member), o))
        return dict(edges=o[0], triangles=o[1], recorded=o[2], capacity=o[3])

    def loads_history(self, member=None):
        """(n, 11) the rows the record holds, oldest first: the row's number since the record was set, then the ten
        LOADS_KEYS values after that step (pucfem_loads_record)."""
        i = self.loads_info(member)
        n = min(i["recorded"], i["capacity"])
        out = np.zeros((n, 11))
        self._c(self.L.pucfem_loads_record(self.h, -1 if member is None else int(member), 0, n, _lib.dptr(out)))
        return out

    def loads_probe(self, iters=10):
        """Kernel time and algorithmic bytes of the loads launch (pucfem_loads_probe; tools/loads_bench.py)."""
        o = (ct.c_double * 2)()
        self._c(self.L.pucfem_loads_probe(self.h, int(iters), o))
        return dict(ms=o[0], bytes=o[1])

    def comm_info(self):
        """Multi-rank data flow of the last step (pucfem_comm_info)."""
        o = (ct.c_int64 * 4)()
        self._c(self.L.pucfem_comm_info(self.h, o))
        return dict(dye_halo_values=o[0], allgather_values=o[1], tracer_allreduce_values=o[2],
                    backend={0: None, 1: "local", 2: "rccl"}[o[3]])

    def comm_counters(self):
        """Cumulative communicator traffic of this rank (pucfem_comm_counters)."""
        o = (ct.c_int64 * 6)()
        self._c(self.L.pucfem_comm_counters(self.h, o))
        return dict(allreduce_calls=o[0], allreduce_values=o[1], sends=o[2], send_bytes=o[3], groups=o[4],
                    broadcasts=o[5])

    def comm_selftest(self):
        """All-reduce + ring send/recv check of the context's communicator (pucfem_comm_selftest)."""
        o = (ct.c_double * 4)()
        self._c(self.L.pucfem_comm_selftest(self.h, o))
        return dict(sum_err=o[0], max_err=o[1], recv_err=o[2], backend={1: "local", 2: "rccl"}[int(o[3])])

    def timing(self, on):
        self._c(self.L.pucfem_timing_enable(self.h, int(on)))

    def timing_get(self, kclass):
        ms, n, b = ct.c_double(), ct.c_int64(), ct.c_double()
        self._c(self.L.pucfem_timing_get(self.h, kclass, ct.byref(ms), ct.byref(n), ct.byref(b)))
        return ms.value, n.value, b.value

    def counters(self):
        """(kernel launches of this thread, algorithmic bytes of the context's kernels), cumulative
        (pucfem_counters): differences over a timed region give launches and the HBM floor per step."""
        n, b = ct.c_int64(), ct.c_double()
        self._c(self.L.pucfem_counters(self.h, ct.byref(n), ct.byref(b)))
        return n.value, b.value

    def class_counters(self, kclass):
        """(launches, algorithmic bytes) of one kernel class over every launch so far (pucfem_class_counters)."""
        n, b = ct.c_int64(), ct.c_double()
        self._c(self.L.pucfem_class_counters(self.h, int(kclass), ct.byref(n), ct.byref(b)))
        return n.value, b.value

    def sync(self):
        self._c(self.L.pucfem_sync(self.h))

    def host_csr(self, op):
        """Host-assembled operator (this rank's rows, caller numbering) as scipy CSR (rows, N)."""
        import scipy.sparse as sp

        nr, nnz = ct.c_int64(), ct.c_int64()
        self._c(self.L.pucfem_host_get_csr(self.h, op, ct.byref(nr), ct.byref(nnz), None, None, None))
        rp = np.zeros(nr.value + 1, dtype=np.int64)
        col = np.zeros(nnz.value, dtype=np.int64)
        val = np.zeros(nnz.value)
        self._c(self.L.pucfem_host_get_csr(self.h, op, ct.byref(nr), ct.byref(nnz), _lib.lptr(rp), _lib.lptr(col),
                                           _lib.dptr(val)))
        return sp.csr_matrix((val, col, rp), shape=(nr.value, self.N))

    def host_partition(self, rank, world):
        no, ng, ns = ct.c_int64(), ct.c_int64(), ct.c_int64()
        self._c(self.L.pucfem_host_partition(self.h, rank, world, ct.byref(no), ct.byref(ng), None, None, None,
                                             ct.byref(ns), None, None))
        owned = np.zeros(no.value, dtype=np.int64)
        ghosts = np.zeros(ng.value, dtype=np.int64)
        gown = np.zeros(ng.value, dtype=np.int32)
        sid = np.zeros(ns.value, dtype=np.int64)
        speer = np.zeros(ns.value, dtype=np.int32)
        self._c(self.L.pucfem_host_partition(self.h, rank, world, ct.byref(no), ct.byref(ng), _lib.lptr(owned),
                                             _lib.lptr(ghosts), _lib.iptr(gown), ct.byref(ns), _lib.lptr(sid),
                                             _lib.iptr(speer)))
        return dict(owned=owned, ghosts=ghosts, ghost_owner=gown, send_ids=sid, send_peer=speer)


# ------------------------------------------------------------------------------------------------
def stokes_setup(mesh: Mesh, bc: SquirmerBC):
    """Host-side setup of StokesColor.py:441-464: filtered periodic pairs, Dirichlet list and values."""
    X = mesh.coords
    pairs = filter_wall_pairs(X, find_boundary_pairs(X, L=1.0))
    wall, inner, dirichlet, interior = boundary_sets(X, mesh.markers)
    vals_inner = squirmer_values(X, inner, bc.B1, bc.B2, bc.center)
    nodes = np.concatenate([wall, inner]).astype(np.int32)
    vals = np.concatenate([np.tile(np.asarray(bc.outer_value, dtype=np.float64), (len(wall), 1)), vals_inner])
    return pairs, nodes, vals


class StokesSimulation:
    """The StokesColor.py (scheme='color') / StokesFood.py (scheme='food') time loop on one GPU,
    or on one rank of a torch.distributed job (dist=(rank, world, unique_id))."""

    def __init__(self, mesh: Mesh, bc: SquirmerBC | None = None, dt=0.05, scheme="color", device=0,
                 tol: Tolerances | None = None, dist=None, tracers=None, nstrips=0, inertia=False, advection="sl",
                 tracer_diffusivity=0.0, tracer_seed=0, force=None, buoyancy=None, stroke=None,
                 trajectory="euler", tracer_stretch=False):
        adv = advection_scheme(advection)
        trj = trajectory_order(trajectory)
        if _stretch_flag(tracer_stretch) and scheme != "food":
            raise ValueError("tracer_stretch belongs to scheme 'food': a 'color' run has no tracers")
        _check_stroke(stroke)
        f_const, f_field = _force_args(force, mesh.N)
        if buoyancy is not None and not isinstance(buoyancy, Buoyancy):
            raise ValueError("buoyancy must be a Buoyancy or None")
        if buoyancy is not None and scheme != "color":
            raise ValueError("buoyancy belongs to scheme 'color': a 'food' run has no dye")
        # (the dye's scheme on color runs, the velocity's too on inertial ones)
        adv_what = (_lib.ADV_DYE if scheme == "color" else 0) | (_lib.ADV_VELOCITY if inertia else 0)
        if adv and not adv_what:
            raise ValueError("advection='maccormack' moves the dye of a 'color' run and the velocity of an inertial "
                             "one: a 'food' run without inertia has neither")
        # (whatever the run transports: the dye on color runs, the velocity on inertial ones, the tracers on food runs)
        trj_what = ((_lib.TRJ_DYE if scheme == "color" else 0) | (_lib.TRJ_VELOCITY if inertia else 0) |
                    (_lib.TRJ_TRACERS if scheme == "food" else 0))
        self.mesh = mesh
        self.bc = bc or SquirmerBC()
        self.dt = dt
        self.scheme = scheme
        self.ctx = Context(device, dist)
        self.ctx.upload(mesh)
        pairs, nodes, vals = stokes_setup(mesh, self.bc)
        self.pairs = pairs
        self.dirichlet_nodes = nodes
        self._stroke = None
        self.ctx.set_pairs(0, pairs)
        self.ctx.set_pairs(1, pairs)
        self.ctx.set_dirichlet(nodes, vals)
        tol = tol or Tolerances()
        if mesh.base is not None and mesh.levels > 0 and tol.precond in ("mg", "auto"):
            self.ctx.set_hierarchy(mesh.base, mesh.levels)
        self.ctx.build(scheme, dt, self.bc.nu, tol, self.bc.capture_radius, self.bc.center, nstrips)
        self.step_count = 0
        self.history = []
        if scheme == "food":
            from .tracers import tracer_init

            pts = tracer_init(self.bc.squirmer_radius, self.bc.center) if tracers is None else tracers
            pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
            self.ctx.set_field(_lib.F_TRACERS, pts)
            self.n_tracers = len(pts)
        try:
            if inertia:
                self.ctx.set_inertia(True)
            if adv:
                self.ctx.set_advection(adv_what, adv)
            if trj != _lib.TRJ_EULER:
                self.ctx.set_trajectory(trj_what, trj)
            if tracer_diffusivity != 0.0 or tracer_seed != 0:
                self.ctx.set_tracer_diffusion(tracer_diffusivity, tracer_seed)
            if tracer_stretch:
                self.ctx.set_tracer_stretch(True)
            self._force = (None, None)
            self._buoyancy = None
            if force is not None:
                self.set_force(f_const, f_field)
            if buoyancy is not None:
                self.buoyancy = buoyancy
            if stroke is not None:
                self.stroke = stroke
        except Exception:
            self.ctx.close()
            raise

    # ---- time-dependent strokes: the squirmer's boundary values per step
    @property
    def stroke(self):
        """The Stroke of the steps, or None: every step imposes the squirmer values of its table row -- v_t =
        sum_j amp[row, j] sin((j + 1) theta) along the tangent -- where a plain run holds SquirmerBC.B1 / B2 fixed.
        The walls keep their values.  Setting it does not touch u and starts the stroke's step count at 0; None
        restores the values of SquirmerBC.B1 / B2.  A stroked step is the static step of its row's amplitudes, taken
        from the same fields; a small-mesh run steps uncaptured while a stroke is set."""
        return self._stroke

    @stroke.setter
    def stroke(self, stroke):
        _check_stroke(stroke)
        if stroke is None:
            self.ctx.set_stroke(None)
        else:
            inner = boundary_sets(self.mesh.coords, self.mesh.markers)[1]
            shape, dirs = stroke_geometry(self.mesh.coords, inner, stroke.K, self.bc.center)
            self.ctx.set_stroke(stroke, inner, shape, dirs)
        self._stroke = stroke

    def stroke_info(self):
        """Context.stroke_info of this run: K (0: off), P, start, the steps taken since the stroke was set, the row
        the next step imposes, the driven nodes."""
        return self.ctx.stroke_info()

    @property
    def boundary_values(self):
        """(nodes, values): the Dirichlet nodes and the (n, 2) values the device holds for them now."""
        return self.dirichlet_nodes.copy(), self.ctx.get_dirichlet(len(self.dirichlet_nodes))

    # ---- body forces: r = base + dt * f in front of the viscous solve
    def set_force(self, constant=None, field=None):
        """The uniform force (a pair) and the nodal force field ((N, 2)) at once; None for a part that is absent.
        It takes effect at the next step."""
        if field is not None and np.shape(field) != (self.mesh.N, 2):
            raise ValueError(f"force: the nodal field must be ({self.mesh.N}, 2), got {np.shape(field)}")
        self.ctx.set_force(constant, field)
        self._force = (None if constant is None else np.array(constant, dtype=np.float64),
                       None if field is None else np.array(field, dtype=np.float64))

    @property
    def force(self):
        """The body force of the steps: a pair (uniform: a mean pressure gradient in the x-periodic channel), an (N, 2)
        nodal field, or None.  The viscous solve takes r = base + dt * f where it took base (u, or u_a with
        inertia on).  set_force gives both parts at once; the getter returns (constant, field) when both are set."""
        F, fn = self._force
        return F if fn is None else fn if F is None else (F, fn)

    @force.setter
    def force(self, force):
        self.set_force(*_force_args(force, self.mesh.N))

    @property
    def buoyancy(self):
        """The Buoyancy of the dye (scheme 'color'), or None: f = g * sum_t beta_t * (s_t - ref_t) on top of the
        force, read from the dye at the start of each step.  Such steps wait for the previous step's dye in front
        of the viscous solve instead of overlapping it.  Removing or redefining the dye channels while a term names
        one switches it off."""
        return self._buoyancy if self.ctx.force_info()["buoyancy"] else None

    @buoyancy.setter
    def buoyancy(self, b):
        if b is None and self.scheme != "color":  # (a 'food' run has none to switch off)
            return
        self.ctx.set_buoyancy(b)
        self._buoyancy = b

    @property
    def force_field(self):
        """(N, 2) the total force f of the current state (PUCFEM_F_FORCE), formed on the device when read."""
        return self.ctx.get_field(_lib.F_FORCE, (self.mesh.N, 2))

    @property
    def u_rhs(self):
        """(N, 2) the r of the last forced step (PUCFEM_F_U_RHS): what its viscous solve took as right-hand side."""
        return self.ctx.get_field(_lib.F_U_RHS, (self.mesh.N, 2))

    def force_info(self):
        """Context.force_info of this run."""
        return self.ctx.force_info()

    @property
    def tracer_diffusivity(self):
        """The tracers' diffusivity D (Brownian food): with D > 0 every free tracer takes, per step, a random-walk
        increment uniform on [-a, a], a = sqrt(6 D dt), on top of its move (variance 2 D dt per coordinate), is
        reflected at the walls and, once eaten, stays where it was absorbed.  0 (the default): the reference's
        deterministic tracers.  Setting it takes effect at the next step."""
        return self.ctx.tracer_diffusion()[0]

    @tracer_diffusivity.setter
    def tracer_diffusivity(self, D):
        self.ctx.set_tracer_diffusion(D, self.ctx.tracer_diffusion()[1])

    @property
    def tracer_seed(self):
        """The 64-bit seed of the tracers' random walk: the increments depend on (seed, tracer, tracer step) alone."""
        return self.ctx.tracer_diffusion()[1]

    @tracer_seed.setter
    def tracer_seed(self, seed):
        self.ctx.set_tracer_diffusion(self.ctx.tracer_diffusion()[0], seed)

    def step(self, n=1):
        st = self.ctx.step(n)
        self.step_count += n
        self.history.extend(st)
        return st

    @property
    def u(self):
        return self.ctx.get_field(_lib.F_U, (self.mesh.N, 2))

    @u.setter
    def u(self, v):
        self.ctx.set_field(_lib.F_U, v)

    @property
    def c(self):
        return self.ctx.get_field(_lib.F_C, (self.mesh.N,))

    @c.setter
    def c(self, v):
        self.ctx.set_field(_lib.F_C, v)

    def field(self, f, ncomp=1):
        return self.ctx.get_field(f, (self.mesh.N, ncomp) if ncomp > 1 else (self.mesh.N,))

    @property
    def dyes(self):
        """(K, N) the dye channels: extra dye fields advected beside c with every step's final u, the departure
        point and its triangle found once per node for all of them.  Channel k holds the bits c would hold in a run
        started from c = channel k.  Setting them (K = 0 .. 16 rows; dye_patterns gives the reference's three starts)
        resets the channel step count; an empty array removes them."""
        K = self.ctx.dyes_info()["channels"]
        return self.ctx.get_field(_lib.F_DYES, (K, self.mesh.N))

    @dyes.setter
    def dyes(self, v):
        a = np.ascontiguousarray(v, dtype=np.float64)
        if a.size and (a.ndim != 2 or a.shape[1] != self.mesh.N):
            raise ValueError(f"dyes must have shape (K, {self.mesh.N})")
        if a.size == 0:
            self.ctx._c(self.ctx.L.pucfem_set_field(self.ctx.h, _lib.F_DYES, None, 0))
        else:
            self.ctx.set_field(_lib.F_DYES, a)

    @property
    def inertia(self):
        """Whether the steps carry the inertial term: u_a = SL(u; u, dt), each velocity component advected by the
        semi-Lagrangian scheme of the dye, in front of the viscous solve (finite Reynolds number; off: the
        reference's Stokes step).  Setting it takes effect at the next step."""
        return self.ctx.inertia_info()["on"]

    @inertia.setter
    def inertia(self, on):
        self.ctx.set_inertia(bool(on))

    @property
    def u_advected(self):
        """(N, 2) the u_a of the last inertial step (PUCFEM_F_U_ADV): what its viscous solve took as right-hand side."""
        return self.ctx.get_field(_lib.F_U_ADV, (self.mesh.N, 2))

    def inertia_info(self):
        """Context.inertia_info of this run as (on, steps, notfound, bytes)."""
        d = self.ctx.inertia_info()
        return d["on"], d["steps"], d["notfound"], d["bytes"]

    @property
    def dye_advection(self):
        """'sl' or 'maccormack': how every step moves c and the dye channels -- the reference's first-order
        semi-Lagrangian step, or two of them and a clamp (Selle et al.'s limited MacCormack scheme, second order; not
        conservative).  Setting it takes effect at the next step."""
        return self.ctx.advection_info()["dye"]

    @dye_advection.setter
    def dye_advection(self, scheme):
        self.ctx.set_advection(_lib.ADV_DYE, scheme)

    @property
    def velocity_advection(self):
        """'sl' or 'maccormack': how an inertial step forms u_a from u.  It may be set while inertia is off and takes
        effect when inertia is on."""
        return self.ctx.advection_info()["velocity"]

    @velocity_advection.setter
    def velocity_advection(self, scheme):
        self.ctx.set_advection(_lib.ADV_VELOCITY, scheme)

    def advection_info(self):
        """Context.advection_info of this run."""
        return self.ctx.advection_info()

    # ---- midpoint trajectories (pucfem_set_trajectory)
    @property
    def dye_trajectory(self):
        """'euler' | 'midpoint': the path the dye and its channels are traced back along.  'midpoint' reads the
        velocity again half a step along the straight trace and takes the whole step with it (second order along a
        steady flow); 'euler' is the reference's step."""
        return self.ctx.trajectory_info()["dye"]

    @dye_trajectory.setter
    def dye_trajectory(self, order):
        self.ctx.set_trajectory(_lib.TRJ_DYE, order)

    @property
    def velocity_trajectory(self):
        """... of the inertial step's velocity (it may be set while inertia is off and waits for it)."""
        return self.ctx.trajectory_info()["velocity"]

    @velocity_trajectory.setter
    def velocity_trajectory(self, order):
        self.ctx.set_trajectory(_lib.TRJ_VELOCITY, order)

    @property
    def tracer_trajectory(self):
        """... of the tracers of a 'food' run: the move is taken with the velocity at the midpoint of the Euler
        step; a tracer whose midpoint leaves the mesh takes its Euler step (trajectory_info counts them)."""
        return self.ctx.trajectory_info()["tracers"]

    @tracer_trajectory.setter
    def tracer_trajectory(self, order):
        self.ctx.set_trajectory(_lib.TRJ_TRACERS, order)

    def trajectory_info(self):
        """Context.trajectory_info of this run."""
        return self.ctx.trajectory_info()

    def dye_mixing(self):
        """(K, 3): mixing_index (StokesColor.py:391-403) (I, mu, var) of every dye channel over marker == 0, reduced
        on the device when called."""
        return self.ctx.dyes_mixing()

    def dyes_info(self):
        """Context.dyes_info of this run as (channels, steps, notfound, bytes)."""
        d = self.ctx.dyes_info()
        return d["channels"], d["steps"], d["notfound"], d["bytes"]

    @property
    def vorticity(self):
        """(N,) calculate_vorticity (scripts/good_visualization2.py:310-345) of the current u, formed on the device
        when read."""
        return self.ctx.get_field(_lib.F_VORTICITY, (self.mesh.N,))

    def flow_info(self):
        """Context.flow_info of this run."""
        return self.ctx.flow_info()

    def swimmer_loads(self):
        """Context.swimmer_loads of this run: the force and torque on the swimmer, its power and the dissipation."""
        return self.ctx.swimmer_loads()

    def surface_traction(self):
        """Context.surface_traction of this run: the per-edge pressure and viscous parts around the body."""
        return self.ctx.surface_traction()

    def record_loads(self, capacity):
        """Context.record_loads: every later step appends its loads to a device ring of `capacity` rows (0: off)."""
        self.ctx.record_loads(capacity)

    def loads_history(self):
        """Context.loads_history of this run: (n, 11), the rows held, oldest first."""
        return self.ctx.loads_history()

    def loads_info(self):
        return self.ctx.loads_info()

    def sample(self, points, fields=("u", "c")):
        """The fields at arbitrary points (Context.sample): ({field: values}, triangle ids)."""
        return self.ctx.sample(fields, points)

    def raster(self, width, height, fields=("c", "u"), window=None):
        """The fields as images (Context.raster): {name: float32 (height, width) or (2, height, width)}."""
        return self.ctx.raster(fields, width, height, window)

    def streamlines(self, seeds, h, nsteps, unit=True, order=2, both=False, vmin=0.0, fields=()):
        """Streamlines of the current velocity (Context.streamlines): points (lines, nsteps + 1, 2), status, npts and
        values[name] (lines, nsteps + 1) or (lines, nsteps + 1, 2)."""
        return self.ctx.streamlines(seeds, h, nsteps, unit, order, both, vmin, fields)

    @property
    def tracers(self):
        n = self._ntr()
        return self.ctx.get_field(_lib.F_TRACERS, (n, 2))

    @tracers.setter
    def tracers(self, v):
        """A new tracer set, of any size: status 0, no capture steps, step count 0."""
        if self.scheme != "food":
            raise ValueError("tracers belong to scheme 'food'")
        pts = np.asarray(v, dtype=np.float64).reshape(-1, 2)
        self.ctx.set_field(_lib.F_TRACERS, pts)
        self.n_tracers = len(pts)

    @property
    def tracer_status(self):
        return self.ctx.get_field(_lib.F_STATUS, (self._ntr(),)).astype(np.int64)

    @tracer_status.setter
    def tracer_status(self, v):
        self.ctx.set_field(_lib.F_STATUS, np.asarray(v, dtype=np.float64))

    @property
    def capture_step(self):
        """Per tracer, the 1-based tracer step (since the tracers were set) in which it was eaten; -1: never."""
        return self.ctx.get_field(_lib.F_CAPTURE_STEP, (self._ntr(),)).astype(np.int64)

    def tracer_info(self):
        return self.ctx.tracer_info()

    # ---- tracer stretching (pucfem_set_tracer_stretch)
    @property
    def tracer_stretch(self):
        """Whether the tracers carry the deformation gradient F = dPhi/dX of the flow map along their paths: the
        exact Jacobian of the discrete tracer steps (Euler or midpoint), updated in the tracer launch itself.  It only
        reads the path: positions, status and capture steps are those of the run without it.  Switching it on starts
        F at the identity, switching it off frees it; setting the tracers resets it."""
        return self.ctx.stretch_info()["on"]

    @tracer_stretch.setter
    def tracer_stretch(self, on):
        self.ctx.set_tracer_stretch(on)

    @property
    def deformation_gradient(self):
        """(n, 2, 2) the tracers' F (PUCFEM_F_DEFGRAD); NaN for a tracer that left the mesh.  Setting it resumes a
        run.  tracers.stretch / tracers.ftle turn it into stretching factors and Lyapunov exponents."""
        return self.ctx.get_field(_lib.F_DEFGRAD, (self._ntr(), 2, 2))

    @deformation_gradient.setter
    def deformation_gradient(self, F):
        F = np.ascontiguousarray(F, dtype=np.float64)
        if F.shape != (self._ntr(), 2, 2):
            raise ValueError(f"deformation_gradient must be ({self._ntr()}, 2, 2), got {F.shape}")
        self.ctx.set_field(_lib.F_DEFGRAD, F)

    def stretch_info(self, T=None):
        """Context.stretch_info of this run; T: the elapsed time of the stretch steps, for ftle_mean and ftle_max."""
        return self.ctx.stretch_info(T=T)

    def _ntr(self):
        return getattr(self, "n_tracers", 0)

    def close(self):
        self.ctx.close()


_SHARED_BC_FIELDS = ("nu", "center", "capture_radius", "squirmer_radius")


def _check_ensemble_bcs(bcs):
    bcs = list(bcs)
    if not bcs:
        raise ValueError("an ensemble needs at least one SquirmerBC")
    for f in _SHARED_BC_FIELDS:
        vals = [tuple(getattr(b, f)) if f == "center" else getattr(b, f) for b in bcs]
        if any(v != vals[0] for v in vals):
            raise ValueError(f"ensemble members share the fluid and the swimmer's geometry: {f} differs ({vals})")
    return bcs


def _ensemble_flags(inertia, M):
    """The inertia= argument of an ensemble of M members as an (M,) bool array: one bool for all, or M of them."""
    a = np.asarray(inertia)
    if a.ndim == 0:
        return np.full(M, bool(a))
    if a.shape != (M,):
        raise ValueError(f"inertia must be a bool or one bool per member: {M} members, got shape {a.shape}")
    return a.astype(bool)


def _ensemble_stretch(tracer_stretch, M):
    """The tracer_stretch= argument of an ensemble of M members as an (M,) bool array: one bool for all members or
    one per member."""
    if isinstance(tracer_stretch, (bool, np.bool_)):
        return np.full(M, bool(tracer_stretch))
    if isinstance(tracer_stretch, (str, bytes)) or not hasattr(tracer_stretch, "__len__"):
        raise ValueError(f"tracer_stretch must be True, False or one of them per member, got {tracer_stretch!r}")
    flags = list(tracer_stretch)
    if len(flags) != M:
        raise ValueError(f"tracer_stretch must be one flag or one per member: {M} members, got {len(flags)}")
    return np.array([_stretch_flag(v) for v in flags], dtype=bool)


def _ensemble_diffusion(tracer_diffusivity, tracer_seed, M):
    """The tracer_diffusivity= and tracer_seed= arguments of an ensemble of M members as an (M,) float64 and an (M,)
    uint64 array: one value for all, or M of them."""
    d = np.asarray(tracer_diffusivity, dtype=np.float64)
    if d.ndim != 0 and d.shape != (M,):
        raise ValueError(f"tracer_diffusivity must be one value or one per member: {M} members, got shape {d.shape}")
    s = np.asarray(tracer_seed, dtype=object)  # (Python ints: all 64 bits)
    if s.ndim != 0 and s.shape != (M,):
        raise ValueError(f"tracer_seed must be one value or one per member: {M} members, got shape {s.shape}")
    seeds = np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in np.broadcast_to(s, (M,)).tolist()], dtype=np.uint64)
    return np.broadcast_to(d, (M,)).copy(), seeds


def _ensemble_strokes(stroke, M):
    """The stroke= argument of an ensemble of M members checked: None, one Stroke for all, or M entries each a Stroke
    or None, all of one K."""
    if stroke is None or isinstance(stroke, Stroke):
        return
    if not isinstance(stroke, (list, tuple)):
        raise ValueError("stroke must be a Stroke, None, or a list with one Stroke or None per member")
    if len(stroke) != M:
        raise ValueError(f"stroke: one entry per member: {M} members, got {len(stroke)}")
    for s in stroke:
        _check_stroke(s)
    if len({s.K for s in stroke if s is not None}) > 1:
        raise ValueError("stroke: the strokes of an ensemble have one number of modes K (the shapes are shared)")


def _ensemble_advection(advection):
    """The advection= keyword of ensembles takes 'sl' alone: members carry a dye scheme and a velocity scheme each."""
    if advection_scheme(advection) != 0:
        raise ValueError("ensembles take dye_advection= and velocity_advection= (one name for all members or one per "
                         "member), not advection='maccormack': that keyword belongs to StokesSimulation / solve (one "
                         "squirmer per context)")


def _ensemble_schemes(scheme, M, name):
    """The dye_advection= / velocity_advection= argument of an ensemble of M members as an (M,) array of
    PUCFEM_ADV_* values: one name for all, or M of them."""
    if isinstance(scheme, (str, int, np.integer)):
        return np.full(M, advection_scheme(scheme), dtype=np.int32)
    names = list(scheme)
    if len(names) != M:
        raise ValueError(f"{name} must be one name or one per member: {M} members, got {len(names)}")
    return np.array([advection_scheme(v) for v in names], dtype=np.int32)


def _ensemble_orders(order, M, name):
    """The dye_trajectory= / velocity_trajectory= / tracer_trajectory= argument of an ensemble of M members as an (M,)
    array of PUCFEM_TRJ_* values: one name for all, or M of them."""
    if isinstance(order, (str, int, np.integer)):
        return np.full(M, trajectory_order(order), dtype=np.int32)
    names = list(order)
    if len(names) != M:
        raise ValueError(f"{name} must be one name or one per member: {M} members, got {len(names)}")
    return np.array([trajectory_order(v) for v in names], dtype=np.int32)


def _ensemble_trajectories(scheme, flags, trajectory, dye, velocity, tracers):
    """The trajectory keywords of an ensemble as three (M,) arrays of PUCFEM_TRJ_* values (dye, velocity, tracers).
    trajectory= is StokesSimulation's rule per member: the dye on 'color', the tracers on 'food', the velocity for the
    members whose inertia flag is on; a per-part keyword, where given, wins for that part."""
    M = len(flags)
    euler = np.full(M, _lib.TRJ_EULER, dtype=np.int32)
    if not isinstance(trajectory, (str, int, np.integer)):
        raise ValueError("trajectory is one name for the ensemble: use dye_trajectory=, velocity_trajectory= and "
                         "tracer_trajectory= for one per member")
    trj = np.full(M, trajectory_order(trajectory), dtype=np.int32)
    d = _ensemble_orders(dye, M, "dye_trajectory") if dye is not None else (trj if scheme == "color" else euler)
    v = (_ensemble_orders(velocity, M, "velocity_trajectory") if velocity is not None
         else np.where(flags, trj, euler).astype(np.int32))
    t = _ensemble_orders(tracers, M, "tracer_trajectory") if tracers is not None else (trj if scheme == "food" else euler)
    if dye is not None and (d != _lib.TRJ_EULER).any() and scheme != "color":
        raise ValueError("dye_trajectory='midpoint' belongs to scheme 'color': a 'food' run has no dye")
    if tracers is not None and (t != _lib.TRJ_EULER).any() and scheme != "food":
        raise ValueError("tracer_trajectory='midpoint' belongs to scheme 'food': a 'color' run has no tracers")
    return d, v, t


def _ensemble_dyes(dyes, M, N):
    """The dyes= argument of an ensemble of M members on N nodes as an (M, K, N) float64 array, K = 0 .. 16: (K, N)
    channels for all members, or (M, K, N) with each member's own; None or an empty array means no channels
    ((M, 0, N))."""
    a = np.zeros((0, N)) if dyes is None else np.asarray(dyes, dtype=np.float64)
    if a.size == 0:
        return np.zeros((M, 0, N))
    if a.ndim == 2:
        if a.shape[1] != N:
            raise ValueError(f"dyes must have shape (K, {N}) or ({M}, K, {N}): got {a.shape}")
        a = np.broadcast_to(a, (M,) + a.shape)
    elif a.ndim != 3 or a.shape[0] != M or a.shape[2] != N:
        raise ValueError(f"dyes must have shape (K, {N}) or ({M}, K, {N}): got {a.shape}")
    if a.shape[1] > _lib.MAX_DYES:
        raise ValueError(f"at most {_lib.MAX_DYES} dye channels: got {a.shape[1]}")
    return np.ascontiguousarray(a)


def ensemble_dirichlet_values(mesh: Mesh, bcs):
    """Dirichlet nodes and per-member values (M, n_dir, 2) of an ensemble: row m is stokes_setup(mesh, bcs[m])'s
    values (the wall values, then the squirmer surface values of makeDirBCU, StokesColor.py:405-427).  Host only."""
    bcs = _check_ensemble_bcs(bcs)
    nodes = None
    vals = []
    for bc in bcs:
        _, n, v = stokes_setup(mesh, bc)
        if nodes is None:
            nodes = n
        elif not np.array_equal(nodes, n):
            raise ValueError("ensemble members must share the Dirichlet node list")
        vals.append(v)
    return nodes, np.ascontiguousarray(np.stack(vals, 0), dtype=np.float64)


class StokesEnsemble:
    """M squirmers on one mesh and fluid, stepped together on one GPU context (pucfem_ens_*): the reference's
    experiment (README.md:43-45: the neutral, pusher and puller squirmer on mesh.1) or a B1 / B2 sweep in one
    launch chain.  Members share nu, dt, the mesh and the swimmer's geometry and differ in their boundary values,
    fields and tracers; each member's fields are bit-identical to a StokesSimulation with its SquirmerBC.
    Small meshes only (the dense path: N <= 1500), scheme 'color' (semi-Lagrangian dye) or 'food'.
    inertia: a bool for all members or one bool per member -- a member with it on steps as
    StokesSimulation(..., inertia=True) does, bit for bit (finite Reynolds number); the others step as before.
    force: one pair (a tuple or array) or (N, 2) field for all members, or a list with one entry per member, each a
    pair, an (N, 2) field or None; buoyancy: one (g, beta, ref) for all members or a list of them (None: off) -- a
    forced member steps as StokesSimulation(..., force=, buoyancy=Buoyancy(g, {"c": (beta, ref)})) does, bit for
    bit (set_force, set_buoyancy).
    dye_advection, velocity_advection: 'sl' or 'maccormack', one name for all members or one per member -- a member
    whose dye scheme is 'maccormack' moves its c as StokesSimulation(..., advection="maccormack") does, one whose
    velocity scheme is forms its u_a that way while its inertia is on, bit for bit (set_advection).
    dye_trajectory, velocity_trajectory, tracer_trajectory: 'euler' or 'midpoint', one name for all members or one per
    member -- a member with a part on moves its c, its u_a (while its inertia is on) or its tracers along midpoint
    traces as StokesSimulation(...) with that part on does, bit for bit (set_trajectory).  trajectory= is
    StokesSimulation's keyword applied per member: the dye on 'color', the tracers on 'food', the velocity of the
    members whose inertia flag is on; a per-part keyword, where given, wins over it for that part.
    dyes (scheme 'color'): (K, N) dye channels for all members or (M, K, N), K = 0 .. 16 -- every member's channels
    move beside its c along the path of its c, as StokesSimulation.dyes do, bit for bit (dyes, set_dyes, dye_mixing,
    dyes_info)."""

    def __init__(self, mesh: Mesh, bcs, dt=0.05, scheme="color", device=0, tol: Tolerances | None = None,
                 tracers=None, inertia=False, advection="sl", tracer_diffusivity=0.0, tracer_seed=0, force=None,
                 buoyancy=None, dye_advection="sl", velocity_advection="sl", stroke=None, dye_trajectory=None,
                 velocity_trajectory=None, tracer_trajectory=None, trajectory="euler", dyes=None,
                 tracer_stretch=False):
        _ensemble_advection(advection)
        stretch = _ensemble_stretch(tracer_stretch, len(_check_ensemble_bcs(bcs)))
        if stretch.any() and scheme != "food":
            raise ValueError("tracer_stretch belongs to scheme 'food': a 'color' run has no tracers")
        if buoyancy is not None and scheme != "color":
            raise ValueError("buoyancy belongs to scheme 'color': a 'food' run has no dye")
        self.bcs = _check_ensemble_bcs(bcs)
        dyes = _ensemble_dyes(dyes, len(self.bcs), mesh.N)
        if dyes.shape[1] and scheme != "color":
            raise ValueError("dyes belong to scheme 'color': a 'food' run has no dye")
        _ensemble_strokes(stroke, len(self.bcs))
        if scheme not in ("color", "food"):
            raise ValueError("ensembles step the Stokes schemes 'color' and 'food'")
        flags = _ensemble_flags(inertia, len(self.bcs))
        adv_dye = _ensemble_schemes(dye_advection, len(self.bcs), "dye_advection")
        adv_vel = _ensemble_schemes(velocity_advection, len(self.bcs), "velocity_advection")
        if adv_dye.any() and scheme != "color":
            raise ValueError("dye_advection='maccormack' belongs to scheme 'color': a 'food' run has no dye")
        trj_dye, trj_vel, trj_trc = _ensemble_trajectories(scheme, flags, trajectory, dye_trajectory,
                                                           velocity_trajectory, tracer_trajectory)
        diff, seeds = _ensemble_diffusion(tracer_diffusivity, tracer_seed, len(self.bcs))
        nodes, vals = ensemble_dirichlet_values(mesh, self.bcs)
        self.mesh = mesh
        self.dt = dt
        self.scheme = scheme
        self.M = len(self.bcs)
        bc0 = self.bcs[0]
        self.ctx = Context(device)
        try:
            self.ctx.upload(mesh)
            pairs, _, _ = stokes_setup(mesh, bc0)
            self.ctx.set_pairs(0, pairs)
            self.ctx.set_pairs(1, pairs)
            self.ctx.set_dirichlet(nodes, vals[0])
            self.ctx.build(scheme, dt, bc0.nu, tol or Tolerances(), bc0.capture_radius, bc0.center, 0)
            self.n_tracers = 0
            if scheme == "food":
                from .tracers import tracer_init

                pts = tracer_init(bc0.squirmer_radius, bc0.center) if tracers is None else tracers
                pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
                self.ctx.set_field(_lib.F_TRACERS, pts)
                self.n_tracers = len(pts)
            self.ctx._c(self.ctx.L.pucfem_ens_create(self.ctx.h, self.M, _lib.dptr(vals)))
            if flags.any():
                self.inertia = flags
            if adv_dye.any():
                self.dye_advection = adv_dye
            if adv_vel.any():
                self.velocity_advection = adv_vel
            if (trj_dye != _lib.TRJ_EULER).any():
                self.dye_trajectory = trj_dye
            if (trj_vel != _lib.TRJ_EULER).any():
                self.velocity_trajectory = trj_vel
            if (trj_trc != _lib.TRJ_EULER).any():
                self.tracer_trajectory = trj_trc
            if diff.any() or seeds.any():
                self.set_tracer_diffusion(diff, seeds)
            if stretch.any():
                self.tracer_stretch = stretch
            if force is not None:
                self.set_force(force)
            if buoyancy is not None:
                self.set_buoyancy(buoyancy)
            if stroke is not None:
                self.set_stroke(stroke)
            if dyes.shape[1]:
                self.dyes = dyes
        except Exception:
            self.ctx.close()
            raise
        self.step_count = 0
        self.history = []

    # ---- fields (member = None: all members, leading axis M)
    def _shape(self, f, ncomp=1):
        if f == _lib.F_TRACERS:
            return (self.n_tracers, 2)
        if f in (_lib.F_STATUS, _lib.F_CAPTURE_STEP):
            return (self.n_tracers,)
        if f == _lib.F_DEFGRAD:
            return (self.n_tracers, 2, 2)
        return (self.mesh.N, ncomp) if ncomp > 1 else (self.mesh.N,)

    def get(self, f, ncomp=1, member=None):
        shape = self._shape(f, ncomp)
        out = np.zeros(shape if member is not None else (self.M,) + shape)
        self.ctx._c(self.ctx.L.pucfem_ens_get_field(self.ctx.h, f, -1 if member is None else int(member),
                                                    _lib.dptr(out), out.size))
        return out

    def set(self, f, a, member=None):
        a = np.ascontiguousarray(a, dtype=np.float64)
        self.ctx._c(self.ctx.L.pucfem_ens_set_field(self.ctx.h, f, -1 if member is None else int(member),
                                                    _lib.dptr(a), a.size))

    def field(self, f, ncomp=1):
        return self.get(f, ncomp)

    @property
    def u(self):
        return self.get(_lib.F_U, 2)

    @u.setter
    def u(self, v):
        self.set(_lib.F_U, v)

    @property
    def c(self):
        return self.get(_lib.F_C)

    @c.setter
    def c(self, v):
        self.set(_lib.F_C, v)

    # ---- dye channels per member (pucfem_ens_set_dyes)
    def dyes_info(self, member=None):
        """pucfem_ens_dyes_info per member, with Context.dyes_info's keys: the number of channels, the channel steps
        since the member's channels were last set, the not-found rows of its last dye launch and the device bytes the
        ensemble holds for channels -- one member's dict, or (member=None) a dict of (M,) arrays."""
        def one(m):
            o = (ct.c_int64 * 4)()
            self.ctx._c(self.ctx.L.pucfem_ens_dyes_info(self.ctx.h, int(m), o))
            return dict(channels=int(o[0]), steps=int(o[1]), notfound=int(o[2]), bytes=int(o[3]))

        if member is not None:
            return one(member)
        rows = [one(m) for m in range(self.M)]
        return {k: np.array([r[k] for r in rows]) for k in ("channels", "steps", "notfound", "bytes")}

    @property
    def dyes(self):
        """(M, K, N) every member's dye channels: K extra dye fields per member, the same K for all, advected beside
        the member's c with every step's final u along the path of its c (its dye scheme and trajectory), the
        departure point and its triangle found once per pass and row for c and all of them.  Channel k of member m
        holds the bits of channel k of a StokesSimulation with the member's boundary values, settings and starting
        channels.  Setting them takes (K, N) for all members or (M, K, N) and resets the channel step counts; an empty
        array removes them."""
        K = self.dyes_info(0)["channels"]
        out = np.zeros((self.M, K, self.mesh.N))
        if K:
            self.ctx._c(self.ctx.L.pucfem_ens_get_field(self.ctx.h, _lib.F_DYES, -1, _lib.dptr(out), out.size))
        return out

    @dyes.setter
    def dyes(self, v):
        a = _ensemble_dyes(v, self.M, self.mesh.N)
        K = a.shape[1]
        if K == 0:
            self.ctx._c(self.ctx.L.pucfem_ens_set_dyes(self.ctx.h, 0, None))
            return
        # (defines K from member 0's channels; then every member's own where they differ)
        self.ctx._c(self.ctx.L.pucfem_ens_set_dyes(self.ctx.h, K, _lib.dptr(np.ascontiguousarray(a[0]))))
        if (a != a[0]).any():
            self.set(_lib.F_DYES, a)

    def set_dyes(self, a, member):
        """One member's channels, (K, N) with the ensemble's K (pucfem_ens_set_field, PUCFEM_F_DYES): its channel step
        count starts again, the other members keep theirs."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != self.mesh.N:
            raise ValueError(f"a member's dyes must have shape (K, {self.mesh.N})")
        self.set(_lib.F_DYES, a, int(member))

    def dye_mixing(self, member=None):
        """(M, K, 3), or (K, 3) of one member: (I, mu, var) of every dye channel over marker == 0
        (pucfem_ens_dyes_mixing), row for row StokesSimulation.dye_mixing of the member's single run."""
        K = self.dyes_info(0)["channels"]
        out = np.zeros((self.M, K, 3) if member is None else (K, 3))
        self.ctx._c(self.ctx.L.pucfem_ens_dyes_mixing(self.ctx.h, -1 if member is None else int(member),
                                                      _lib.dptr(out)))
        return out

    @property
    def vorticity(self):
        """(M, N): every member's vorticity, formed on the device when read."""
        return self.get(_lib.F_VORTICITY)

    # ---- inertia per member (pucfem_ens_set_inertia)
    def set_inertia(self, on, member=None):
        """Switch the inertial term of one member (or, member=None, of all) on or off; it takes effect at the next
        step.  Switching a member on starts its counts (inertia_info) again."""
        self.ctx._c(self.ctx.L.pucfem_ens_set_inertia(self.ctx.h, -1 if member is None else int(member),
                                                      1 if on else 0))

    def inertia_info(self, member=None):
        """pucfem_ens_inertia_info: on, the inertial steps since the member was switched on, the not-found rows of its
        last inertial launch and the device bytes the ensemble holds for inertia -- one member's dict, or
        (member=None) a dict of (M,) arrays."""
        def one(m):
            o = (ct.c_int64 * 4)()
            self.ctx._c(self.ctx.L.pucfem_ens_inertia_info(self.ctx.h, int(m), o))
            return dict(on=bool(o[0]), steps=int(o[1]), notfound=int(o[2]), bytes=int(o[3]))

        if member is not None:
            return one(member)
        rows = [one(m) for m in range(self.M)]
        return {k: np.array([r[k] for r in rows]) for k in ("on", "steps", "notfound", "bytes")}

    @property
    def inertia(self):
        """(M,) bool: which members carry the inertial term u_a = SL(u; u, dt) in front of the viscous product
        (StokesSimulation.inertia per member).  Set it with one bool for all or one per member."""
        return self.inertia_info()["on"]

    @inertia.setter
    def inertia(self, on):
        flags = _ensemble_flags(on, self.M)
        if flags.all() or not flags.any():
            self.set_inertia(bool(flags[0]))
        else:
            for m, f in enumerate(flags):
                self.set_inertia(bool(f), m)

    # ---- MacCormack advection per member (pucfem_ens_set_advection)
    def set_advection(self, what, scheme, member=None):
        """The advection scheme of one member (or, member=None, of all): of its dye (what = ADV_DYE), of its inertial
        step's velocity (ADV_VELOCITY) or of both (their sum); 'sl' or 'maccormack'.  It takes effect at the next
        step (the velocity's while the member's inertia is on); switching a scheme on starts the member's counts
        (advection_info) again."""
        self.ctx._c(self.ctx.L.pucfem_ens_set_advection(self.ctx.h, -1 if member is None else int(member), int(what),
                                                        advection_scheme(scheme)))

    def advection_info(self, member=None):
        """pucfem_ens_advection_info, with Context.advection_info's keys: the member's two schemes, the MacCormack
        steps since each was switched on, the counts of its last launch of each (rows without T1, rows without T2,
        clamped values) and the device bytes the ensemble holds for MacCormack -- one member's dict, or
        (member=None) a dict of (M,) arrays ((M, 3) for the counts)."""
        def one(m):
            o = (ct.c_int64 * 11)()
            self.ctx._c(self.ctx.L.pucfem_ens_advection_info(self.ctx.h, int(m), o))
            return dict(dye=ADVECTION_NAMES[o[0]], velocity=ADVECTION_NAMES[o[1]], dye_steps=o[2],
                        velocity_steps=o[3], dye_counts=(o[4], o[5], o[6]), velocity_counts=(o[7], o[8], o[9]),
                        bytes=o[10])

        if member is not None:
            return one(member)
        rows = [one(m) for m in range(self.M)]
        return {k: np.array([r[k] for r in rows]) for k in rows[0]}

    def _set_schemes(self, what, scheme, name):
        v = _ensemble_schemes(scheme, self.M, name)
        if (v == v[0]).all():
            self.set_advection(what, int(v[0]))
        else:
            for m, k in enumerate(v):
                self.set_advection(what, int(k), m)

    @property
    def dye_advection(self):
        """One name per member, 'sl' or 'maccormack': how each member's step moves its c
        (StokesSimulation.dye_advection per member).  Set it with one name for all or one per member."""
        return list(self.advection_info()["dye"])

    @dye_advection.setter
    def dye_advection(self, scheme):
        self._set_schemes(_lib.ADV_DYE, scheme, "dye_advection")

    @property
    def velocity_advection(self):
        """One name per member: how each member's inertial step forms u_a from u.  It may be set while the member's
        inertia is off and takes effect when it is on."""
        return list(self.advection_info()["velocity"])

    @velocity_advection.setter
    def velocity_advection(self, scheme):
        self._set_schemes(_lib.ADV_VELOCITY, scheme, "velocity_advection")

    # ---- midpoint trajectories per member (pucfem_ens_set_trajectory)
    def set_trajectory(self, what, order, member=None):
        """The trajectory order of one member (or, member=None, of all): of its dye (what = TRJ_DYE), of its inertial
        step's velocity (TRJ_VELOCITY), of its tracers (TRJ_TRACERS) or of several (their sum); 'euler' or 'midpoint'.
        It takes effect at the next step (the velocity's while the member's inertia is on); switching a part on starts
        the member's counts (trajectory_info) again."""
        self.ctx._c(self.ctx.L.pucfem_ens_set_trajectory(self.ctx.h, -1 if member is None else int(member), int(what),
                                                         trajectory_order(order)))

    def trajectory_info(self, member=None):
        """pucfem_ens_trajectory_info, with Context.trajectory_info's keys: the member's three orders, the steps each
        part has taken while on, the rows of its last dye and velocity launch whose midpoint was not found, the tracers
        of its last launch that fell back to their Euler step and the device bytes the ensemble holds for
        trajectories -- one member's dict, or (member=None) a list of them, one per member."""
        def one(m):
            o = (ct.c_int64 * 10)()
            self.ctx._c(self.ctx.L.pucfem_ens_trajectory_info(self.ctx.h, int(m), o))
            return dict(dye=TRAJECTORY_NAMES[o[0] - 1], velocity=TRAJECTORY_NAMES[o[1] - 1],
                        tracers=TRAJECTORY_NAMES[o[2] - 1], dye_steps=o[3], velocity_steps=o[4], tracer_steps=o[5],
                        dye_mid_notfound=o[6], velocity_mid_notfound=o[7], tracers_fell_back=o[8], bytes=o[9])

        if member is not None:
            return one(member)
        return [one(m) for m in range(self.M)]

    def _set_orders(self, what, order, name):
        v = _ensemble_orders(order, self.M, name)
        if (v == v[0]).all():
            self.set_trajectory(what, int(v[0]))
        else:
            for m, k in enumerate(v):
                self.set_trajectory(what, int(k), m)

    def _orders(self, key):
        return np.array([r[key] for r in self.trajectory_info()])

    @property
    def dye_trajectory(self):
        """(M,) names, 'euler' or 'midpoint': the trace each member's step moves its c along
        (StokesSimulation.dye_trajectory per member).  Set it with one name for all or one per member."""
        return self._orders("dye")

    @dye_trajectory.setter
    def dye_trajectory(self, order):
        self._set_orders(_lib.TRJ_DYE, order, "dye_trajectory")

    @property
    def velocity_trajectory(self):
        """(M,) names: the trace each member's inertial step forms u_a along.  It may be set while the member's
        inertia is off and takes effect when it is on."""
        return self._orders("velocity")

    @velocity_trajectory.setter
    def velocity_trajectory(self, order):
        self._set_orders(_lib.TRJ_VELOCITY, order, "velocity_trajectory")

    @property
    def tracer_trajectory(self):
        """(M,) names: 'midpoint' members read their tracers' velocity again half a step along the first one; a
        tracer whose midpoint leaves the mesh takes its Euler step (trajectory_info counts them)."""
        return self._orders("tracers")

    @tracer_trajectory.setter
    def tracer_trajectory(self, order):
        self._set_orders(_lib.TRJ_TRACERS, order, "tracer_trajectory")

    # ---- time-dependent strokes per member (pucfem_ens_set_stroke)
    def set_stroke(self, stroke, member=None):
        """The Stroke of one member, or (member=None) of all: a Stroke or None -- or, member=None, a list with one
        such entry per member.  Every stroke of an ensemble has one number of modes K (the shapes are shared).  A
        stroked member steps as StokesSimulation(..., stroke=) does, bit for bit, from its own start row and step
        count; a member without one keeps its SquirmerBC values.  It takes effect at the next step."""
        def one(s, m):
            _check_stroke(s)
            if s is None:
                return self.ctx.set_stroke(None, member=m)
            inner = boundary_sets(self.mesh.coords, self.mesh.markers)[1]
            shape, dirs = stroke_geometry(self.mesh.coords, inner, s.K, self.bcs[0].center)
            self.ctx.set_stroke(s, inner, shape, dirs, member=m)

        if member is not None:
            return one(stroke, int(member))
        if isinstance(stroke, (list, tuple)):
            _ensemble_strokes(stroke, self.M)
            for m, s in enumerate(stroke):
                if s is None:
                    one(None, m)
            for m, s in enumerate(stroke):
                if s is not None:
                    one(s, m)
        else:
            one(stroke, -1)

    def stroke_info(self, member=None):
        """pucfem_stroke_info per member: K (0: off), P, start, the steps its stroke has taken, the row its next step
        imposes, the driven nodes -- one member's dict, or (member=None) a dict of (M,) arrays."""
        if member is not None:
            return self.ctx.stroke_info(int(member))
        rows = [self.ctx.stroke_info(m) for m in range(self.M)]
        return {k: np.array([r[k] for r in rows]) for k in rows[0]}

    def boundary_values(self, member):
        """(nodes, values) of one member: the Dirichlet nodes and the (n, 2) values the device holds for them now."""
        nodes = stokes_setup(self.mesh, self.bcs[0])[1]
        return nodes, self.ctx.get_dirichlet(len(nodes), member=int(member))

    # ---- body forces per member (pucfem_ens_set_force, pucfem_ens_set_buoyancy)
    def set_force(self, force, member=None):
        """The body force of one member, or (member=None) of all: a pair, an (N, 2) field, a (pair, field) tuple or
        None -- or, member=None, a list with one such entry per member.  A forced member steps as
        StokesSimulation(..., force=...) does, bit for bit.  It takes effect at the next step."""
        L, h, N = self.ctx.L, self.ctx.h, self.mesh.N

        def one(f, m):
            if isinstance(f, tuple) and len(f) == 2 and np.shape(f[1]) == (N, 2):
                F, fn = np.asarray(f[0], dtype=np.float64), np.asarray(f[1], dtype=np.float64)
            else:
                F, fn = _force_args(f, N)
            F = None if F is None else np.ascontiguousarray(F, dtype=np.float64)
            fn = None if fn is None else np.ascontiguousarray(fn, dtype=np.float64)
            self.ctx._c(L.pucfem_ens_set_force(h, m, None if F is None else _lib.dptr(F),
                                               None if fn is None else _lib.dptr(fn)))

        if member is not None:
            return one(force, int(member))
        if isinstance(force, list):
            if len(force) != self.M:
                raise ValueError(f"force: one entry per member: {self.M} members, got {len(force)}")
            for m, f in enumerate(force):
                one(f, m)
        else:
            one(force, -1)

    def set_buoyancy(self, buoyancy, member=None):
        """The buoyancy of one member's dye c, or (member=None) of all: (g, beta, ref) -- f += g * beta * (c - ref) --
        or None for off; or, member=None, a list with one such entry per member."""
        L, h = self.ctx.L, self.ctx.h

        def one(b, m):
            if b is None:
                self.ctx._c(L.pucfem_ens_set_buoyancy(h, m, None, 0.0, 0.0))
                return
            try:
                g, beta, ref = b
                g = np.ascontiguousarray(g, dtype=np.float64)
                ok = g.shape == (2,)
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError("buoyancy: a member's entry is (g, beta, ref) with g a pair, or None")
            self.ctx._c(L.pucfem_ens_set_buoyancy(h, m, _lib.dptr(g), float(beta), float(ref)))

        if member is not None:
            return one(buoyancy, int(member))
        if isinstance(buoyancy, list):
            if len(buoyancy) != self.M:
                raise ValueError(f"buoyancy: one entry per member: {self.M} members, got {len(buoyancy)}")
            for m, b in enumerate(buoyancy):
                one(b, m)
        else:
            one(buoyancy, -1)

    def force_info(self, member=None):
        """pucfem_force_info per member: the mask of its terms, the forced steps since its setting last changed, its
        buoyancy terms and the device bytes the ensemble holds for forces -- one member's dict, or (member=None) a
        dict of (M,) arrays."""
        def one(m):
            o = (ct.c_int64 * 4)()
            self.ctx._c(self.ctx.L.pucfem_force_info(self.ctx.h, int(m), o))
            return dict(mask=int(o[0]), steps=int(o[1]), terms=int(o[2]), bytes=int(o[3]))

        if member is not None:
            return one(member)
        rows = [one(m) for m in range(self.M)]
        return {k: np.array([r[k] for r in rows]) for k in ("mask", "steps", "terms", "bytes")}

    @property
    def force_field(self):
        """(M, N, 2) every member's total force f of the current state (PUCFEM_F_FORCE); zeros for an unforced one."""
        return self.get(_lib.F_FORCE, 2)

    @property
    def u_rhs(self):
        """(M, N, 2) every member's r of its last forced step (PUCFEM_F_U_RHS); members that have taken none since
        their setting last changed make this an error: read one member with get(F_U_RHS, 2, member)."""
        return self.get(_lib.F_U_RHS, 2)

    # ---- Brownian tracers per member (pucfem_ens_set_tracer_diffusion)
    def set_tracer_diffusion(self, D, seed=0, member=None):
        """The tracers' diffusivity and random seed of one member, or (member=None) of all: one value each, or one per
        member.  A member steps as StokesSimulation(..., tracer_diffusivity=D, tracer_seed=seed) does, bit for bit;
        members with one seed draw the same increments.  It takes effect at the next step."""
        L, h = self.ctx.L, self.ctx.h
        if member is not None:
            self.ctx._c(L.pucfem_ens_set_tracer_diffusion(h, int(member), float(D), int(seed) & 0xFFFFFFFFFFFFFFFF))
            return
        d, s = _ensemble_diffusion(D, seed, self.M)
        if (d == d[0]).all() and (s == s[0]).all():
            self.ctx._c(L.pucfem_ens_set_tracer_diffusion(h, -1, float(d[0]), int(s[0])))
        else:
            for m in range(self.M):
                self.ctx._c(L.pucfem_ens_set_tracer_diffusion(h, m, float(d[m]), int(s[m])))

    @property
    def tracer_diffusivity(self):
        """(M,) the members' tracer diffusivities (StokesSimulation.tracer_diffusivity per member)."""
        return np.array([self.ctx.tracer_diffusion(m)[0] for m in range(self.M)])

    @property
    def tracer_seed(self):
        """(M,) uint64: the members' random seeds."""
        return np.array([self.ctx.tracer_diffusion(m)[1] for m in range(self.M)], dtype=np.uint64)

    @property
    def u_advected(self):
        """(M, N, 2) every member's u_a of its last inertial step (PUCFEM_F_U_ADV); members that have taken none
        since they were switched on make this an error: read one member with get(F_U_ADV, 2, member)."""
        return self.get(_lib.F_U_ADV, 2)

    def flow_info(self):
        """Context.flow_info of every member (one call each): {name: (M,) array}."""
        rows = [self.ctx.flow_info(m) for m in range(self.M)]
        return {k: np.array([r[k] for r in rows]) for k in FLOW_KEYS}

    def swimmer_loads(self):
        """Context.swimmer_loads of every member (one call each): {name: (M,) array}."""
        rows = [self.ctx.swimmer_loads(m) for m in range(self.M)]
        return {k: np.array([r[k] for r in rows]) for k in rows[0]}

    def surface_traction(self, member=None):
        """Context.surface_traction of every member: {name: (M, E) array}; theta and length are the mesh's, (E,).
        member = m: that member's alone."""
        if member is not None:
            return self.ctx.surface_traction(member)
        rows = [self.ctx.surface_traction(m) for m in range(self.M)]
        d = {k: np.stack([r[k] for r in rows]) for k in LOADS_KEYS[:8]}
        d["theta"], d["length"] = rows[0]["theta"], rows[0]["length"]
        return d

    def record_loads(self, capacity):
        """Context.record_loads for every member: each later step appends one row per member (0: off).  The step
        stays one captured graph; the rows' indices are counts in device memory."""
        self.ctx.record_loads(capacity)

    def loads_history(self):
        """(M, n, 11): every member's rows held, oldest first (Context.loads_history per member)."""
        return np.stack([self.ctx.loads_history(m) for m in range(self.M)])

    def loads_info(self, member=0):
        return self.ctx.loads_info(member)

    @property
    def tracers(self):
        return self.get(_lib.F_TRACERS)

    @tracers.setter
    def tracers(self, v):
        self.set(_lib.F_TRACERS, v)

    @property
    def tracer_status(self):
        return self.get(_lib.F_STATUS).astype(np.int64)

    @tracer_status.setter
    def tracer_status(self, v):
        self.set(_lib.F_STATUS, np.asarray(v, dtype=np.float64))

    @property
    def capture_step(self):
        """(M, n): per member and tracer, the 1-based step in which it was eaten; -1: never."""
        return self.get(_lib.F_CAPTURE_STEP).astype(np.int64)

    def tracer_info(self, member=0):
        return self.ctx.tracer_info(member)

    # ---- tracer stretching per member (pucfem_ens_set_tracer_stretch)
    def set_tracer_stretch(self, on, member=None):
        """Tracer stretching of one member (or, member=None, of all): its tracers carry the deformation gradient F
        as StokesSimulation(..., tracer_stretch=True) does, bit for bit; everything else of every member is the
        ensemble without it.  Switching a member on or off sets its F to the identity and its step count to 0.  The
        step stays one captured chain."""
        self.ctx.set_tracer_stretch(on, -1 if member is None else int(member))

    @property
    def tracer_stretch(self):
        """(M,) bool: the members' stretching flags.  Set it with one bool for all or one per member."""
        return np.array([self.ctx.stretch_info(m)["on"] for m in range(self.M)], dtype=bool)

    @tracer_stretch.setter
    def tracer_stretch(self, on):
        flags = _ensemble_stretch(on, self.M)
        if (flags == flags[0]).all():
            self.set_tracer_stretch(bool(flags[0]))
        else:
            for m, v in enumerate(flags):
                self.set_tracer_stretch(bool(v), m)

    @property
    def deformation_gradient(self):
        """(M, n, 2, 2) the members' F (identity for a member whose flag is off); needs a member with the flag on."""
        return self.get(_lib.F_DEFGRAD)

    @deformation_gradient.setter
    def deformation_gradient(self, F):
        F = np.ascontiguousarray(F, dtype=np.float64)
        if F.shape != (self.M, self.n_tracers, 2, 2):
            raise ValueError(f"deformation_gradient must be ({self.M}, {self.n_tracers}, 2, 2), got {F.shape}")
        self.set(_lib.F_DEFGRAD, F)

    def stretch_info(self, member=None, T=None):
        """Context.stretch_info of one member, or (member=None) the list over all members."""
        if member is not None:
            return self.ctx.stretch_info(int(member), T)
        return [self.ctx.stretch_info(m, T) for m in range(self.M)]

    def raster(self, width, height, fields=("c", "u"), window=None, member=None):
        """Every member's fields as images (pucfem_ens_raster: the swimmers side by side, each pixel located once
        for all members): {name: float32 (M, height, width) or (M, 2, height, width)}; member = m: that member's
        images without the leading axis.  Fields "u", "u_star", "p", "p2", "c", "vorticity" and, with dye channels,
        "dye0" .. "dye15" (channel k < K of every member)."""
        names, ids, ncomp = _sample_spec(fields)
        w, wp = _window(window)
        nm = self.M if member is None else 1
        img = np.zeros((nm, sum(ncomp), max(int(height), 0), max(int(width), 0)), dtype=np.float32)
        self.ctx._c(self.ctx.L.pucfem_ens_raster(self.ctx.h, len(ids), _lib.iptr(ids),
                                                 -1 if member is None else int(member), int(width), int(height), wp,
                                                 _lib.fptr(img)))
        return _split_images(names, ncomp, img if member is None else img[0])

    def streamlines(self, seeds, h, nsteps, unit=True, order=2, both=False, vmin=0.0, member=None):
        """Every member's streamlines from the same seeds (pucfem_ens_streamlines; Context.streamlines' arguments): a
        Streamlines with points (M, lines, nsteps + 1, 2), status and npts (M, lines); member = m: that member's
        alone, without the leading axis.  Each member's lines are those of a single run with its boundary values."""
        P, flags = _streamline_args(seeds, h, nsteps, unit, order, both, vmin)
        n, lines, ns = P.shape[0], P.shape[0] * (2 if both else 1), max(int(nsteps), 0) + 1
        nm = self.M if member is None else 1
        big = n < 1 or ns * lines * nm > (1 << 26)
        pts = np.zeros((1, 1, 1, 2) if big else (nm, ns, lines, 2))
        st = np.zeros((1, 1) if big else (nm, lines), dtype=np.int32)
        npts = np.zeros((1, 1) if big else (nm, lines), dtype=np.int32)
        self.ctx._c(self.ctx.L.pucfem_ens_streamlines(self.ctx.h, -1 if member is None else int(member), n,
                                                      _lib.dptr(P), float(h), int(nsteps), flags, float(vmin),
                                                      _lib.dptr(pts), _lib.iptr(st), _lib.iptr(npts)))
        pts = pts.transpose(0, 2, 1, 3)
        return Streamlines(pts, st, npts) if member is None else Streamlines(pts[0], st[0], npts[0])

    def step(self, n=1, stats=True):
        """n steps of every member: a list over the steps of lists over the members of step records
        (stats=False: no records are copied back, an empty list -- long sweeps that read only the final fields)."""
        self.step_count += n
        if not stats:
            self.ctx._c(self.ctx.L.pucfem_ens_step(self.ctx.h, n, None))
            return []
        st = (_lib.StepStats * max(n * self.M, 1))()
        self.ctx._c(self.ctx.L.pucfem_ens_step(self.ctx.h, n, st))
        out = [[st[s * self.M + m] for m in range(self.M)] for s in range(n)]
        self.history.extend(out)
        return out

    def info(self):
        o = (ct.c_int64 * 4)()
        self.ctx._c(self.ctx.L.pucfem_ens_info(self.ctx.h, o))
        return dict(members=o[0], member_tile=o[1], state_bytes=o[2], steps=o[3])

    def close(self):
        self.ctx.close()


def solve_ensemble(mesh: Mesh, bcs, dt=None, steps=1, scheme="color", device=0, tol: Tolerances | None = None,
                   inertia=False, advection="sl", tracer_diffusivity=0.0, tracer_seed=0, force=None, buoyancy=None,
                   dye_advection="sl", velocity_advection="sl", stroke=None, dye_trajectory=None,
                   velocity_trajectory=None, tracer_trajectory=None, trajectory="euler", dyes=None, loads=False,
                   tracer_stretch=False):
    """solve() for several squirmers at once (StokesEnsemble): one Result per member of `bcs`.  inertia: one bool
    for all members or one per member (StokesEnsemble.inertia).  dye_advection, velocity_advection: 'sl' or
    'maccormack', one name for all members or one per member (StokesEnsemble.set_advection); advection: 'sl' only (it
    would not say which of the two).  tracer_diffusivity, tracer_seed: one value for all members or one per member
    (StokesEnsemble.set_tracer_diffusion).  force, buoyancy: one setting for all members or a list with one per
    member (StokesEnsemble.set_force / set_buoyancy).  stroke: a Stroke for all members or a list with one Stroke or
    None per member (StokesEnsemble.set_stroke).  dye_trajectory, velocity_trajectory, tracer_trajectory: 'euler' or
    'midpoint', one name for all members or one per member; trajectory: StokesSimulation's keyword per member
    (StokesEnsemble.set_trajectory).  dyes (scheme 'color'): (K, N) dye channels for all members or (M, K, N)
    (StokesEnsemble.dyes); each member's Result.dyes holds its channels after the last step.  loads: every step records
    every member's loads on the device (StokesEnsemble.record_loads); each member's Result.loads holds its rows.
    tracer_stretch (scheme 'food'): one bool for all members or one per member (StokesEnsemble.set_tracer_stretch);
    the Result.deformation_gradient of a member whose flag is on holds its F after the last step."""
    _ensemble_advection(advection)
    if scheme not in ("color", "food"):
        raise ValueError("ensembles step the Stokes schemes 'color' and 'food'")
    dt = dt if dt is not None else (0.05 if scheme == "color" else 0.01)
    ens = StokesEnsemble(mesh, bcs, dt, scheme, device, tol, inertia=inertia, tracer_diffusivity=tracer_diffusivity,
                         tracer_seed=tracer_seed, force=force, buoyancy=buoyancy, dye_advection=dye_advection,
                         velocity_advection=velocity_advection, stroke=stroke, dye_trajectory=dye_trajectory,
                         velocity_trajectory=velocity_trajectory, tracer_trajectory=tracer_trajectory,
                         trajectory=trajectory, dyes=dyes, tracer_stretch=tracer_stretch)
    try:
        if loads:
            ens.record_loads(max(int(steps), 1))
        st = ens.step(steps) if steps else []
        u, p = ens.u, ens.get(_lib.F_P)
        ld = ens.loads_history() if loads else None
        dy = ens.dyes if dyes is not None else None
        c = ens.c if scheme == "color" else None
        tr, ts, cs = (ens.tracers, ens.tracer_status, ens.capture_step) if scheme == "food" else (None, None, None)
        on = ens.tracer_stretch if scheme == "food" else np.zeros(ens.M, dtype=bool)
        dg = ens.deformation_gradient if on.any() else None
    finally:
        ens.close()
    res = []
    for m in range(ens.M):
        r = Result(scheme, steps, u=u[m], p=p[m], stats=[s[m] for s in st])
        if ld is not None:
            r.loads = ld[m]
        if scheme == "color":
            r.c = c[m]
            if dy is not None:
                r.dyes = dy[m]
        else:
            r.tracers, r.tracer_status, r.capture_step = tr[m], ts[m], cs[m]
            if on[m]:
                r.deformation_gradient = dg[m]
        res.append(r)
    return res


def _literal_setup(mesh32: Mesh):
    """poisson.py:221-278 / heatEq.py:222-301 host setup on fp32 coordinates."""
    X = mesh32.coords
    assert X.dtype == np.float32, "poisson / heat read float32 coordinates (poisson.py:40)"
    pairs_all = find_boundary_pairs(X, L=1.0)
    op_pairs = filter_wall_pairs(X, pairs_all)
    y = X[:, 1]
    wall = (np.abs(y - np.float32(0.0)) < 1e-6) | (np.abs(y - np.float32(1.0)) < 1e-6)
    inner = mesh32.markers == INNER_BOUNDARY_MARKER
    nodes = np.where(wall | inner)[0].astype(np.int32)
    vals = np.where(inner[nodes], 0.0, 1.0)  # INNER_BOUNDARY_VALUE 0.0, OUTER (wall) 1.0
    return pairs_all, op_pairs, nodes, vals


def g_source_default(x, y):
    """poisson.py:235-236"""
    return 50 * np.sin(3 * y)


def poisson_load(mesh32: Mesh, g_source=g_source_default):
    """g(centroid) per triangle in the coordinates' dtype (poisson.py:135-139)."""
    X, T = mesh32.coords, mesh32.triangles
    x = X[T, 0]
    y = X[T, 1]
    three = X.dtype.type(3)
    return g_source((x[:, 0] + x[:, 1] + x[:, 2]) / three, (y[:, 0] + y[:, 1] + y[:, 2]) / three)


def poisson_solve(mesh: Mesh, g_source=g_source_default, device=0, tol: Tolerances | None = None):
    """poisson.py end to end on the GPU: fp32 assembly, literal periodic row merge and Dirichlet
    rows, BiCGStab on the literal operator.  Returns f (N,)."""
    m32 = mesh if mesh.coords.dtype == np.float32 else mesh.as_fp32()
    pairs_all, op_pairs, nodes, vals = _literal_setup(m32)
    ctx = Context(device)
    ctx.upload(Mesh(m32.coords.astype(np.float64), m32.markers, m32.triangles), coord_fp32=True)
    ctx.set_pairs(0, op_pairs)
    ctx.set_pairs(1, pairs_all)
    ctx.set_dirichlet(nodes, vals)
    ctx.set_source(poisson_load(m32, g_source))
    ctx.build("poisson", dt=0.0, tol=tol)
    ctx.step(1)
    f = ctx.get_field(_lib.F_SCALAR, (m32.N,))
    ctx.close()
    return f


class HeatSimulation:
    """heatEq.py: backward Euler (I + DT*A) u^{n+1} = u^n on the Poisson operator incl. BC rows,
    then reapply_periodic_u (unfiltered pairs) and reapply_dirchlect_u."""

    def __init__(self, mesh: Mesh, dt=0.02, device=0, tol: Tolerances | None = None):
        m32 = mesh if mesh.coords.dtype == np.float32 else mesh.as_fp32()
        self.mesh = m32
        pairs_all, op_pairs, nodes, vals = _literal_setup(m32)
        self.ctx = Context(device)
        self.ctx.upload(Mesh(m32.coords.astype(np.float64), m32.markers, m32.triangles), coord_fp32=True)
        self.ctx.set_pairs(0, op_pairs)
        self.ctx.set_pairs(1, pairs_all)
        self.ctx.set_dirichlet(nodes, vals)
        self.ctx.set_source(poisson_load(m32))
        self.ctx.build("heat", dt=dt, tol=tol)
        # heatEq.py:308-310: u = 0; reapply periodic; reapply Dirichlet
        u0 = np.zeros(m32.N)
        for m, s in pairs_all:
            u0[s] = u0[m]
        u0[nodes] = vals
        self.ctx.set_field(_lib.F_SCALAR, u0)

    def step(self, n=1):
        return self.ctx.step(n)

    @property
    def u(self):
        return self.ctx.get_field(_lib.F_SCALAR, (self.mesh.N,))

    def close(self):
        self.ctx.close()


DYE_PATTERNS = ("half", "stripe", "blob")


def dye_patterns(mesh: Mesh, names=DYE_PATTERNS):
    """(len(names), N) the reference's three dye starts, each 0 / 1 per node, for StokesSimulation.dyes:
      "half"   c = 1 where x < 0.5                                  (code/StokesColor.py:493-495)
      "stripe" c = 1 where |x - 0.2| < 0.05 / 2                     (scripts/good_visualization2.py:520-524)
      "blob"   c = 1 where |(x, y) - (0.5, 0.75)| < 0.1             (scripts/good_visualization.py:555-559)
    with the reference's expressions.  On a coarse mesh the 0.05-wide stripe can catch no node (mesh.1: check)."""
    X = np.asarray(mesh.coords, dtype=np.float64)
    out = np.zeros((len(names), len(X)))
    for k, name in enumerate(names):
        if name == "half":
            out[k, X[:, 0] < 0.5] = 1.0
        elif name == "stripe":
            out[k, np.where(np.abs(X[:, 0] - 0.2) < 0.05 / 2.0)[0]] = 1.0
        elif name == "blob":
            out[k, np.linalg.norm(X - np.array([0.5, 0.75]), axis=1) < 0.1] = 1.0
        else:
            raise ValueError(f"unknown dye pattern {name!r}: one of {DYE_PATTERNS}")
    return out


@dataclass
class Result:
    scheme: str
    steps: int
    u: np.ndarray | None = None
    c: np.ndarray | None = None
    p: np.ndarray | None = None
    tracers: np.ndarray | None = None
    tracer_status: np.ndarray | None = None
    capture_step: np.ndarray | None = None  # scheme 'food': per tracer, the 1-based step it was eaten in (-1: never)
    scalar: np.ndarray | None = None
    stats: list = field(default_factory=list)
    dyes: np.ndarray | None = None  # scheme 'color' with dyes=: the final dye channels (K, N)
    deformation_gradient: np.ndarray | None = None  # scheme 'food' with tracer_stretch=True: (n, 2, 2) per tracer
    loads: np.ndarray | None = None  # Stokes schemes with loads=True: (steps, 11), the row number and LOADS_KEYS per step


def solve(mesh: Mesh, bc: SquirmerBC | None = None, dt=None, steps=1, scheme="color", device=0,
          tol: Tolerances | None = None, log=None, dyes=None, inertia=False, advection="sl", tracer_diffusivity=0.0,
          tracer_seed=0, force=None, buoyancy=None, stroke=None, trajectory="euler", loads=False,
          tracer_stretch=False):
    """The north-star call surface: run `steps` steps of a reference script's loop on the GPU.

    scheme 'color' = StokesColor.py, 'food' = StokesFood.py, 'heat' = heatEq.py (steps of
    backward Euler), 'poisson' = poisson.py (one steady solve).  `log`, if given, receives the
    reference's per-step print line (StokesColor.py:586 / StokesFood.py:505).  dyes (scheme 'color'): (K, N) dye
    channels advected beside c (StokesSimulation.dyes); the result's `dyes` holds them after the last step.
    inertia (schemes 'color' and 'food'): every step advects the velocity by itself in front of the viscous solve
    (StokesSimulation.inertia).  advection 'sl' | 'maccormack' (schemes 'color' and 'food'): the first-order
    semi-Lagrangian transport of the reference, or the limited MacCormack scheme (second order) for the dye of a
    'color' run and the velocity of an inertial one (StokesSimulation.dye_advection / velocity_advection).
    tracer_diffusivity, tracer_seed (schemes 'color' and 'food'): Brownian tracers, a random walk of that diffusivity
    per tracer and step on top of the move, reproducible from the seed (StokesSimulation.tracer_diffusivity).
    force, buoyancy (schemes 'color' and 'food'; buoyancy 'color'): the body force of the steps, a pair, an (N, 2)
    field or None, and the Buoyancy of the dye (StokesSimulation.force / buoyancy; its terms may name the dyes=).
    stroke (schemes 'color' and 'food'): a Stroke, the squirmer's boundary values per step (StokesSimulation.stroke).
    trajectory 'euler' | 'midpoint' (schemes 'color' and 'food'): the path of whatever the run transports -- the dye
    on 'color', the velocity with inertia, the tracers on 'food' (StokesSimulation.dye_trajectory and its kin).
    loads (schemes 'color' and 'food'): every step records the swimmer's loads on the device
    (StokesSimulation.record_loads); the result's `loads` holds the (steps, 11) rows.
    tracer_stretch (scheme 'food'): the tracers carry their deformation gradient (StokesSimulation.tracer_stretch);
    the result's `deformation_gradient` holds it after the last step."""
    if _stretch_flag(tracer_stretch) and scheme != "food":
        raise ValueError("tracer_stretch belongs to scheme 'food'")
    if loads and scheme not in ("color", "food"):
        raise ValueError("loads belong to the Stokes schemes 'color' and 'food'")
    if trajectory_order(trajectory) != _lib.TRJ_EULER and scheme not in ("color", "food"):
        raise ValueError("trajectory belongs to the Stokes schemes 'color' and 'food'")
    if stroke is not None and scheme not in ("color", "food"):
        raise ValueError("stroke belongs to the Stokes schemes 'color' and 'food'")
    _check_stroke(stroke)
    if force is not None and scheme not in ("color", "food"):
        raise ValueError("force belongs to the Stokes schemes 'color' and 'food'")
    if buoyancy is not None and scheme != "color":
        raise ValueError("buoyancy belongs to scheme 'color'")
    if (tracer_diffusivity != 0.0 or tracer_seed != 0) and scheme not in ("color", "food"):
        raise ValueError("tracer_diffusivity belongs to the Stokes schemes 'color' and 'food'")
    if advection_scheme(advection) and scheme not in ("color", "food"):
        raise ValueError("advection belongs to the Stokes schemes 'color' and 'food'")
    if dyes is not None and scheme != "color":
        raise ValueError("dyes belong to scheme 'color'")
    if inertia and scheme not in ("color", "food"):
        raise ValueError("inertia belongs to the Stokes schemes 'color' and 'food'")
    if scheme in ("color", "food"):
        bc = bc or (SquirmerBC() if scheme == "color" else SquirmerBC(nu=1.0))
        dt = dt if dt is not None else (0.05 if scheme == "color" else 0.01)
        sim = StokesSimulation(mesh, bc, dt, scheme, device, tol, inertia=inertia, advection=advection,
                               tracer_diffusivity=tracer_diffusivity, tracer_seed=tracer_seed, force=force,
                               stroke=stroke, trajectory=trajectory, tracer_stretch=tracer_stretch)
        if dyes is not None:
            sim.dyes = dyes
        if buoyancy is not None:  # (behind the channels its terms may name)
            sim.buoyancy = buoyancy
        if loads:
            sim.record_loads(max(int(steps), 1))
        st = sim.step(steps) if steps else []
        res = Result(scheme, steps, u=sim.u, p=sim.field(_lib.F_P), stats=st)
        if loads:
            res.loads = sim.loads_history()
        if dyes is not None:
            res.dyes = sim.dyes
        if scheme == "color":
            res.c = sim.c
            if log:
                _, _, var0 = _mixing0(mesh, sim)
                for k, s in enumerate(st):
                    log(f"Step: {k}, Div(u*): {s.max_div_star:.2e}, Final Div(u): {s.max_final_div:.2e}, "
                        f"Color mixing progress={1.0 - s.mix_var / (var0 + 1e-16):.3f}")
        else:
            res.tracers, res.tracer_status, res.capture_step = sim.tracers, sim.tracer_status, sim.capture_step
            if tracer_stretch:
                res.deformation_gradient = sim.deformation_gradient
            if log:
                for k, s in enumerate(st):
                    log(f"Step: {k}, Div(u*): {s.max_div_star:.2e}, Final Div(u): {s.max_final_div:.2e}, "
                        f"Eaten (Red): {s.eaten}, Uneaten (Blue): {len(res.tracer_status) - s.eaten}")
        sim.close()
        return res
    if scheme == "heat":
        h = HeatSimulation(mesh, dt if dt is not None else 0.02, device, tol)
        st = h.step(steps)
        res = Result(scheme, steps, scalar=h.u, stats=st)
        h.close()
        return res
    if scheme == "poisson":
        return Result(scheme, 1, scalar=poisson_solve(mesh, device=device, tol=tol))
    raise ValueError(f"unknown scheme {scheme!r}")


def _mixing0(mesh, sim):
    """I0, mu0, var0 of the initial dye field c = 1[x < 0.5] (StokesColor.py:493-497)."""
    c0 = np.zeros(mesh.N)
    c0[mesh.coords[:, 0] < 0.5] = 1.0
    from .ops import mixing_index_host

    return mixing_index_host(mesh, c0)
