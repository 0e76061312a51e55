"""Tracer stretching restated in numpy (include/pucfem.h "tracer stretching"; helper of
tests/test_stretch_host.py, tests/test_gpu_stretch.py and tests/test_gpu_ens_stretch.py).

Written from the text of the semantics, not from the kernels: every product and sum as written there, elementwise in
float64 (no einsum and no @, which could reorder the sums), so F holds the device's bits.  The plane coefficients are
the oracle's (locate_bary / plane_coefficients), the velocities brownian_reference.velocity's, the midpoint
trajectory_reference.tracer_mid_velocity's; the positions, status and capture steps move by the restatements the
tracer kernels are already held to (brownian_reference, trajectory_reference).
"""
import numpy as np

import brownian_reference as B
import oracle as O
import trajectory_reference as TR

HOLE_SEED = (0.5, 0.5)  # inside the swimmer: no triangle holds it, so it has no velocity from the first step on


def identity(n):
    F = np.zeros((n, 4))
    F[:, 0] = F[:, 3] = 1.0
    return F


def coefficients(tri, u, X, T):
    """(n, 4): (pa, pb) of ux and (pa, pb) of uy in the triangles tri; NaN where tri < 0."""
    g = np.full((len(tri), 4), np.nan)
    ok = tri >= 0
    for d in range(2):
        pc = O.plane_coefficients(X, T, np.ascontiguousarray(u[:, d]))[tri[ok]]
        g[ok, 2 * d] = pc[:, 0]
        g[ok, 2 * d + 1] = pc[:, 1]
    return g


def jacobian(pts, u, dt, X, T, midpoint):
    """(J (n, 4), t, tm): the Jacobian J00 J01 J10 J11 of one tracer step at pts (NaN where the tracer has no
    velocity), the triangle of the start and that of the midpoint (-1: none, the Euler J)."""
    n = len(pts)
    t = O.locate_bary(X, T, pts[:, 0], pts[:, 1])
    g = coefficients(t, u, X, T)
    ax, bx, ay, by = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
    J = np.stack([1.0 + dt * ax, dt * bx, dt * ay, 1.0 + dt * by], 1)
    tm = -np.ones(n, dtype=np.int64)
    if not midpoint:
        return J, t, tm
    hdt = 0.5 * dt
    w, v, fell = TR.tracer_mid_velocity(pts, u, dt, X, T)
    assert np.array_equal(np.isnan(v[:, 0]), t < 0)
    with np.errstate(invalid="ignore"):
        mx, my = np.mod(pts[:, 0] + v[:, 0] * hdt, 1.0), pts[:, 1] + v[:, 1] * hdt
    tm = O.locate_bary(X, T, mx, my)
    assert np.array_equal(fell, (t >= 0) & (tm < 0))
    h = coefficients(tm, u, X, T)
    cx, dx, cy, dy = h[:, 0], h[:, 1], h[:, 2], h[:, 3]
    A00, A01, A10, A11 = 1.0 + hdt * ax, hdt * bx, hdt * ay, 1.0 + hdt * by
    B00, B01 = cx * A00 + dx * A10, cx * A01 + dx * A11
    B10, B11 = cy * A00 + dy * A10, cy * A01 + dy * A11
    Jm = np.stack([1.0 + dt * B00, dt * B01, dt * B10, 1.0 + dt * B11], 1)
    got = tm >= 0
    J[got] = Jm[got]
    return J, t, tm


def update(F, J, t, moved=None):
    """F' = J F for the tracers whose iteration runs (moved; None: all): NaN rows where the tracer has no velocity."""
    F00, F01, F10, F11 = F[:, 0], F[:, 1], F[:, 2], F[:, 3]
    J00, J01, J10, J11 = J[:, 0], J[:, 1], J[:, 2], J[:, 3]
    with np.errstate(invalid="ignore"):
        out = np.stack([J00 * F00 + J01 * F10, J00 * F01 + J01 * F11, J10 * F00 + J11 * F10, J10 * F01 + J11 * F11], 1)
    out[t < 0] = np.nan
    if moved is not None:
        out[~moved] = F[~moved]
    return out


def step(pts, status, capstep, F, stepno, u, dt, X, T, midpoint=False, D=0.0, seed=0, capture=0.28,
         center=(0.5, 0.5)):
    """One tracer step with stretching on: (pts, status, capstep, F, info), info = dict(t, tm, moved, fell)."""
    moved = status != 1 if D > 0 else np.ones(len(pts), dtype=bool)
    J, t, tm = jacobian(pts, u, dt, X, T, midpoint)
    Fn = update(F, J, t, moved)
    fell = 0
    if midpoint:
        p, s, c, fell = TR.tracer_step(pts, status, capstep, stepno, u, dt, X, T, D, seed, capture, center)
    elif D > 0:
        p, s, c = B.brownian_step(pts, status, capstep, stepno, u, dt, X, T, D, seed, capture, center)
    else:
        p, s, c = B.plain_step(pts, status, capstep, stepno, u, dt, X, T, capture, center)
    return p, s, c, Fn, dict(t=t, tm=tm, moved=moved, fell=fell)


def run(pts, u, dt, X, T, nsteps, midpoint=False, D=0.0, seed=0, capture=0.28, center=(0.5, 0.5)):
    """nsteps tracer steps from status 0 and F = I in the frozen flow u: the states after every step (lists of pts,
    status, capstep, F) and per step the triangle sequences (t: start, tm: midpoint) and the moved masks."""
    n = len(pts)
    p, s, c, F = pts.copy(), np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int64), identity(n)
    out = dict(pts=[], status=[], capture=[], F=[], t=[], tm=[], moved=[], fell=[])
    for k in range(1, nsteps + 1):
        p, s, c, F, info = step(p, s, c, F, k, u, dt, X, T, midpoint, D, seed, capture, center)
        for key, val in (("pts", p), ("status", s), ("capture", c), ("F", F)):
            out[key].append(val.copy())
        for key in ("t", "tm", "moved", "fell"):
            out[key].append(info[key])
    return out


def summary(F):
    """pucfem_tracer_stretch_info's values 2..7 of F (n, 4) and the terms of the log sum: dict(finite, folded,
    lam_max, lam_min, sum_log, terms, abs_log); with no finite row lam_max = 0 and lam_min = inf."""
    F00, F01, F10, F11 = F[:, 0], F[:, 1], F[:, 2], F[:, 3]
    fin = np.isfinite(F).all(1)
    with np.errstate(invalid="ignore"):
        C00, C01, C11 = F00 * F00 + F10 * F10, F00 * F01 + F10 * F11, F01 * F01 + F11 * F11
        lam = 0.5 * ((C00 + C11) + np.sqrt((C00 - C11) * (C00 - C11) + 4.0 * (C01 * C01)))
        det = F00 * F11 - F01 * F10
    lam, det = lam[fin], det[fin]
    pos = lam > 0
    logs = np.log(lam[pos])
    return dict(finite=int(fin.sum()), folded=int((det <= 0).sum()), lam_max=float(lam.max()) if len(lam) else 0.0,
                lam_min=float(lam.min()) if len(lam) else np.inf, sum_log=float(logs.sum()), terms=int(pos.sum()),
                abs_log=float(np.abs(logs).sum()))


def frozen_flow(mesh, B1=1.0, B2=2.0, nu=0.1, dt=0.05, nsteps=4):
    """u after nsteps oracle Stokes steps from rest: the frozen flow of the Jacobian and device tests."""
    ref = O.StokesRef(mesh.coords, mesh.markers, mesh.triangles, dt, nu, B1, B2, "color")
    u, c = ref.initial()
    for _ in range(nsteps):
        out = ref.step(u, c)
        u, c = out["u"], out["c"]
    return np.ascontiguousarray(u)


# ---- the inputs of tests/test_gpu_stretch.py (tests/test_stretch_host.py asserts the branches they reach)
B1, B2, NU, DT = 1.0, 2.0, 0.1, 0.05
DENSITIES = {489: 25, 561: 27}  # tracers -> tracer_init's density
DIFFUSION = ((0.0, 0), (1e-3, 7))  # (D, seed)
NSTEPS = 8
# The squirmer's flow is tangential at the swimmer, so no midpoint of these seeds leaves the mesh in it: the rigid
# rotation of tests/trajectory_reference.py (theta = 0.5 per step) carries the corner seeds' midpoints through the
# walls, three steps of it with D = 0 are the fallen-back midpoint's case.
ROTATION_STEPS = 3
_cache = {}


def gpu_flow(mesh, name):
    key = ("flow", name)
    if key not in _cache:
        _cache[key] = (frozen_flow(mesh, B1, B2, NU, DT) if name == "squirmer" else TR.rotation(mesh.coords, DT, 0.5))
    return _cache[key]


def gpu_cases(n, midpoint):
    """(flow name, D, seed, steps) of the device test with n tracers."""
    cases = [("squirmer", D, seed, NSTEPS) for D, seed in DIFFUSION]
    if midpoint:
        cases.append(("rotation", 0.0, 0, ROTATION_STEPS))
    return cases


def gpu_run(mesh, n, midpoint, flow, D, seed, nsteps):
    """run() of one device case, computed once and shared (callers leave it unchanged)."""
    key = (n, midpoint, flow, D, seed, nsteps)
    if key not in _cache:
        _cache[key] = run(seeds(DENSITIES[n]), gpu_flow(mesh, flow), DT, mesh.coords, mesh.triangles, nsteps, midpoint,
                          D, seed)
    return _cache[key]


def seeds(density):
    """tracer_init(density=density) and the seed inside the swimmer's hole appended: 489 tracers for density 25 (the
    one-block kernel), 561 for 27 (the cloud kernel)."""
    return np.ascontiguousarray(np.vstack([O.tracer_init(density=density), np.array([HOLE_SEED])]))
