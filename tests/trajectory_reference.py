"""The oracle of the midpoint trajectories (helper of tests/test_trajectory_host.py and tests/test_gpu_trajectory.py).

The midpoint trace is a composition of operations the oracle already has, so it needs no reference code of its own:

    W   = sl_advect(u[:, k], u, dt / 2) per component   the velocity half a step back; a node whose midpoint is not
                                                        found keeps u (sl_advect keeps the node's own value)
    out = sl_advect(c, W, dt)                           the whole step along it

and with MacCormack (tests/maccormack_reference.py)

    ch = sl_advect(c, W+, dt),  cb = sl_advect(ch, W-, -dt),  W- from -dt / 2,  then the clamp on T1 = ch's triangle.

The tracer step reads the velocity again at the midpoint of the Euler step and moves with it; a tracer whose midpoint
leaves the mesh moves with the velocity it started with (brownian_reference.velocity, brownian_step with vel=).
"""
import numpy as np

import brownian_reference as B
import maccormack_reference as R
import oracle as O

NO_BACK, NO_FWD, NO_MID1, NO_MID2 = 1, 2, 4, 8


def rotation(X, dt, theta=0.5, center=(0.5, 0.5)):
    """The rigid rotation u = Omega x (X - center) with Omega dt = theta."""
    om = theta / dt
    return np.ascontiguousarray(np.stack([-om * (X[:, 1] - center[1]), om * (X[:, 0] - center[0])], 1))


def ring(X, lo=0.30, hi=0.44, center=(0.5, 0.5)):
    r = np.hypot(X[:, 0] - center[0], X[:, 1] - center[1])
    return (r > lo) & (r < hi), r


def mid_velocity(u, dt, X, T, tree):
    """(W, not-found mask): u interpolated at every node's half-step departure point, the node's own where none."""
    W = np.empty_like(u)
    nf = None
    for k in range(2):
        W[:, k], nfk = O.sl_advect(np.ascontiguousarray(u[:, k]), u, 0.5 * dt, X, T, tree)
        assert nf is None or np.array_equal(nf, nfk)  # (the locate does not depend on the field)
        nf = nfk
    return np.ascontiguousarray(W), nf


def mid_advect(c, u, dt, X, T, tree):
    """One midpoint semi-Lagrangian step of the nodal field c: (out, marks, W)."""
    W, nfm = mid_velocity(u, dt, X, T, tree)
    out, nf = O.sl_advect(c, W, dt, X, T, tree)
    return out, nf.astype(np.int32) * NO_BACK + nfm.astype(np.int32) * NO_MID1, W


def mid_mc_advect(c, u, dt, X, T, tree, rule="tree"):
    """One limited MacCormack step along midpoint trajectories: (out, marks, T1, clamped mask)."""
    Wp, nfm1 = mid_velocity(u, dt, X, T, tree)
    Wm, nfm2 = mid_velocity(u, -dt, X, T, tree)
    ch, nf1 = O.sl_advect(c, Wp, dt, X, T, tree)
    cb, nf2 = O.sl_advect(ch, Wm, -dt, X, T, tree)
    t1 = R.locate(Wp, dt, X, T, tree, rule=rule)
    assert np.array_equal(t1 < 0, nf1)
    out, clamped = R.limit(c, ch, cb, t1, nf1, nf2, T)
    marks = (nf1.astype(np.int32) * NO_BACK + nf2.astype(np.int32) * NO_FWD + nfm1.astype(np.int32) * NO_MID1 +
             nfm2.astype(np.int32) * NO_MID2)
    return out, marks, t1, clamped


def departure_radius(u, dt, X, center=(0.5, 0.5)):
    """|X - dt u - center| per node: the radius the straight step along u departs from."""
    q = X - dt * u
    return np.hypot(q[:, 0] - center[0], q[:, 1] - center[1])


def tracer_mid_velocity(pts, u, dt, X, T):
    """(w, v, fell): the velocity at the midpoint of each tracer's Euler step, the velocity at its position, and the
    tracers that have a velocity but whose midpoint is outside the mesh (they keep it)."""
    v = B.velocity(pts, u, X, T)
    hdt = 0.5 * dt
    with np.errstate(invalid="ignore"):
        pm = np.stack([np.mod(pts[:, 0] + v[:, 0] * hdt, 1.0), pts[:, 1] + v[:, 1] * hdt], 1)
    w = B.velocity(pm, u, X, T)
    lost = np.isnan(w[:, 0])
    return np.where(lost[:, None], v, w), v, lost & ~np.isnan(v[:, 0])


def tracer_step(pts, status, capstep, stepno, u, dt, X, T, D=0.0, seed=0, capture=0.28, center=(0.5, 0.5)):
    """One midpoint tracer step, plain (D = 0: every tracer moves, eaten ones too) or Brownian: (pts, status, capstep,
    fell), fell the count of tracers that fell back among those the step moves."""
    w, _, fell = tracer_mid_velocity(pts, u, dt, X, T)
    if D > 0:
        moved = status != 1
        p, s, c = B.brownian_step(pts, status, capstep, stepno, u, dt, X, T, D, seed, capture, center, vel=w)
        return p, s, c, int((fell & moved).sum())
    p = pts.copy()
    p[:, 0] = np.mod(p[:, 0] + w[:, 0] * dt, 1.0)
    p[:, 1] = p[:, 1] + w[:, 1] * dt
    with np.errstate(invalid="ignore"):
        hit = np.sqrt((p[:, 0] - center[0]) * (p[:, 0] - center[0]) + (p[:, 1] - center[1]) * (p[:, 1] - center[1])) <= capture
    s, c = status.copy(), capstep.copy()
    c[hit & (s != 1)] = stepno
    s[hit] = 1
    return p, s, c, int(fell.sum())
