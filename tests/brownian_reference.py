"""Brownian tracers restated in numpy (include/pucfem.h): Philox4x32-10, the 53-bit uniforms
and one tracer step with the random-walk increment.  Written from the text of the semantics, not from the kernels:
every product and sum as written there, in float64, so the increments, the wrap and the reflection hold the device's
bits; the interpolated velocity is the oracle's (locate_bary / plane_coefficients), as in oracle.tracer_step.
"""
import numpy as np

import oracle as O

M0, M1 = 0xD2511F53, 0xCD9E8D57  # the round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # the key increments
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: (..., 4) and key: (..., 2) arrays of 32-bit words (broadcast against each other) -> (..., 4) uint32."""
    c = np.asarray(counter, dtype=np.uint64) & MASK
    k = np.asarray(key, dtype=np.uint64) & MASK
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for r in range(10):
        p0 = np.uint64(M0) * c0  # (32 x 32 -> 64 bits: no overflow in uint64)
        p1 = np.uint64(M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        if r < 9:
            k0 = (k0 + np.uint64(W0)) & MASK
            k1 = (k1 + np.uint64(W1)) & MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def uniform53(hi, lo):
    """U = ((hi >> 5) * 2^26 + (lo >> 6)) * 2^-53 in [0, 1): 27 bits of hi, 26 of lo, every step exact."""
    hi = np.asarray(hi, dtype=np.uint32)
    lo = np.asarray(lo, dtype=np.uint32)
    return ((hi >> np.uint32(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint32(6)).astype(np.float64)) * 2.0**-53


def uniforms(seed, k, stepno):
    """(U1, U2) of tracers k (array) in the 1-based tracer step stepno."""
    k = np.asarray(k, dtype=np.uint64)
    ctr = np.stack([k, np.full_like(k, stepno), np.zeros_like(k), np.zeros_like(k)], -1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    return uniform53(r[..., 0], r[..., 1]), uniform53(r[..., 2], r[..., 3])


def velocity(pts, u, X, T):
    """oracle.tracer_step's interpolation: (n, 2), NaN outside the mesh.  u = None: the fluid at rest (exact zeros
    inside the mesh)."""
    tri = O.locate_bary(X, T, pts[:, 0], pts[:, 1])
    vel = np.full((len(pts), 2), np.nan)
    ok = tri >= 0
    if u is None:
        vel[ok] = 0.0
        return vel
    for d in range(2):
        pc = O.plane_coefficients(X, T, u[:, d])[tri[ok]]
        vel[ok, d] = pc[:, 0] * pts[ok, 0] + pc[:, 1] * pts[ok, 1] + pc[:, 2]
    return vel


def brownian_step(pts, status, capstep, stepno, u, dt, X, T, D, seed, capture=0.28, center=(0.5, 0.5), ylo=None,
                  yhi=None, vel=None):
    """One Brownian tracer step (D > 0) of the tracer step `stepno` (1-based): new (pts, status, capstep).  Absorbed
    tracers (status 1 on entry) are left as they are.  vel: the velocities, when the caller has them already."""
    ylo = X[:, 1].min() if ylo is None else ylo
    yhi = X[:, 1].max() if yhi is None else yhi
    pts, status, capstep = pts.copy(), status.copy(), capstep.copy()
    free = np.where(status != 1)[0]
    if len(free) == 0:
        return pts, status, capstep
    p = pts[free]
    v = velocity(p, u, X, T) if vel is None else vel[free]
    u1, u2 = uniforms(seed, free, stepno)
    a = np.sqrt(6.0 * D * dt)
    nx = (p[:, 0] + v[:, 0] * dt) + a * (2.0 * u1 - 1.0)
    ny = (p[:, 1] + v[:, 1] * dt) + a * (2.0 * u2 - 1.0)
    nx = np.mod(nx, 1.0)
    with np.errstate(invalid="ignore"):
        low, high = ny < ylo, ny > yhi
    ny = np.where(low, ylo + (ylo - ny), np.where(high, yhi - (ny - yhi), ny))
    pts[free, 0], pts[free, 1] = nx, ny
    ddx, ddy = nx - center[0], ny - center[1]
    with np.errstate(invalid="ignore"):
        hit = np.sqrt(ddx * ddx + ddy * ddy) <= capture
    status[free[hit]] = 1
    capstep[free[hit]] = stepno
    return pts, status, capstep


def plain_step(pts, status, capstep, stepno, u, dt, X, T, capture=0.28, center=(0.5, 0.5)):
    """The step with D = 0 (oracle.tracer_step, with the capture steps): eaten tracers keep moving."""
    st0 = status
    pts, status = O.tracer_step(pts, status, u, dt, X, T, capture, center)
    capstep = capstep.copy()
    capstep[(status == 1) & (st0 != 1)] = stepno
    return pts, status, capstep


def run(pts, u, dt, X, T, D, seed, nsteps, capture=0.28, center=(0.5, 0.5)):
    """nsteps tracer steps from status 0 in the frozen flow u: dict of the final state and the per-step eaten counts,
    the smallest margin |dist - capture| met (over free tracers' new positions), and the non-finite count."""
    status = np.zeros(len(pts), dtype=np.int64)
    capstep = np.full(len(pts), -1, dtype=np.int64)
    eaten, margin = [], np.inf
    for s in range(1, nsteps + 1):
        moved = status != 1 if D > 0 else np.ones(len(pts), dtype=bool)
        if D > 0:
            pts, status, capstep = brownian_step(pts, status, capstep, s, u, dt, X, T, D, seed, capture, center)
        else:
            pts, status, capstep = plain_step(pts, status, capstep, s, u, dt, X, T, capture, center)
        d = np.sqrt((pts[moved, 0] - center[0]) ** 2 + (pts[moved, 1] - center[1]) ** 2)
        if np.isfinite(d).any():
            margin = min(margin, float(np.nanmin(np.abs(d - capture))))
        eaten.append(int((status == 1).sum()))
    return dict(tracers=pts, status=status, capture=capstep, eaten=eaten, margin=margin,
                nonfinite=int((~np.isfinite(pts)).any(1).sum()))
