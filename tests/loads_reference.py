"""The numpy restatement of the swimmer loads (helper of tests/test_loads_host.py and the GPU loads tests).

Definitions: include/pucfem.h ("swimmer loads") and csrc/pucfem_loads.hpp.  Every product and sum is a numpy line (or
one left-to-right expression) of its own, in the kernel's order; the library is built with -ffp-contract=off, so the
per-edge values and the per-triangle dissipation terms hold the device's bits.  The reduced values are compared with
math.fsum of these terms within the worst case of any summation order.
"""
import math

import numpy as np

LOADS_KEYS = ("force_pressure_x", "force_pressure_y", "force_viscous_x", "force_viscous_y", "torque_pressure",
              "torque_viscous", "power_pressure", "power_viscous", "dissipation", "perimeter")
EPS = 2.0 ** -53


def surface_edges(X, markers, T):
    """tri, a, b, opp (int32) of the swimmer surface: the local edges k -> (k + 1) mod 3 whose two ends carry marker 2
    and which lie in exactly one triangle, ascending in (triangle, k)."""
    T = np.asarray(T)
    inner = np.asarray(markers) == 2
    cand = []
    count = {}
    for t in range(len(T)):
        for k in range(3):
            i, j = int(T[t, k]), int(T[t, (k + 1) % 3])
            if inner[i] and inner[j]:
                cand.append((t, k, i, j))
                key = (min(i, j), max(i, j))
                count[key] = count.get(key, 0) + 1
    keep = [(t, k, i, j) for t, k, i, j in cand if count[(min(i, j), max(i, j))] == 1]
    keep.sort()
    tri = np.array([e[0] for e in keep], dtype=np.int32)
    a = np.array([e[2] for e in keep], dtype=np.int32)
    b = np.array([e[3] for e in keep], dtype=np.int32)
    opp = np.array([T[e[0], (e[1] + 2) % 3] for e in keep], dtype=np.int32)
    return tri, a, b, opp


def tri_gradients(X, T, u):
    """Gxx, Gxy, Gyx, Gyy, det, ok per triangle: the constant P1 gradient of u, the oracle's _divergence_sums form."""
    T = np.asarray(T)
    x1, y1 = X[T[:, 0], 0], X[T[:, 0], 1]
    x2, y2 = X[T[:, 1], 0], X[T[:, 1], 1]
    x3, y3 = X[T[:, 2], 0], X[T[:, 2], 1]
    b1 = y2 - y3
    b2 = y3 - y1
    b3 = y1 - y2
    c1 = x3 - x2
    c2 = x1 - x3
    c3 = x2 - x1
    det = x1 * b1 + x2 * b2 + x3 * b3
    ok = np.abs(det) >= 1e-14
    inv = 1.0 / np.where(ok, det, 1.0)
    ux, uy = u[:, 0], u[:, 1]
    a, b, c = T[:, 0], T[:, 1], T[:, 2]
    gxx = (ux[a] * b1 + ux[b] * b2 + ux[c] * b3) * inv
    gxy = (ux[a] * c1 + ux[b] * c2 + ux[c] * c3) * inv
    gyx = (uy[a] * b1 + uy[b] * b2 + uy[c] * b3) * inv
    gyy = (uy[a] * c1 + uy[b] * c2 + uy[c] * c3) * inv
    return gxx, gxy, gyx, gyy, det, ok


def edge_terms(X, T, edges, u, p, p2, nu, center=(0.5, 0.5)):
    """(E, 8) the per-edge values in LOADS_KEYS' order and (E,) the lengths."""
    tri, i, j, o = edges
    gxx, gxy, gyx, gyy, _, _ = tri_gradients(X, np.asarray(T)[tri], u)
    xi, yi = X[i, 0], X[i, 1]
    xj, yj = X[j, 0], X[j, 1]
    xo, yo = X[o, 0], X[o, 1]
    Pi = p[i] + p2[i]
    Pj = p[j] + p2[j]
    ex = xj - xi
    ey = yj - yi
    nx = ey
    ny = -ex
    side = nx * (xo - xi) + ny * (yo - yi)
    flip = side < 0.0
    nx = np.where(flip, -nx, nx)
    ny = np.where(flip, -ny, ny)
    Pb = (Pi + Pj) * 0.5
    fpx = -(Pb * nx)
    fpy = -(Pb * ny)
    sxx = gxx + gxx
    sxy = gxy + gyx
    syy = gyy + gyy
    fvx = nu * (sxx * nx + sxy * ny)
    fvy = nu * (sxy * nx + syy * ny)
    ubx = (u[i, 0] + u[j, 0]) * 0.5
    uby = (u[i, 1] + u[j, 1]) * 0.5
    rx = (xi + xj) * 0.5 - center[0]
    ry = (yi + yj) * 0.5 - center[1]
    tp = rx * fpy - ry * fpx
    tv = rx * fvy - ry * fvx
    wp = -(ubx * fpx + uby * fpy)
    wv = -(ubx * fvx + uby * fvy)
    length = np.sqrt(ex * ex + ey * ey)
    return np.stack([fpx, fpy, fvx, fvy, tp, tv, wp, wv], axis=1), length


def dissipation_terms(X, T, u, nu):
    """The per-triangle terms nu (|det| / 2) ((2 Gxx^2 + 2 Gyy^2) + (Gxy + Gyx)^2) of the triangles with
    |det| >= 1e-14."""
    gxx, gxy, gyx, gyy, det, ok = tri_gradients(X, T, u)
    s = gxy + gyx
    q = (2.0 * (gxx * gxx) + 2.0 * (gyy * gyy)) + s * s
    d = nu * ((0.5 * np.abs(det)) * q)
    return d[ok]


def loads(X, T, edges, u, p, p2, nu, center=(0.5, 0.5)):
    """The ten values by exact summation (math.fsum) of the terms, and per value the sum of the terms' magnitudes."""
    e8, length = edge_terms(X, T, edges, u, p, p2, nu, center)
    d = dissipation_terms(X, T, u, nu)
    cols = [e8[:, q] for q in range(8)] + [d, length]
    return (np.array([math.fsum(c) for c in cols]), np.array([math.fsum(np.abs(c)) for c in cols]))


def polygon_area(X, edges, center=(0.5, 0.5)):
    """The shoelace area of the surface polygon (the edges taken counter-clockwise about the centre)."""
    _, i, j, _ = edges
    xi, yi = X[i, 0] - center[0], X[i, 1] - center[1]
    xj, yj = X[j, 0] - center[0], X[j, 1] - center[1]
    cr = xi * yj - xj * yi
    return 0.5 * math.fsum(np.abs(cr))
