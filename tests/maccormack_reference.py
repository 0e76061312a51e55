"""The oracle of MacCormack advection (helper of tests/test_maccormack_host.py and tests/test_gpu_maccormack.py).

Selle et al.'s limited MacCormack step is two first-order advections and a clamp, so it is a composition of oracle
functions and needs no reference code of its own:

    ch, nf1 = sl_advect(c,  u, +dt)          T1 = the triangle that advection interpolated in
    cb, nf2 = sl_advect(ch, u, -dt)
    out = c                                   where nf1            (mark bit 0)
          ch                                  where nf2            (mark bit 1; bit 0 decides the value)
          clamp(ch + 0.5 * (c - cb), min / max of c at T1's vertices)   elsewhere

oracle.sl_advect does not return its triangle, so T1 is restated here (locate): the k = 10 nearest centroids, the
first whose weights are all >= 0.  "First" has two readings that differ only where several triangles pass, i.e. at a
departure point on a mesh node or edge (zero velocity: the walls): the KDTree's own order (rule "tree", what
sl_advect does) and the (d^2, id) order the device uses (rule "key").  Both are here; the GPU tests take T1 from the
device and verify it instead of assuming either.
"""
import numpy as np

import oracle as O

NO_BACK, NO_FWD = 1, 2


def departure(u, dt, X):
    """oracle.sl_advect's back-traced points (fem_ref.py:422-425)."""
    xb = np.remainder(X[:, 0] - dt * u[:, 0] * 1.0, 1.0)
    yb = X[:, 1] - dt * u[:, 1] * 1.0
    yb = np.where(yb < 0.0, 1e-12, yb)
    yb = np.where(yb > 1.0, 1.0 - 1e-12, yb)
    return xb, yb


def weight_test(X, tri3, xq, yq):
    """The reference's weight test (fem_ref.py:437-444) of the points (xq, yq) in the triangles tri3 (n, 3)."""
    i, j, l_ = tri3[:, 0], tri3[:, 1], tri3[:, 2]
    x1, y1, x2, y2, x3, y3 = X[i, 0], X[i, 1], X[j, 0], X[j, 1], X[l_, 0], X[l_, 1]
    det = (x2 - x1) * (y3 - y1) - (x3 - x1) * (y2 - y1)
    okd = np.abs(det) >= 1e-14
    sd = np.where(okd, det, 1.0)
    w1 = ((x2 - xq) * (y3 - yq) - (x3 - xq) * (y2 - yq)) / sd
    w2 = ((x3 - xq) * (y1 - yq) - (x1 - xq) * (y3 - yq)) / sd
    w3 = 1.0 - w1 - w2
    return okd & (w1 >= 0.0) & (w2 >= 0.0) & (w3 >= 0.0)


def interpolate(X, tri3, xq, yq, c):
    """The reference's interpolation with periodic x differences (fem_ref.py:449-464) of c in the triangles tri3."""
    def dx(a, b):
        d = a - b
        d = np.where(d > 0.5, d - 1.0, d)
        return np.where(d < -0.5, d + 1.0, d)

    i, j, l_ = tri3[:, 0], tri3[:, 1], tri3[:, 2]
    x1, y1, x2, y2, x3, y3 = X[i, 0], X[i, 1], X[j, 0], X[j, 1], X[l_, 0], X[l_, 1]
    det = dx(x2, x1) * (y3 - y1) - dx(x3, x1) * (y2 - y1)
    w1 = (dx(x2, xq) * (y3 - yq) - dx(x3, xq) * (y2 - yq)) / det
    w2 = (dx(x3, xq) * (y1 - yq) - dx(x1, xq) * (y3 - yq)) / det
    w3 = 1.0 - w1 - w2
    return w1 * c[i] + w2 * c[j] + w3 * c[l_]


def locate(u, dt, X, T, tree, k=10, rule="tree"):
    """(N,) the triangle PointLocator.find returns for every node's departure point, -1 where none of the k nearest
    centroids passes.  rule "tree": the candidates in the KDTree's order; "key": sorted by (d^2, id), d^2 the squared
    distance to the centroid (x1 + x2 + x3) / 3."""
    xb, yb = departure(u, dt, X)
    _, idx = tree.query(np.stack([xb, yb], 1), k=k)
    if rule == "key":
        cx = (X[T[:, 0], 0] + X[T[:, 1], 0] + X[T[:, 2], 0]) / 3.0
        cy = (X[T[:, 0], 1] + X[T[:, 1], 1] + X[T[:, 2], 1]) / 3.0
        ex, ey = cx[idx] - xb[:, None], cy[idx] - yb[:, None]
        d2 = ex * ex + ey * ey
        order = np.lexsort((idx, d2), axis=1)
        idx = np.take_along_axis(idx, order, axis=1)
    else:
        assert rule == "tree"
    found = -np.ones(len(X), dtype=np.int64)
    for kk in range(k):
        t = idx[:, kk]
        hit = weight_test(X, T[t], xb, yb) & (found < 0)
        found[hit] = t[hit]
    return found


def limit(c, ch, cb, t1, nf1, nf2, T):
    """The clamp formulas on given ch, cb and T1: (out, clamped mask)."""
    ok = ~nf1 & ~nf2
    tri3 = T[np.where(t1 >= 0, t1, 0)]
    fa, fb, fd = c[tri3[:, 0]], c[tri3[:, 1]], c[tri3[:, 2]]
    lo = np.where(fb < fa, fb, fa)
    lo = np.where(fd < lo, fd, lo)
    hi = np.where(fb > fa, fb, fa)
    hi = np.where(fd > hi, fd, hi)
    e = ch + 0.5 * (c - cb)
    lim = np.where(e < lo, lo, np.where(e > hi, hi, e))
    out = np.where(nf1, c, np.where(nf2, ch, lim))
    return out, ok & ((e < lo) | (e > hi))


def mc_advect(c, u, dt, X, T, tree, rule="tree"):
    """One limited MacCormack step of the nodal field c: (out, marks, T1, clamped mask)."""
    ch, nf1 = O.sl_advect(c, u, dt, X, T, tree)
    cb, nf2 = O.sl_advect(ch, u, -dt, X, T, tree)
    t1 = locate(u, dt, X, T, tree, rule=rule)
    assert np.array_equal(t1 < 0, nf1)  # (the restated locate finds a triangle exactly where sl_advect does)
    out, clamped = limit(c, ch, cb, t1, nf1, nf2, T)
    marks = nf1.astype(np.int32) * NO_BACK + nf2.astype(np.int32) * NO_FWD
    return out, marks, t1, clamped


def mc_advect_velocity(ref, u):
    """(u_a, marks, clamped (N, 2)): each component of u moved by u with mc_advect."""
    ua = np.empty_like(u)
    cl = np.zeros(u.shape, dtype=bool)
    marks = None
    for k in range(2):
        ua[:, k], mk, _, cl[:, k] = mc_advect(np.ascontiguousarray(u[:, k]), u, ref.dt, ref.X, ref.T, ref.tree)
        assert marks is None or np.array_equal(marks, mk)  # (the locates do not depend on the field)
        marks = mk
    return ua, marks, cl


def mc_inertial_step(ref, u, c=None, tracers=None, status=None, dye=False):
    """inertia_reference.inertial_step with mc_advect per component: ref.step's dict with "u_adv", "adv_marks" and
    "adv_clamped" added.  dye: c moves by mc_advect with the step's final u too ("c", "mixing", "c_marks",
    "c_clamped" replaced / added)."""
    ua, marks, cl = mc_advect_velocity(ref, u)
    out = ref.step(ua, c, tracers, status)
    out["u_adv"], out["adv_marks"], out["adv_clamped"] = ua, marks, cl
    if dye and c is not None:
        mc_dye(ref, out, c)
    return out


def mc_dye(ref, out, c):
    """Replace the first-order dye of the step record `out` (ref.step's dict) by the MacCormack step of c."""
    c2, mk, _, cl = mc_advect(c, out["u"], ref.dt, ref.X, ref.T, ref.tree)
    out["c"], out["c_marks"], out["c_clamped"] = c2, mk, cl
    out["sl_notfound"] = (mk & NO_BACK) != 0
    out["mixing"] = O.mixing_index(c2, ref.M, mask=ref.mask_inner)
    return out
