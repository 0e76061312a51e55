"""The oracle of a forced step (helper of tests/test_force_host.py and tests/test_gpu_force.py).

The reference forms the viscous right-hand side as u + DT * b_force (StokesColor.py:485-486, 540-541);
StokesRef.step(u, c) uses its u only as that right-hand side (oracle/fem_ref.py:586-587).  So a forced step is a
composition of existing oracle functions and needs no reference code of its own:

    f   = body_force(...)           the total force per node, in the order include/pucfem.h fixes
    r   = rhs(base, dt, f)          base + dt * f  (base: u, or with inertia the advected u_a)
    out = ref.step(r, c)

Every product and sum is a numpy line of its own, in the order of the definition, and absent terms are skipped (not
added as zeros): the device's r holds the same bits.
"""
import numpy as np

from inertia_reference import advect_velocity


def body_force(X, F=None, fn=None, buoy=None, fields=None):
    """(N, 2) the total force.  F: a pair or None; fn: (N, 2) or None; buoy: (g, [(name, beta, ref), ...]) or None,
    the names looked up in fields (a dict of (N,) arrays: "c", "dye0", ...)."""
    N = len(X)
    f = np.zeros((N, 2))
    if F is not None:
        f = np.tile(np.asarray(F, dtype=np.float64), (N, 1))
    if fn is not None:
        fn = np.asarray(fn, dtype=np.float64)
        f = f + fn if F is not None else fn.copy()
    if buoy is not None:
        g, terms = buoy
        name, beta, ref = terms[0]
        b = beta * (fields[name] - ref)
        for name, beta, ref in terms[1:]:
            b = b + beta * (fields[name] - ref)
        f = np.stack([f[:, 0] + g[0] * b, f[:, 1] + g[1] * b], axis=1)
    return f


def rhs(base, dt, f):
    """r = base + dt * f"""
    return base + dt * f


def forced_step(ref, u, c=None, F=None, fn=None, buoy=None, fields=None, inertia=False, tracers=None, status=None):
    """One step of StokesRef with a body force: ref.step's dict with "u_rhs" (the viscous solve's right-hand side) and
    "force" added.  fields defaults to {"c": c}."""
    base = advect_velocity(ref, u)[0] if inertia else u
    if fields is None and c is not None:
        fields = {"c": c}
    f = body_force(ref.X, F, fn, buoy, fields)
    r = rhs(base, ref.dt, f)
    out = ref.step(r, c, tracers, status)
    out["u_rhs"] = r
    out["force"] = f
    return out
