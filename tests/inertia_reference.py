"""The oracle of a step with inertia (helper of tests/test_inertia_host.py and tests/test_gpu_inertia.py).

StokesRef.step(u, c) uses its u only as the right-hand side of the viscous solve (oracle/fem_ref.py:586-587, the
reference's u + DT * 0 placeholder, StokesColor.py:540-547).  Stam's splitting puts the semi-Lagrangian advection of
the velocity by itself in front of it, so the inertial step is a composition of two oracle functions and needs no
reference code of its own:

    ua[:, k] = sl_advect(u[:, k], u, dt, X, T, tree)[0]    k = 0, 1
    out      = ref.step(ua, c)
"""
import numpy as np

import oracle as O


def advect_velocity(ref, u):
    """(u_a, not-found mask): each component of u advected by u with oracle.sl_advect (advect_semilagrange)."""
    ua = np.empty_like(u)
    nf = None
    for k in range(2):
        ua[:, k], nfk = O.sl_advect(np.ascontiguousarray(u[:, k]), u, ref.dt, ref.X, ref.T, ref.tree)
        assert nf is None or np.array_equal(nf, nfk)  # (the locate does not depend on the field)
        nf = nfk
    return ua, nf


def inertial_step(ref, u, c=None, tracers=None, status=None):
    """One step of StokesRef with the inertial term: ref.step's dict, with "u_adv" (the viscous solve's right-hand
    side) and "adv_notfound" (the rows of u_a that kept their value) added."""
    ua, nf = advect_velocity(ref, u)
    out = ref.step(ua, c, tracers, status)
    out["u_adv"] = ua
    out["adv_notfound"] = nf
    return out
