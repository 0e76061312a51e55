"""The numpy restatement of a time-dependent stroke (helper of tests/test_stroke_host.py, tests/test_gpu_stroke.py and
tests/test_gpu_ens_stroke.py).

The oracle's StokesRef holds the squirmer's boundary values in ref.inner_vals and reads them only in its bc()
(oracle/fem_ref.py); the viscous matrix has its Dirichlet rows and columns zeroed.  So a stroked step needs no oracle
code of its own:

    ref.inner_vals = stroke_values(X, ref.inner, center, table, k, start)
    out            = ref.step(u, c)          (or forced_step of tests/force_reference.py with inertia or a force)

Every product and sum is a numpy line of its own, in the order include/pucfem.h fixes: the device holds the same bits.
"""
import numpy as np

from force_reference import forced_step


def stroke_row(table, k, start=0):
    """The table row the k-th step (k = 0 the first) imposes."""
    return (start + k) % len(table)


def stroke_values(X, inner, center, table, k, start=0):
    """(len(inner), 2) the values step k of the stroke imposes at the nodes `inner`: the shapes sin((j + 1) theta) and
    the direction (-sin theta, cos theta) formed as squirmer_values / oracle.squirmer_bc form them."""
    table = np.asarray(table, dtype=np.float64)
    a = table[stroke_row(table, k, start)]
    rx = X[inner, 0] - center[0]
    ry = X[inner, 1] - center[1]
    th = np.arctan2(ry, rx)
    vt = a[0] * np.sin(th)
    for j in range(1, table.shape[1]):
        s = np.sin((j + 1) * th)
        p = a[j] * s
        vt = vt + p
    dx = -np.sin(th)
    dy = np.cos(th)
    vx = vt * dx
    vy = vt * dy
    return np.stack([vx, vy], 1)


def stroked_step(ref, u, c=None, table=None, k=0, start=0, center=(0.5, 0.5), inertia=False, F=None, tracers=None,
                 status=None):
    """One step of StokesRef under row (start + k) mod P of the stroke: ref.step's dict with "values" added.
    ref.inner_vals is put back afterwards.  With inertia or a uniform force F the step is forced_step's."""
    keep = ref.inner_vals
    vals = stroke_values(ref.X, ref.inner, center, table, k, start)
    ref.inner_vals = vals
    try:
        if inertia or F is not None:
            out = forced_step(ref, u, c, F=F, inertia=inertia, tracers=tracers, status=status)
        else:
            out = ref.step(u, c, tracers, status)
    finally:
        ref.inner_vals = keep
    out["values"] = vals
    return out
