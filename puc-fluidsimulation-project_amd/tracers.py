"""Passive tracer ("food") seeding of StokesFood.py:420-436, and the capture-time map of a seeded cloud."""
from __future__ import annotations

import numpy as np

# Tracer sets of at least this many tracers step one tracer per thread on a grid, smaller ones in one block
# (TRACER_CLOUD_MIN in csrc/pucfem_kernels_impl.hpp; a tuning constant: both forms give the same bits)
CLOUD_MIN = 512


def _seed_grid(squirmer_radius, center, density, L, H):
    xx = np.linspace(0.05, L - 0.05, density)
    yy = np.linspace(0.05, H - 0.05, density)
    gx, gy = np.meshgrid(xx, yy)
    pts = np.vstack([gx.ravel(), gy.ravel()]).T
    d = np.linalg.norm(pts - np.asarray(center, dtype=np.float64), axis=1)
    return pts, d > squirmer_radius


def tracer_init(squirmer_radius=0.25, center=(0.5, 0.5), density=25, L=1.0, H=1.0):
    """25x25 grid on [0.05, 0.95]^2 minus the points with |x - c| <= R (StokesFood.py:421-429)."""
    pts, keep = _seed_grid(squirmer_radius, center, density, L, H)
    return np.ascontiguousarray(pts[keep])


def capture_map(capture_step, density, squirmer_radius=0.25, center=(0.5, 0.5)):
    """The capture steps of a tracer_init(density=density) cloud back on its density x density seed grid: a float
    (density, density) array, row j the seeds at y = yy[j] and column i those at x = xx[i] (tracer_init's order),
    holding the step in which the tracer seeded there was eaten and NaN where the seed was dropped (inside the
    swimmer) or the tracer was never captured (capture step -1): the "when was it eaten" image of a food run."""
    cs = np.asarray(capture_step).reshape(-1)
    _, keep = _seed_grid(squirmer_radius, center, density, 1.0, 1.0)
    if cs.shape[0] != int(keep.sum()):
        raise ValueError(f"{cs.shape[0]} capture steps for the {int(keep.sum())} seeds tracer_init(density={density}) "
                         "keeps")
    out = np.full(density * density, np.nan)
    out[keep] = np.where(cs >= 0, cs, np.nan)
    return out.reshape(density, density)
