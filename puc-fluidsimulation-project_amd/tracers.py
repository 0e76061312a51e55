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


def seed_map(values, density, squirmer_radius=0.25, center=(0.5, 0.5), fill=np.nan):
    """Any per-tracer array of a tracer_init(density=density) cloud back on its density x density seed grid: a float
    array (density, density) + values.shape[1:], row j the seeds at y = yy[j] and column i those at x = xx[i]
    (tracer_init's order), `fill` where the seed was dropped (inside the swimmer)."""
    v = np.asarray(values, dtype=np.float64)
    _, keep = _seed_grid(squirmer_radius, center, density, 1.0, 1.0)
    if v.ndim == 0 or v.shape[0] != int(keep.sum()):
        raise ValueError(f"{v.shape[0] if v.ndim else 1} values for the {int(keep.sum())} seeds "
                         f"tracer_init(density={density}) keeps")
    out = np.full((density * density,) + v.shape[1:], fill, dtype=np.float64)
    out[keep] = v
    return out.reshape((density, density) + v.shape[1:])


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


def stretch(F):
    """(lam, det, integrand) per tracer of the deformation gradients F (..., 2, 2) or (..., 4): the larger eigenvalue
    lam of the Cauchy-Green tensor F^T F (the squared stretching factor of the most stretched material line), det F
    (<= 0: the discrete flow map folded there) and the FTLE integrand 0.5 * log(lam) -- with the formulas of
    pucfem_tracer_stretch_info, every product and sum as written there.  NaN rows stay NaN."""
    F = np.asarray(F, dtype=np.float64)
    if F.shape[-2:] == (2, 2):
        F = F.reshape(F.shape[:-2] + (4,))
    if F.shape[-1] != 4:
        raise ValueError(f"F must be (..., 2, 2) or (..., 4), got {F.shape}")
    F00, F01, F10, F11 = F[..., 0], F[..., 1], F[..., 2], F[..., 3]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        C00 = F00 * F00 + F10 * F10
        C01 = F00 * F01 + F10 * F11
        C11 = F01 * F01 + F11 * F11
        lam = 0.5 * ((C00 + C11) + np.sqrt((C00 - C11) * (C00 - C11) + 4.0 * (C01 * C01)))
        det = F00 * F11 - F01 * F10
        integrand = 0.5 * np.log(lam)
    return lam, det, integrand


def ftle(F, T):
    """The finite-time Lyapunov exponent per tracer, log(lam) / (2 T), of the deformation gradients F over the
    elapsed time T (steps x dt of the steps taken with stretching on)."""
    T = float(T)
    if not T > 0.0:
        raise ValueError("T must be positive")
    return stretch(F)[2] / T
