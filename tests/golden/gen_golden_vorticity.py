#!/usr/bin/env python3
"""Generate tests/golden/golden_vorticity.npz by RUNNING the reference's calculate_vorticity
(scripts/good_visualization2.py:310-345) on the goldens' velocity fields.

It reuses gen_golden.py's AST harness (``_extract``: the reference script's ``def`` nodes executed in a fresh
namespace) and, like it, runs only where the reference is checked out.  The output is data only: for each of the
meshes ``mesh1`` and ``fine`` the nodal vorticity of ``u_rand``, ``u_swirl`` and ``color_s2_u`` from
golden_<mesh>.npz, under the keys ``<mesh>_vort_rand``, ``<mesh>_vort_swirl`` and ``<mesh>_vort_color_s2``.

Run:  python tests/golden/gen_golden_vorticity.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402

FIELDS = {"rand": "u_rand", "swirl": "u_swirl", "color_s2": "color_s2_u"}


def main():
    G._install_stubs()
    V = G._extract("scripts/good_visualization2.py")
    out = {}
    for mesh in ("mesh1", "fine"):
        g = np.load(os.path.join(G.OUT, f"golden_{mesh}.npz"))
        X, T = g["coords64"], g["tris"]
        for tag, key in FIELDS.items():
            out[f"{mesh}_vort_{tag}"] = V["calculate_vorticity"](X, T, g[key])
    path = os.path.join(G.OUT, "golden_vorticity.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", sorted(out))


if __name__ == "__main__":
    main()
