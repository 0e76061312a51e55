"""pucfem-mi355x: the MI355X (gfx950) hot path of TobiasHoffmannP/PUC-Fluidsimulation-Project.

Host side: Python (this package) -> ctypes -> libpucfem.so (C ABI, include/pucfem.h) -> HIP
kernels for CDNA4.  Entry points mirror the reference (code/StokesColor.py, StokesFood.py,
poisson.py, heatEq.py): the mesh loaders readNode / readEle / readPoly, the reference-named
operators, and ``solve(mesh, bc, dt, steps, scheme)``.

The directory name contains hyphens, so import it with
``importlib.import_module("puc-fluidsimulation-project_amd")``.
"""
from ._lib import PucfemError, device_count, lib as _load_library  # noqa: F401
from .mesh import (Mesh, boundary_sets, filter_wall_pairs, find_boundary_pairs, load_mesh, readEle,  # noqa: F401
                   readNode, readPoly, writeEle, writeNode, writePoly)
from .ops import (advect_maccormack, advect_maccormack_vector, advect_semilagrange, advect_semilagrange_multi, advect_semilagrange_vector, apply_body_force, buildLumpedMassMatrix,  # noqa: F401
                  buildStiffnessMatrix, calculate_divergence, build_mass_and_convection_mass, calculate_gradiant,
                  calculate_vorticity, dye_implicit_step,
                  makeDirBCU, makePerBCU, mixing_index, set_globals, solve_pressure, solve_viscous, surface_edges,
                  swimmer_loads)
from .solver import (LOADS_KEYS, SAMPLE_FIELDS, Buoyancy, Context, HeatSimulation, Result, SquirmerBC, StokesEnsemble,  # noqa: F401
                     StokesSimulation, Streamlines, Stroke, Tolerances, dye_patterns, ensemble_dirichlet_values,
                     pixel_centres, poisson_solve, solve, solve_ensemble, squirmer_values, streamline_segments,
                     stroke_geometry)
from .frames import FrameRecorder, load_npz, render, save_npz, write_vtk  # noqa: F401
from .tracers import capture_map, ftle, seed_map, stretch, tracer_init  # noqa: F401

__version__ = "0.1.0"
