"""ctypes binding of libpucfem.so (include/pucfem.h).

The library is built in-tree (``python -c "import __graft_entry__ as g; g.build()"``) and loaded
from this package directory.  There is no fallback: if the shared object is missing or a call
fails, a ``PucfemError`` is raised.
"""
from __future__ import annotations

import ctypes as ct
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBNAME = "libpucfem.so"

# enums (pucfem.h)
STOKES_COLOR, STOKES_FOOD, HEAT, POISSON = 0, 1, 2, 3
F_U, F_USTAR, F_P, F_P2, F_DIV_STAR, F_DIV_U, F_FINAL_DIV, F_C, F_SCALAR, F_TRACERS, F_STATUS = range(11)
F_CAPTURE_STEP = 11
F_VORTICITY = 12
F_DYES = 13  # all dye channels (K, N); channel k is field F_DYE0 + k
F_DYE0 = 64
F_U_ADV = 14  # u_a (N, 2) of the last inertial step, read only
F_FORCE = 15  # the total body force f (N, 2) of the current state, read only
F_U_RHS = 16  # r (N, 2) of the last forced step, read only
F_DEFGRAD = 17  # the tracers' deformation gradient (n_tr, 4) while pucfem_set_tracer_stretch is on
# pucfem_tracer_stretch_info: the eight values, in order
STRETCH_KEYS = ("on", "steps", "finite", "folded", "lam_max", "lam_min", "sum_log", "terms")
FORCE_UNIFORM, FORCE_NODAL, FORCE_BUOYANCY = 1, 2, 4  # pucfem_force_info: the terms present (a mask)
MAX_DYES = 16
STROKE_MAX_MODES, STROKE_MAX_PERIOD = 8, 65536  # pucfem_set_stroke: K and P at the most
# pucfem_swimmer_loads: the ten reduced values, in order; the first eight are also pucfem_surface_traction's columns
LOADS_KEYS = ("force_pressure_x", "force_pressure_y", "force_viscous_x", "force_viscous_y", "torque_pressure",
              "torque_viscous", "power_pressure", "power_viscous", "dissipation", "perimeter")
ADV_DYE, ADV_VELOCITY = 1, 2  # pucfem_set_advection: what (a mask)
ADV_SL, ADV_MACCORMACK = 0, 1  # ... and the scheme
MC_NO_BACK, MC_NO_FWD = 1, 2  # marks of pucfem_sl_advect_mc
TRJ_DYE, TRJ_VELOCITY, TRJ_TRACERS = 1, 2, 4  # pucfem_set_trajectory: what (a mask)
TRJ_EULER, TRJ_MIDPOINT = 1, 2  # ... and the order
TRJ_NO_MID1, TRJ_NO_MID2 = 4, 8  # marks of pucfem_sl_advect_traj beside MC_NO_BACK / MC_NO_FWD
OP_K, OP_VISC, OP_PRES, OP_GX, OP_GY, OP_DIV, OP_GRAD, OP_LIT, OP_MCONS, OP_MLUMP, OP_ASUM = range(11)
OP_CURL = 11
SLN_UNIT, SLN_EULER, SLN_BOTH = 1, 2, 4  # pucfem_streamline_flag
SLN_COMPLETE, SLN_LEFT, SLN_STAGNANT, SLN_SEED_OUTSIDE = range(4)  # pucfem_streamline_status
HOST_ONLY = -1
ERRORS = {-1: "EINVAL", -2: "EHIP", -3: "ENOCONV", -4: "ESTATE", -5: "ENCCL", -6: "ENOMEM", -7: "ENODEV"}


class PucfemError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"pucfem {ERRORS.get(code, code)}: {msg}")
        self.code = code


class Params(ct.Structure):
    _fields_ = [
        ("scheme", ct.c_int32), ("nstrips", ct.c_int32), ("dt", ct.c_double), ("nu", ct.c_double),
        ("rtol_visc", ct.c_double), ("rtol_pres", ct.c_double), ("rtol_lin", ct.c_double),
        ("maxit_visc", ct.c_int32), ("maxit_pres", ct.c_int32), ("maxit_lin", ct.c_int32),
        ("warm_start", ct.c_int32), ("sl_k", ct.c_int32), ("capture_radius", ct.c_double),
        ("center_x", ct.c_double), ("center_y", ct.c_double), ("precond", ct.c_int32),
        ("mg_degree", ct.c_int32), ("mg_ratio", ct.c_double), ("mg_post", ct.c_int32),
        ("mg_single", ct.c_int32), ("mg_rep_nodes", ct.c_int64), ("mg_f32_vals", ct.c_int32),
        ("idx32", ct.c_int32), ("proj_k", ct.c_int32), ("proj_k_visc", ct.c_int32), ("mg_kind", ct.c_int32),
        ("solver_path", ct.c_int32), ("assembled", ct.c_int32), ("dye_scheme", ct.c_int32),
        ("dye_diffusivity", ct.c_double), ("assembly", ct.c_int32), ("proj_shared", ct.c_int32),
    ]


class StepStats(ct.Structure):
    _fields_ = [
        ("max_div_star", ct.c_double), ("max_final_div", ct.c_double), ("mix_I", ct.c_double),
        ("mix_mu", ct.c_double), ("mix_var", ct.c_double), ("eaten", ct.c_int64), ("it_visc", ct.c_int32),
        ("it_p", ct.c_int32), ("it_p2", ct.c_int32), ("sl_notfound", ct.c_int32),
    ]


_P = ct.c_void_p
_D = ct.POINTER(ct.c_double)
_I32 = ct.POINTER(ct.c_int32)
_I64 = ct.POINTER(ct.c_int64)
_F = ct.POINTER(ct.c_float)
_U8 = ct.POINTER(ct.c_uint8)

SIGNATURES = {
    "pucfem_abi_version": ([], ct.c_int),
    "pucfem_last_error": ([_P], ct.c_char_p),
    "pucfem_device_count": ([_I32], ct.c_int),
    "pucfem_ctx_create": ([ct.c_int32, ct.POINTER(_P)], ct.c_int),
    "pucfem_rccl_unique_id": ([_U8], ct.c_int),
    "pucfem_ctx_create_dist": ([ct.c_int32, ct.c_int32, ct.c_int32, _U8, ct.POINTER(_P)], ct.c_int),
    "pucfem_ctx_destroy": ([_P], ct.c_int),
    "pucfem_mesh_upload": ([_P, ct.c_int64, _D, _I32, ct.c_int64, _I32, ct.c_int32], ct.c_int),
    "pucfem_set_pairs": ([_P, ct.c_int32, ct.c_int64, _I64], ct.c_int),
    "pucfem_set_dirichlet": ([_P, ct.c_int64, _I32, _D, ct.c_int32], ct.c_int),
    "pucfem_set_source": ([_P, ct.c_int64, _F], ct.c_int),
    "pucfem_set_hierarchy": ([_P, ct.c_int64, _D, _I32, ct.c_int64, _I32, ct.c_int32], ct.c_int),
    "pucfem_build_operators": ([_P, ct.POINTER(Params)], ct.c_int),
    "pucfem_set_field": ([_P, ct.c_int32, _D, ct.c_int64], ct.c_int),
    "pucfem_get_field": ([_P, ct.c_int32, _D, ct.c_int64], ct.c_int),
    "pucfem_step": ([_P, ct.c_int32, ct.POINTER(StepStats)], ct.c_int),
    "pucfem_ens_create": ([_P, ct.c_int32, _D], ct.c_int),
    "pucfem_ens_destroy": ([_P], ct.c_int),
    "pucfem_ens_set_field": ([_P, ct.c_int32, ct.c_int32, _D, ct.c_int64], ct.c_int),
    "pucfem_ens_get_field": ([_P, ct.c_int32, ct.c_int32, _D, ct.c_int64], ct.c_int),
    "pucfem_ens_step": ([_P, ct.c_int32, ct.POINTER(StepStats)], ct.c_int),
    "pucfem_ens_info": ([_P, _I64], ct.c_int),
    "pucfem_sample_points": ([_P, ct.c_int32, _I32, ct.c_int64, _D, _D, _I32], ct.c_int),
    "pucfem_raster": ([_P, ct.c_int32, _I32, ct.c_int32, ct.c_int32, _D, _F], ct.c_int),
    "pucfem_ens_raster": ([_P, ct.c_int32, _I32, ct.c_int32, ct.c_int32, ct.c_int32, _D, _F], ct.c_int),
    "pucfem_raster_probe": ([_P, ct.c_int32, _I32, ct.c_int32, ct.c_int32, _D, ct.c_int32, _D], ct.c_int),
    "pucfem_streamlines": ([_P, ct.c_int64, _D, ct.c_double, ct.c_int32, ct.c_int32, ct.c_double, ct.c_int32, _I32, _D,
                            _I32, _I32, _D], ct.c_int),
    "pucfem_streamlines_probe": ([_P, ct.c_int64, _D, ct.c_double, ct.c_int32, ct.c_int32, ct.c_double, ct.c_int32, _D],
                                 ct.c_int),
    "pucfem_ens_streamlines": ([_P, ct.c_int32, ct.c_int64, _D, ct.c_double, ct.c_int32, ct.c_int32, ct.c_double, _D,
                                _I32, _I32], ct.c_int),
    "pucfem_flow_info": ([_P, ct.c_int32, _D], ct.c_int),
    "pucfem_apply": ([_P, ct.c_int32, _D, _D], ct.c_int),
    "pucfem_solve": ([_P, ct.c_int32, _D, _D, ct.c_double, ct.c_int32, _I32], ct.c_int),
    "pucfem_sl_advect": ([_P, _D, _D, ct.c_double, _D, _I32], ct.c_int),
    "pucfem_sl_advect_multi": ([_P, ct.c_int32, _D, _D, ct.c_double, _D, _I32], ct.c_int),
    "pucfem_dyes_info": ([_P, _I64], ct.c_int),
    "pucfem_dyes_mixing": ([_P, _D], ct.c_int),
    "pucfem_dyes_probe": ([_P, ct.c_int32, ct.c_int32, _D], ct.c_int),
    "pucfem_set_inertia": ([_P, ct.c_int32], ct.c_int),
    "pucfem_inertia_info": ([_P, _I64], ct.c_int),
    "pucfem_sl_advect_vel": ([_P, _D, _D, ct.c_double, _D, _I32], ct.c_int),
    "pucfem_inertia_probe": ([_P, ct.c_int32, _D], ct.c_int),
    "pucfem_ens_set_inertia": ([_P, ct.c_int32, ct.c_int32], ct.c_int),
    "pucfem_ens_inertia_info": ([_P, ct.c_int32, _I64], ct.c_int),
    "pucfem_set_force": ([_P, _D, _D], ct.c_int),
    "pucfem_set_buoyancy": ([_P, _D, ct.c_int32, _I32, _D, _D], ct.c_int),
    "pucfem_ens_set_force": ([_P, ct.c_int32, _D, _D], ct.c_int),
    "pucfem_ens_set_buoyancy": ([_P, ct.c_int32, _D, ct.c_double, ct.c_double], ct.c_int),
    "pucfem_force_info": ([_P, ct.c_int32, _I64], ct.c_int),
    "pucfem_force_apply": ([_P, _D, ct.c_double, _D], ct.c_int),
    "pucfem_force_probe": ([_P, ct.c_int32, _D], ct.c_int),
    "pucfem_set_stroke": ([_P, ct.c_int32, ct.c_int32, _D, ct.c_int32, _I32, _D, _D, ct.c_int64], ct.c_int),
    "pucfem_ens_set_stroke": ([_P, ct.c_int32, ct.c_int32, ct.c_int32, _D, ct.c_int32, _I32, _D, _D, ct.c_int64],
                              ct.c_int),
    "pucfem_stroke_info": ([_P, ct.c_int32, _I64], ct.c_int),
    "pucfem_get_dirichlet": ([_P, ct.c_int32, _D], ct.c_int),
    "pucfem_stroke_apply": ([_P, ct.c_int32, ct.c_int64, _D], ct.c_int),
    "pucfem_stroke_probe": ([_P, ct.c_int32, _D], ct.c_int),
    "pucfem_set_tracer_diffusion":([_P, ct.c_double, ct.c_uint64], ct.c_int),
    "pucfem_ens_set_tracer_diffusion": ([_P, ct.c_int32, ct.c_double, ct.c_uint64], ct.c_int),
    "pucfem_get_tracer_diffusion": ([_P, ct.c_int32, _D, ct.POINTER(ct.c_uint64)], ct.c_int),
    "pucfem_tracer_probe": ([_P, ct.c_double, ct.c_int32, _D], ct.c_int),
    "pucfem_set_tracer_stretch": ([_P, ct.c_int32], ct.c_int),
    "pucfem_ens_set_tracer_stretch": ([_P, ct.c_int32, ct.c_int32], ct.c_int),
    "pucfem_tracer_stretch_info": ([_P, ct.c_int32, _D], ct.c_int),
    "pucfem_set_advection": ([_P, ct.c_int32, ct.c_int32], ct.c_int),
    "pucfem_advection_info": ([_P, _I64], ct.c_int),
    "pucfem_sl_advect_mc": ([_P, ct.c_int32, _D, _D, ct.c_double, _D, _I32, _I32], ct.c_int),
    "pucfem_sl_advect_vel_mc": ([_P, _D, _D, ct.c_double, _D, _I32, _I32], ct.c_int),
    "pucfem_advection_probe": ([_P, ct.c_int32, ct.c_int32, ct.c_int32, _D], ct.c_int),
    "pucfem_set_trajectory": ([_P, ct.c_int32, ct.c_int32], ct.c_int),
    "pucfem_trajectory_info": ([_P, _I64], ct.c_int),
    "pucfem_sl_advect_traj": ([_P, ct.c_int32, ct.c_int32, ct.c_int32, _D, _D, ct.c_double, _D, _I32, _I32], ct.c_int),
    "pucfem_sl_advect_vel_traj": ([_P, ct.c_int32, ct.c_int32, _D, _D, ct.c_double, _D, _I32, _I32], ct.c_int),
    "pucfem_trajectory_probe": ([_P, ct.c_int32, ct.c_int32, ct.c_int32, ct.c_int32, _D], ct.c_int),
    "pucfem_ens_set_advection": ([_P, ct.c_int32, ct.c_int32, ct.c_int32], ct.c_int),
    "pucfem_ens_advection_info": ([_P, ct.c_int32, _I64], ct.c_int),
    "pucfem_ens_set_trajectory": ([_P, ct.c_int32, ct.c_int32, ct.c_int32], ct.c_int),
    "pucfem_ens_trajectory_info": ([_P, ct.c_int32, _I64], ct.c_int),
    "pucfem_ens_set_dyes": ([_P, ct.c_int32, _D], ct.c_int),
    "pucfem_ens_dyes_info": ([_P, ct.c_int32, _I64], ct.c_int),
    "pucfem_ens_dyes_mixing": ([_P, ct.c_int32, _D], ct.c_int),
    "pucfem_apply_bc": ([_P, ct.c_int32, _D], ct.c_int),
    "pucfem_dye_step": ([_P, _D, _D, _D, _I32], ct.c_int),
    "pucfem_comm_info": ([_P, ct.POINTER(ct.c_int64)], ct.c_int),
    "pucfem_visc_interval": ([_P, ct.POINTER(ct.c_double)], ct.c_int),
    "pucfem_mg_lmax": ([_P, ct.c_int32, _D], ct.c_int),
    "pucfem_mg_probe": ([_P, ct.c_int32, ct.c_int32, _D, _D, _D, _D], ct.c_int),
    "pucfem_proj_info": ([_P, _D], ct.c_int),
    "pucfem_tracer_step": ([_P, _D, ct.c_double, ct.c_int32], ct.c_int),
    "pucfem_tracer_info": ([_P, ct.c_int32, _I64], ct.c_int),
    "pucfem_mixing_index": ([_P, _D, _D], ct.c_int),
    "pucfem_mixing_index_w": ([_P, _D, _D, _D], ct.c_int),
    "pucfem_comm_selftest": ([_P, _D], ct.c_int),
    "pucfem_cgcg_coef_probe": ([_P, _D, ct.c_double, _D, ct.c_double, ct.c_int32, ct.c_int32, ct.c_double, _I32, _D],
                               ct.c_int),
    "pucfem_timing_enable": ([_P, ct.c_int32], ct.c_int),
    "pucfem_timing_get": ([_P, ct.c_int32, _D, _I64, _D], ct.c_int),
    "pucfem_counters": ([_P, _I64, _D], ct.c_int),
    "pucfem_class_counters": ([_P, ct.c_int32, _I64, _D], ct.c_int),
    "pucfem_comm_counters": ([_P, _I64], ct.c_int),
    "pucfem_sync": ([_P], ct.c_int),
    "pucfem_bench_dir": ([_P, ct.c_int32, ct.c_int32, ct.c_int32, _D], ct.c_int),
    "pucfem_bench_kernel": ([_P, ct.c_int32, ct.c_int32, _D, _D, _D], ct.c_int),
    "pucfem_proj_probe": ([_P, ct.c_int32, _D], ct.c_int),
    "pucfem_info": ([_P, _I64], ct.c_int),
    "pucfem_path_info": ([_P, _I64], ct.c_int),
    "pucfem_refine": ([ct.c_int64, _D, _I32, ct.c_int64, _I32, ct.c_int32, _I64, _I64, _D, _I32, _I32], ct.c_int),
    "pucfem_host_get_csr": ([_P, ct.c_int32, _I64, _I64, _I64, _I64, _D], ct.c_int),
    "pucfem_host_lattice_apply": ([_P, ct.c_int32, ct.c_int32, _D, _D], ct.c_int),
    "pucfem_host_partition": ([_P, ct.c_int32, ct.c_int32, _I64, _I64, _I64, _I64, _I32, _I64, _I64, _I32], ct.c_int),
    "pucfem_host_surface_edges": ([_P, _I64, _I32, _I32, _I32, _I32], ct.c_int),
    "pucfem_swimmer_loads": ([_P, ct.c_int32, _D], ct.c_int),
    "pucfem_surface_traction": ([_P, ct.c_int32, _D], ct.c_int),
    "pucfem_loads_apply": ([_P, _D, _D, _D, _D], ct.c_int),
    "pucfem_set_loads_record": ([_P, ct.c_int32], ct.c_int),
    "pucfem_loads_record": ([_P, ct.c_int32, ct.c_int64, ct.c_int64, _D], ct.c_int),
    "pucfem_loads_info": ([_P, ct.c_int32, _I64], ct.c_int),
    "pucfem_loads_probe": ([_P, ct.c_int32, _D], ct.c_int),
}

_lib = None


def lib_path():
    # PUCFEM_LIB_VARIANT=v loads libpucfem.v.so from the same directory (A/B builds of the measurement
    # tools; the default is the library __graft_entry__.build() makes)
    v = os.environ.get("PUCFEM_LIB_VARIANT")
    if v:
        if os.path.basename(v) != v:
            raise PucfemError(-1, "PUCFEM_LIB_VARIANT is a bare variant name")
        return os.path.join(HERE, f"libpucfem.{v}.so")
    return os.path.join(HERE, LIBNAME)


def lib():
    """Load libpucfem.so from the package directory (raises if it has not been built)."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise PucfemError(-7, f"{path} not built: run __graft_entry__.build()")
        L = ct.CDLL(path)
        for name, (args, res) in SIGNATURES.items():
            f = getattr(L, name)
            f.argtypes = args
            f.restype = res
        _lib = L
    return _lib


def check(rc, ctx=None):
    if rc != 0:
        msg = lib().pucfem_last_error(ctx)
        raise PucfemError(rc, msg.decode() if msg else "")


def dptr(a):
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(_D)


def iptr(a):
    assert a.dtype == np.int32 and a.flags.c_contiguous
    return a.ctypes.data_as(_I32)


def lptr(a):
    assert a.dtype == np.int64 and a.flags.c_contiguous
    return a.ctypes.data_as(_I64)


def fptr(a):
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(_F)


def device_count():
    n = ct.c_int32(0)
    rc = lib().pucfem_device_count(ct.byref(n))
    return n.value if rc == 0 else 0
