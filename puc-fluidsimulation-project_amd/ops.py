"""Reference-named entry points (StokesColor.py / poisson.py function names and signatures).

The hot-path functions (calculate_divergence, calculate_gradiant, advect_semilagrange, the two
np.linalg.solve call sites) run on the GPU through a context cached per mesh.  The assembly
functions return the C++ host-assembled operator (dense for small meshes, as the reference's
np.zeros((N, N)) matrices; scipy CSR above DENSE_MAX nodes).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .mesh import Mesh, boundary_sets
from .solver import Context, SquirmerBC, Tolerances, stokes_setup

DENSE_MAX = 8192
_cache: dict = {}


def _key(nodes, triangles):
    n = np.ascontiguousarray(nodes, dtype=np.float64)
    t = np.ascontiguousarray(triangles, dtype=np.int32)
    return (n.shape, t.shape, hash(n.tobytes()), hash(t.tobytes())), n, t


def context_for(nodes, triangles, dt=0.05, nu=0.1, bc: SquirmerBC | None = None, device=0):
    """A single-GPU Stokes context for this mesh (cached by content)."""
    (k, n, t) = _key(nodes, triangles)
    k = k + (dt, nu, None if bc is None else (bc.B1, bc.B2))
    ctx = _cache.get(k)
    if ctx is None:
        mesh = Mesh(n, np.zeros(len(n), dtype=np.int32), t)
        ctx = Context(device)
        ctx.upload(mesh)
        ctx.build("color", dt, nu, Tolerances())
        _cache[k] = ctx
    return ctx


def _stokes_context(mesh: Mesh, dt, nu, bc: SquirmerBC, device=0):
    # the Dirichlet set and values depend on the markers and the squirmer geometry, not only on the mesh
    k = ("stokes", mesh.N, mesh.T, hash(mesh.coords.tobytes()), hash(mesh.triangles.tobytes()),
         hash(np.ascontiguousarray(mesh.markers).tobytes()), dt, nu, bc.B1, bc.B2, tuple(bc.center),
         tuple(bc.outer_value), bc.capture_radius, bc.squirmer_radius)
    ctx = _cache.get(k)
    if ctx is None:
        ctx = Context(device)
        ctx.upload(mesh)
        pairs, nodes, vals = stokes_setup(mesh, bc)
        ctx.set_pairs(0, pairs)
        ctx.set_pairs(1, pairs)
        ctx.set_dirichlet(nodes, vals)
        ctx.build("color", dt, nu, Tolerances(), capture=bc.capture_radius, center=bc.center)
        _cache[k] = ctx
    return ctx


# The reference's functions read module globals (nodes_coords, triangles, pairs, B1, B2, ...,
# StokesColor.py:359,369,405-431); set_globals() plays that role for the shims that keep the
# reference's short signatures (advect_semilagrange(c, u, DT), makeDirBCU(u), makePerBCU(u)).
_globals: dict = {}


def set_globals(mesh: Mesh, bc: SquirmerBC | None = None):
    """Bind the mesh (and squirmer parameters) the reference-signature shims act on."""
    _globals.clear()
    _globals.update(mesh=mesh, bc=bc or SquirmerBC())


def _mesh_or_global(mesh):
    if mesh is None:
        mesh = _globals.get("mesh")
    if mesh is None:
        raise ValueError("no mesh: pass mesh= or call set_globals(mesh) first (the reference's module globals)")
    return mesh


def makeDirBCU(u, mesh: Mesh | None = None, bc: SquirmerBC | None = None):
    """StokesColor.py:405-427 in place on u (N,2): walls to 0, squirmer surface to the tangential
    squirmer velocity, through the device's boundary kernel."""
    mesh = _mesh_or_global(mesh)
    _apply_bc(u, mesh, bc or _globals.get("bc") or SquirmerBC(), 2)


def makePerBCU(u, mesh: Mesh | None = None, bc: SquirmerBC | None = None):
    """StokesColor.py:429-431 in place on u (N,2): u[slave] = u[master] for the filtered pairs."""
    mesh = _mesh_or_global(mesh)
    _apply_bc(u, mesh, bc or _globals.get("bc") or SquirmerBC(), 1)


def _apply_bc(u, mesh, bc, which):
    if not (isinstance(u, np.ndarray) and u.dtype == np.float64 and u.flags.c_contiguous and u.shape == (mesh.N, 2)):
        raise TypeError("u must be a C-contiguous float64 array of shape (N, 2) (modified in place)")
    ctx = _stokes_context(mesh, 0.05, bc.nu, bc)
    _lib.check(ctx.L.pucfem_apply_bc(ctx.h, which, _lib.dptr(u)), ctx.h)


def mixing_index(c, mass, mask=None, mesh: Mesh | None = None):
    """StokesColor.py:391-403: (I, mu, var) of c weighted by `mass` over `mask` (None: every node), on
    the device.  The reference's c[mask], mass[mask] becomes the node weights w = mass on the mask and 0
    elsewhere (an index mask with repeats counts a node repeatedly, a boolean mask selects), so any
    weights and mask the reference accepts are accepted here."""
    mesh = _mesh_or_global(mesh)
    c = np.ascontiguousarray(c, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    if c.shape != (mesh.N,) or mass.shape != (mesh.N,):
        raise ValueError(f"mixing_index: c and mass must have shape ({mesh.N},)")
    if mask is None:
        w = mass
    else:
        m = np.asarray(mask)
        if m.dtype == bool:
            if m.shape != (mesh.N,):
                raise ValueError(f"mixing_index: a boolean mask must have shape ({mesh.N},)")
            w = np.where(m, mass, 0.0)
        else:
            m = m.astype(np.int64).ravel()
            m = np.where(m < 0, m + mesh.N, m)  # numpy's negative indices
            if m.size and (m.min() < 0 or m.max() >= mesh.N):
                raise IndexError("mixing_index: mask index out of range")
            w = np.bincount(m, minlength=mesh.N).astype(np.float64) * mass
    ctx = _stokes_context(mesh, 0.05, 0.1, _globals.get("bc") or SquirmerBC())
    out = np.zeros(3)
    w = np.ascontiguousarray(w, dtype=np.float64)
    _lib.check(ctx.L.pucfem_mixing_index_w(ctx.h, _lib.dptr(c), _lib.dptr(w), _lib.dptr(out)), ctx.h)
    return float(out[0]), float(out[1]), float(out[2])


def calculate_divergence(nodes, triangles, u_star):
    """StokesColor.py:130-165 on the GPU: (N,) lumped nodal divergence."""
    ctx = context_for(nodes, triangles)
    return ctx.apply(_lib.OP_DIV, np.asarray(u_star, dtype=np.float64).reshape(-1, 2), (len(nodes),))


def calculate_vorticity(nodes, triangles, u):
    """scripts/good_visualization2.py:310-345 on the GPU: (N,) lumped nodal vorticity d(u_y)/dx - d(u_x)/dy."""
    ctx = context_for(nodes, triangles)
    return ctx.apply(_lib.OP_CURL, np.asarray(u, dtype=np.float64).reshape(-1, 2), (len(nodes),))


def calculate_gradiant(nodes, triangles, p_scalar):
    """StokesColor.py:224-263 on the GPU: (grad_px, grad_py)."""
    ctx = context_for(nodes, triangles)
    g = ctx.apply(_lib.OP_GRAD, np.asarray(p_scalar, dtype=np.float64), (len(nodes), 2))
    return g[:, 0].copy(), g[:, 1].copy()


def advect_semilagrange(c, u, DT, nodes=None, triangles=None):
    """StokesColor.py:347-389 on the GPU, in place on c like the reference (c[:] = c_new).
    advect_semilagrange(c, u, DT) as in the reference acts on the set_globals() mesh.
    Returns the not-found mask (nodes that kept c[n])."""
    if nodes is None or triangles is None:
        m = _mesh_or_global(None)
        nodes, triangles = m.coords, m.triangles
    ctx = context_for(nodes, triangles)
    cin = np.ascontiguousarray(c, dtype=np.float64)
    uu = np.ascontiguousarray(u, dtype=np.float64).reshape(-1, 2)
    out = np.zeros_like(cin)
    nf = np.zeros(len(cin), dtype=np.int32)
    _lib.check(ctx.L.pucfem_sl_advect(ctx.h, _lib.dptr(cin), _lib.dptr(uu), float(DT), _lib.dptr(out),
                                      _lib.iptr(nf)), ctx.h)
    c[:] = out
    return nf.astype(bool)


def _trajectory(trajectory):
    from .solver import trajectory_order

    return trajectory_order(trajectory)


def advect_semilagrange_multi(C, u, DT, nodes=None, triangles=None, trajectory="euler", marks=None):
    """advect_semilagrange of the K fields C (K, N), K = 1 .. 16, at once (pucfem_sl_advect_multi): one back-trace
    and one point location per node for all of them, every field's bits those of advect_semilagrange alone.
    In place on C like the reference (C[:] = C_new); returns the not-found mask (N,), the same for every field.
    trajectory 'euler' | 'midpoint': with 'midpoint' (pucfem_sl_advect_traj) every node is traced with the velocity
    read half a step along its straight trace; marks (N,) int32, if given, receives the row marks (bit 0 the final
    point was not found, bit 2 the midpoint was not: that node took its Euler step)."""
    order = _trajectory(trajectory)
    if nodes is None or triangles is None:
        m = _mesh_or_global(None)
        nodes, triangles = m.coords, m.triangles
    ctx = context_for(nodes, triangles)
    cin = np.ascontiguousarray(C, dtype=np.float64)
    if cin.ndim != 2 or cin.shape[1] != len(nodes):
        raise ValueError(f"advect_semilagrange_multi: C must have shape (K, {len(nodes)})")
    uu = np.ascontiguousarray(u, dtype=np.float64).reshape(-1, 2)
    out = np.zeros_like(cin)
    nf = np.zeros(cin.shape[1], dtype=np.int32)
    if order == _lib.TRJ_EULER and marks is None:
        _lib.check(ctx.L.pucfem_sl_advect_multi(ctx.h, cin.shape[0], _lib.dptr(cin), _lib.dptr(uu), float(DT),
                                                _lib.dptr(out), _lib.iptr(nf)), ctx.h)
    else:
        _lib.check(ctx.L.pucfem_sl_advect_traj(ctx.h, order, _lib.ADV_SL, cin.shape[0], _lib.dptr(cin), _lib.dptr(uu),
                                               float(DT), _lib.dptr(out), _lib.iptr(nf), None), ctx.h)
        if marks is not None:
            marks[:] = nf
        nf &= _lib.MC_NO_BACK
    C[:] = out
    return nf.astype(bool)


def advect_semilagrange_vector(f, u, DT, nodes=None, triangles=None, trajectory="euler", marks=None):
    """advect_semilagrange of the two components of f (N, 2) at once (pucfem_sl_advect_vel, the inertial step's
    kernel): one back-trace and one point location per node, each component's bits those of advect_semilagrange
    on f[:, k] alone.  f may be u (the inertial term's u_a = SL(u; u, DT)).  In place on f like the reference
    (f[:] = f_new); returns the not-found mask (N,), the same for both components.  trajectory, marks: as
    advect_semilagrange_multi (pucfem_sl_advect_vel_traj)."""
    order = _trajectory(trajectory)
    if nodes is None or triangles is None:
        m = _mesh_or_global(None)
        nodes, triangles = m.coords, m.triangles
    fin = np.ascontiguousarray(f, dtype=np.float64)
    if fin.shape != (len(nodes), 2):
        raise ValueError(f"advect_semilagrange_vector: f must have shape ({len(nodes)}, 2)")
    ctx = context_for(nodes, triangles)
    uu =np.ascontiguousarray(u, dtype=np.float64).reshape(-1, 2)
    out = np.zeros_like(fin)
    nf = np.zeros(len(fin), dtype=np.int32)
    if order == _lib.TRJ_EULER and marks is None:
        _lib.check(ctx.L.pucfem_sl_advect_vel(ctx.h, _lib.dptr(fin), _lib.dptr(uu), float(DT), _lib.dptr(out),
                                              _lib.iptr(nf)), ctx.h)
    else:
        _lib.check(ctx.L.pucfem_sl_advect_vel_traj(ctx.h, order, _lib.ADV_SL, _lib.dptr(fin), _lib.dptr(uu), float(DT),
                                                   _lib.dptr(out), _lib.iptr(nf), None), ctx.h)
        if marks is not None:
            marks[:] = nf
        nf &= _lib.MC_NO_BACK
    f[:] = out
    return nf.astype(bool)


def apply_body_force(u, dt, nodes=None, triangles=None, force=None, buoyancy=None, c=None, dyes=None):
    """The forced step's right-hand side r = u + dt * f (N, 2) (pucfem_force_apply, the step's kernel): force a pair,
    an (N, 2) field or a (pair, field) tuple; buoyancy a Buoyancy whose terms read c (N,) and dyes (K, N).  The
    products and sums in the order include/pucfem.h states, absent terms skipped.  Returns r; u is left alone."""
    from .solver import Buoyancy, _force_args

    if nodes is None or triangles is None:
        m = _mesh_or_global(None)
        nodes, triangles = m.coords, m.triangles
    N = len(nodes)
    base = np.ascontiguousarray(u, dtype=np.float64)
    if base.shape != (N, 2):
        raise ValueError(f"apply_body_force: u must have shape ({N}, 2)")
    if isinstance(force, tuple) and len(force) == 2 and np.shape(force[1]) == (N, 2):
        F, fn = force
    else:
        F, fn = _force_args(force, N)
    if buoyancy is not None and not isinstance(buoyancy, Buoyancy):
        raise ValueError("apply_body_force: buoyancy must be a Buoyancy or None")
    ctx = context_for(nodes, triangles)
    try:
        if buoyancy is not None:
            names = list(buoyancy.terms)
            if "c" in names:
                if c is None:
                    raise ValueError("apply_body_force: the buoyancy reads c")
                ctx.set_field(_lib.F_C, np.ascontiguousarray(c, dtype=np.float64).reshape(N))
            if any(n != "c" for n in names):
                if dyes is None:
                    raise ValueError("apply_body_force: the buoyancy reads dye channels: give dyes (K, N)")
                ctx.set_field(_lib.F_DYES, np.ascontiguousarray(dyes, dtype=np.float64).reshape(-1, N))
        ctx.set_force(F, fn)
        ctx.set_buoyancy(buoyancy)
        return ctx.force_apply(base, dt)
    finally:  # (the cached context serves the other operators: it keeps no force and no channels)
        ctx.set_buoyancy(None)
        ctx.set_force(None, None)
        if dyes is not None:
            ctx._c(ctx.L.pucfem_set_field(ctx.h, _lib.F_DYES, None, 0))


def advect_maccormack(c, u, DT, nodes=None, triangles=None, tri=None, trajectory="euler"):
    """One limited MacCormack step (pucfem_sl_advect_mc; Selle et al. 2008) of the field c (N,) or of the K fields
    c (K, N), K = 1 .. 16, from one point location per pass and node: ch = SL(c; u, DT), cb = SL(ch; u, -DT),
    ch + (c - cb) / 2 clamped into the range of c at the vertices of ch's departure triangle.  In place on c as
    advect_semilagrange; returns the marks (N,) int32: bit 0 the back-trace found no triangle (the node kept c),
    bit 1 the forward trace found none (it kept ch).  tri (N,) int32, if given, receives the departure triangle's
    index in `triangles` (-1: none).  trajectory 'euler' | 'midpoint': with 'midpoint' (pucfem_sl_advect_traj) both
    passes trace with the velocity read half a step along the straight trace; the marks gain bit 2 (pass 1's
    midpoint was not found) and bit 3 (pass 2's)."""
    order = _trajectory(trajectory)
    if nodes is None or triangles is None:
        m = _mesh_or_global(None)
        nodes, triangles = m.coords, m.triangles
    cin = np.ascontiguousarray(c, dtype=np.float64)
    if cin.ndim not in (1, 2) or cin.shape[-1] != len(nodes):
        raise ValueError(f"advect_maccormack: c must have shape ({len(nodes)},) or (K, {len(nodes)})")
    ctx = context_for(nodes, triangles)
    uu = np.ascontiguousarray(u, dtype=np.float64).reshape(-1, 2)
    out = np.zeros_like(cin)
    marks = np.zeros(len(nodes), dtype=np.int32)
    t = np.zeros(len(nodes), dtype=np.int32)
    if order == _lib.TRJ_EULER:
        _lib.check(ctx.L.pucfem_sl_advect_mc(ctx.h, 1 if cin.ndim == 1 else cin.shape[0], _lib.dptr(cin),
                                             _lib.dptr(uu), float(DT), _lib.dptr(out), _lib.iptr(marks), _lib.iptr(t)),
                   ctx.h)
    else:
        _lib.check(ctx.L.pucfem_sl_advect_traj(ctx.h, order, _lib.ADV_MACCORMACK, 1 if cin.ndim == 1 else cin.shape[0],
                                               _lib.dptr(cin), _lib.dptr(uu), float(DT), _lib.dptr(out),
                                               _lib.iptr(marks), _lib.iptr(t)), ctx.h)
    c[:] = out
    if tri is not None:
        tri[:] = t
    return marks


def advect_maccormack_vector(f, u, DT, nodes=None, triangles=None, tri=None, trajectory="euler"):
    """advect_maccormack of the two components of f (N, 2) at once (pucfem_sl_advect_vel_mc, the inertial step's
    kernels): each vertex's pair one load, the components limited separately, each with the bits of
    advect_maccormack on f[:, k] alone.  f may be u.  In place on f; returns the marks (N,).  trajectory: as
    advect_maccormack (pucfem_sl_advect_vel_traj)."""
    order = _trajectory(trajectory)
    if nodes is None or triangles is None:
        m = _mesh_or_global(None)
        nodes, triangles = m.coords, m.triangles
    fin = np.ascontiguousarray(f, dtype=np.float64)
    if fin.shape != (len(nodes), 2):
        raise ValueError(f"advect_maccormack_vector: f must have shape ({len(nodes)}, 2)")
    ctx = context_for(nodes, triangles)
    uu = np.ascontiguousarray(u, dtype=np.float64).reshape(-1, 2)
    out = np.zeros_like(fin)
    marks = np.zeros(len(fin), dtype=np.int32)
    t = np.zeros(len(fin), dtype=np.int32)
    if order == _lib.TRJ_EULER:
        _lib.check(ctx.L.pucfem_sl_advect_vel_mc(ctx.h, _lib.dptr(fin), _lib.dptr(uu), float(DT), _lib.dptr(out),
                                                 _lib.iptr(marks), _lib.iptr(t)), ctx.h)
    else:
        _lib.check(ctx.L.pucfem_sl_advect_vel_traj(ctx.h, order, _lib.ADV_MACCORMACK, _lib.dptr(fin), _lib.dptr(uu),
                                                   float(DT), _lib.dptr(out), _lib.iptr(marks), _lib.iptr(t)), ctx.h)
    f[:] = out
    if tri is not None:
        tri[:] = t
    return marks


def buildStiffnessMatrix(nodes, triangles, g_source=1.0):
    """StokesColor.py:98-128: (A, -B) with B = 0 (the reference never fills it)."""
    ctx = context_for(nodes, triangles)
    A = ctx.host_csr(_lib.OP_K)
    return (A.toarray() if len(nodes) <= DENSE_MAX else A), np.zeros(len(nodes))


def buildLumpedMassMatrix(nodes_coords, triangles):
    """StokesColor.py:266-284 (host setup): M_i = sum of area/3 over incident triangles."""
    X = np.asarray(nodes_coords, dtype=np.float64)
    T = np.asarray(triangles)
    x1, y1, x2, y2, x3, y3 = X[T[:, 0], 0], X[T[:, 0], 1], X[T[:, 1], 0], X[T[:, 1], 1], X[T[:, 2], 0], X[T[:, 2], 1]
    det = x1 * (y2 - y3) + x2 * (y3 - y1) + x3 * (y1 - y2)
    M = np.zeros(len(X))
    np.add.at(M, T.ravel(), np.repeat(0.5 * np.abs(det) / 3.0, 3))
    return M


def mixing_index_host(mesh: Mesh, c):
    """mixing_index (StokesColor.py:391-403) of a host field over marker==0 nodes: used once for
    the initial (I0, mu0, var0) normaliser of the printed progress (StokesColor.py:497)."""
    M = buildLumpedMassMatrix(mesh.coords, mesh.triangles)
    mask = np.where(mesh.markers == 0)[0]
    cc, mm = c[mask], M[mask]
    W = mm.sum()
    mu = (mm @ cc) / W
    var = (mm @ (cc - mu) ** 2) / W
    return var / (mu * (1 - mu) + 1e-16), mu, var


def solve_viscous(mesh: Mesh, rhs, dt=0.05, nu=0.1, bc: SquirmerBC | None = None, rtol=1e-13):
    """The np.linalg.solve(A_visc, rhs) call sites (StokesColor.py:544-545) for both components."""
    ctx = _stokes_context(mesh, dt, nu, bc or SquirmerBC(nu=nu))
    x, it = ctx.solve(_lib.OP_VISC, np.asarray(rhs, dtype=np.float64).reshape(-1, 2), rtol=rtol)
    return x


def solve_pressure(mesh: Mesh, b_p, dt=0.05, nu=0.1, bc: SquirmerBC | None = None, rtol=1e-12):
    """The np.linalg.solve(A_pressure, b_p) call sites (StokesColor.py:555, :569), restated as the
    well-posed periodic-merged system; returns the zero-mean pressure."""
    ctx = _stokes_context(mesh, dt, nu, bc or SquirmerBC(nu=nu))
    x, it = ctx.solve(_lib.OP_PRES, np.asarray(b_p, dtype=np.float64), rtol=rtol)
    return x


def _dye_context(mesh: Mesh, dt, D, device=0):
    k = ("dye", mesh.N, mesh.T, hash(mesh.coords.tobytes()), hash(mesh.triangles.tobytes()), dt, D)
    ctx = _cache.get(k)
    if ctx is None:
        bc = SquirmerBC()
        ctx = Context(device)
        ctx.upload(mesh)
        pairs, nodes, vals = stokes_setup(mesh, bc)
        ctx.set_pairs(0, pairs)
        ctx.set_pairs(1, pairs)
        ctx.set_dirichlet(nodes, vals)
        ctx.build("color", dt, bc.nu, Tolerances(dye="implicit", dye_diffusivity=D))
        _cache[k] = ctx
    return ctx


def dye_implicit_step(c, u, mesh: Mesh, dt=0.05, D=1e-3):
    """One implicit FEM dye advection-diffusion step (scripts/good_visualization.py:700-718) on the
    GPU: A = M + dt (C_u + D K) + diag(dt M_lumped div u), c <- A^-1 M c with the periodic pairs
    merged exactly (the reference's 1e10 penalty in its limit), then c[slave] = c[master].
    Returns (c_new, BiCGStab iterations)."""
    ctx = _dye_context(mesh, dt, D)
    cin = np.ascontiguousarray(c, dtype=np.float64)
    uu = np.ascontiguousarray(u, dtype=np.float64).reshape(-1, 2)
    out = np.zeros_like(cin)
    it = np.zeros(1, dtype=np.int32)
    _lib.check(ctx.L.pucfem_dye_step(ctx.h, _lib.dptr(cin), _lib.dptr(uu), _lib.dptr(out), _lib.iptr(it)), ctx.h)
    return out, int(it[0])


def build_mass_and_convection_mass(mesh: Mesh):
    """The M of build_mass_and_convection (StokesColor.py:286-312): the consistent mass, host-assembled
    (scipy CSR, caller numbering); C_u is assembled on the device inside every implicit dye step."""
    ctx = _dye_context(mesh, 0.05, 1e-3)
    return ctx.host_csr(_lib.OP_MCONS)


def surface_edges(mesh: Mesh):
    """The swimmer surface of the mesh (pucfem_host_surface_edges, on the host: no device needed): the edges whose
    two end nodes carry marker 2 and which lie in exactly one triangle, as int32 arrays tri, a, b, opp in ascending
    (triangle, local edge) order."""
    ctx = Context(_lib.HOST_ONLY)
    try:
        ctx.upload(mesh)
        return ctx.surface_edges()
    finally:
        ctx.close()


def swimmer_loads(u, p, mesh: Mesh, nu, center=(0.5, 0.5), edges=False):
    """The swimmer's loads of the given fields on the device (pucfem_loads_apply): u (N, 2), the pressure p (N).
    The dict of Context.swimmer_loads; with edges=True also the (E, 8) per-edge values."""
    from .solver import loads_dict

    ctx = _stokes_context(mesh, 0.05, nu, SquirmerBC(nu=nu, center=tuple(center)))
    r = ctx.loads_apply(u, p, edges)
    return (loads_dict(r[0]), r[1]) if edges else loads_dict(r)


def clear_cache():
    for c in _cache.values():
        c.close()
    _cache.clear()
