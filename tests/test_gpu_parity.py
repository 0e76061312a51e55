"""GPU parity tests: the HIP path (through the C ABI) against the oracle and the reference's goldens.

Tolerances (north_star): Poisson 1e-10 absolute vs the reference; Stokes per step 1e-6 vs the
oracle with the same (well-posed) pressure formulation; non-pressure kernels 1e-12 relative or
bit-exact; the literal reference's ill-posed pressure is compared at its measured noise floor
(1e-2).
"""
import numpy as np
import pytest
from scipy.spatial import KDTree

import oracle as O
from conftest import has_gpu, load_pkg
from mg_reference import synthetic_mesh

pytestmark = pytest.mark.gpu

pf = load_pkg()
from importlib import import_module  # noqa: E402

L = import_module("puc-fluidsimulation-project_amd._lib")
S = import_module("puc-fluidsimulation-project_amd.solver")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not has_gpu():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def stokes(mesh, scheme="color", dt=0.05, nu=0.1, B2=0.0, tol=None):
    return S.StokesSimulation(mesh, S.SquirmerBC(B2=B2, nu=nu), dt, scheme, 0, tol or S.Tolerances())


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("m", ["mesh1", "fine"])
def test_spmv_div_grad(m, golden):
    g = golden(m)
    mesh = pf.load_mesh(m)
    sim = stokes(mesh)
    ctx = sim.ctx
    K = O.stiffness(mesh.coords, mesh.triangles)
    x = np.random.default_rng(1).standard_normal(mesh.N)
    assert rel(ctx.apply(L.OP_K, x, (mesh.N,)), K @ x) < 1e-13
    div = ctx.apply(L.OP_DIV, g["u_rand"], (mesh.N,))
    assert rel(div, g["div_rand"]) < 1e-12
    assert rel(ctx.apply(L.OP_DIV, np.stack([2 * mesh.coords[:, 0], 3 * mesh.coords[:, 1]], 1), (mesh.N,)),
               g["div_lin"]) < 1e-12
    gr = ctx.apply(L.OP_GRAD, g["p_rand"], (mesh.N, 2))
    assert rel(gr, g["grad_rand"]) < 1e-12
    # reference-named shims
    d2 = pf.calculate_divergence(mesh.coords, mesh.triangles, g["u_rand"])
    assert rel(d2, g["div_rand"]) < 1e-12
    gx, gy = pf.calculate_gradiant(mesh.coords, mesh.triangles, g["p_rand"])
    assert rel(np.stack([gx, gy], 1), g["grad_rand"]) < 1e-12
    sim.close()


@pytest.mark.parametrize("m", ["mesh1", "fine"])
@pytest.mark.parametrize("tag,dt,nu", [("color", 0.05, 0.1), ("food", 0.01, 1.0)])
def test_viscous_solve(m, tag, dt, nu, golden):
    """np.linalg.solve(A_visc, rhs) (StokesColor.py:544) replaced by 2-RHS Jacobi-CG."""
    g = golden(m)
    mesh = pf.load_mesh(m)
    sim = stokes(mesh, dt=dt, nu=nu)
    rhs = np.stack([g["u_rand"][:, 0], g["u_rand"][:, 1]], 1)
    x, it = sim.ctx.solve(L.OP_VISC, rhs, rtol=1e-15)
    np.testing.assert_allclose(x[:, 0], g[f"visc_{tag}_x"], rtol=0, atol=1e-12)
    assert it < 60
    sim.close()


@pytest.mark.parametrize("m", ["mesh1", "fine"])
def test_pressure_solve_matches_oracle(m, golden):
    g = golden(m)
    mesh = pf.load_mesh(m)
    sim = stokes(mesh)
    ps = O.PressureSolver(O.stiffness(mesh.coords, mesh.triangles), O.lumped_mass(mesh.coords, mesh.triangles),
                          g["pairs"])
    b = -20.0 * g["div_rand"]
    p_ref = ps.solve(b)
    p, it = sim.ctx.solve(L.OP_PRES, b, rtol=1e-13)
    free = ps.free
    p = p - p[free].mean()
    assert rel(p, p_ref) < 1e-9
    # gauge-free quantity used by the step: the gradient
    gx, gy = O.gradient(mesh.coords, mesh.triangles, p)
    rx, ry = O.gradient(mesh.coords, mesh.triangles, p_ref)
    assert rel(np.stack([gx, gy]), np.stack([rx, ry])) < 1e-9
    sim.close()


@pytest.mark.parametrize("m", ["mesh1", "mesh21", "fine"])
def test_semilagrange_vs_reference(m, golden):
    """advect_semilagrange + PointLocator (k=10 nearest centroids) vs the reference's own output."""
    g = golden(m)
    mesh = pf.load_mesh(m)
    for tag, dt in (("small", 0.05), ("large", 0.2)):
        c = g["c0"].copy()
        nf = pf.advect_semilagrange(c, g["u_swirl"], dt, mesh.coords, mesh.triangles)
        assert np.array_equal(nf, g[f"sl_{tag}_notfound"])
        assert np.array_equal(c, g[f"sl_{tag}"])


@pytest.mark.parametrize("m,refine", [("mesh1", 0), ("fine", 0), ("fine", 2)])
def test_semilagrange_borderline_points(m, refine):
    """PointLocator restated as locate-then-rank (k_sl) vs the oracle's KDTree k=10 search on
    back-traced points that sit on mesh vertices, on edges (midpoints), in the hole, outside the
    domain (clamped y) and at random.  Generic points must agree bit for bit; at vertices several
    triangles pass the weight test and equidistant centroids may be ordered differently by KDTree
    (DESIGN.md §9), so there the value is compared to 1e-13 and the not-found mask exactly."""
    mesh = pf.load_mesh(m, refine=refine)
    X, T = mesh.coords, mesh.triangles
    N = mesh.N
    rng = np.random.default_rng(7)
    dt = 0.05
    mid = 0.5 * (X[T[:, 0]] + X[T[:, 1]])
    kinds = {
        "random": np.stack([rng.random(N), rng.random(N) * 1.2 - 0.1], 1),
        "vertex": X[rng.integers(0, N, N)],
        "edge": mid[rng.integers(0, len(T), N)],
        "hole": 0.5 + 0.2 * (rng.random((N, 2)) - 0.5),
    }
    c0 = np.sin(7 * X[:, 0]) * np.cos(5 * X[:, 1])
    tree = KDTree(O.centroids(X, T))
    for kind, q in kinds.items():
        u = (X - q) / dt
        c = c0.copy()
        nf = pf.advect_semilagrange(c, u, dt, X, T)
        ref, ref_nf = O.sl_advect(c0, u, dt, X, T, tree)
        assert np.array_equal(nf, ref_nf), kind
        if kind in ("random", "hole"):
            assert np.array_equal(c, ref), kind
        else:
            assert np.abs(c - ref).max() < 1e-13, kind


def sl_on(ctx, c, u, dt):
    cin = np.ascontiguousarray(c, dtype=np.float64)
    uu = np.ascontiguousarray(u, dtype=np.float64)
    out = np.zeros_like(cin)
    nf = np.zeros(len(cin), dtype=np.int32)
    L.check(ctx.L.pucfem_sl_advect(ctx.h, L.dptr(cin), L.dptr(uu), float(dt), L.dptr(out), L.iptr(nf)), ctx.h)
    return out, nf.astype(bool)


@pytest.mark.parametrize("refine", [2, 3])
def test_semilagrange_lattice_locator(refine, monkeypatch):
    """The lattice locator (macro face + lattice cell arithmetic, production path on red-refined
    hierarchies) returns the record locator's triangle for every point, bit for bit, including
    points on vertices and edges where several triangles pass the weight test; and the oracle's
    KDTree k=10 PointLocator on the same points (vertices / edges to 1e-13, as above)."""
    mesh = pf.load_mesh("fine", refine=refine)
    X, T = mesh.coords, mesh.triangles
    N = mesh.N
    sim = stokes(mesh, tol=S.Tolerances.production())
    assert sim.ctx.path_info()["sl_locator"] == "lattice"
    # the second pass's three forms: the numbered list (default, k_sl_wq), each wave its own queue (k_sl_wave), one
    # lane per point (k_sl_slow)
    monkeypatch.setenv("PUCFEM_SL_WAVE", "0")
    lane = stokes(mesh, tol=S.Tolerances.production())
    monkeypatch.setenv("PUCFEM_SL_WAVE", "1")
    wave = stokes(mesh, tol=S.Tolerances.production())
    monkeypatch.delenv("PUCFEM_SL_WAVE")
    monkeypatch.setenv("PUCFEM_SL_RECORDS", "1")
    rec = stokes(mesh, tol=S.Tolerances.production())
    assert rec.ctx.path_info()["sl_locator"] == "records"
    rng = np.random.default_rng(11)
    dt = 0.05
    mid = 0.5 * (X[T[:, 0]] + X[T[:, 1]])
    w = rng.random((N, 3))
    w /= w.sum(1, keepdims=True)
    kinds = {
        "random": np.stack([rng.random(N), rng.random(N) * 1.2 - 0.1], 1),
        "vertex": X[rng.integers(0, N, N)],
        "edge": mid[rng.integers(0, len(T), N)],
        "hole": 0.5 + 0.2 * (rng.random((N, 2)) - 0.5),
        "inside": np.einsum("tk,tkd->td", w, X[T[rng.integers(0, len(T), N)]]),
        "x_wrap": np.stack([rng.choice([0.0, 1.0 - 1e-17, 1e-300], N), rng.random(N)], 1),
    }
    c0 = np.sin(7 * X[:, 0]) * np.cos(5 * X[:, 1])
    tree = KDTree(O.centroids(X, T))
    # zero velocity (no-slip walls): q is the row's own node, answered from the build-time table
    kinds["zero"] = np.where(rng.random((N, 1)) < 0.5, X, kinds["random"])
    for kind, q in kinds.items():
        u = (X - q) / dt
        if kind == "zero":
            u[np.all(q == X, axis=1)] = 0.0
        c, nf = sl_on(sim.ctx, c0, u, dt)
        c_rec, nf_rec = sl_on(rec.ctx, c0, u, dt)
        c_lane, nf_lane = sl_on(lane.ctx, c0, u, dt)
        assert np.array_equal(nf, nf_rec), kind
        assert np.array_equal(c, c_rec), kind
        c_wave, nf_wave = sl_on(wave.ctx, c0, u, dt)
        assert np.array_equal(nf, nf_lane) and np.array_equal(c, c_lane), kind  # k_sl_wq = k_sl_slow, bit for bit
        assert np.array_equal(nf, nf_wave) and np.array_equal(c, c_wave), kind  # = k_sl_wave
        ref, ref_nf = O.sl_advect(c0, u, dt, X, T, tree)
        assert np.array_equal(nf, ref_nf), kind
        if kind in ("random", "hole", "inside"):
            assert np.array_equal(c, ref), kind
        else:
            assert np.abs(c - ref).max() < 1e-13, kind
    sim.close()
    rec.close()
    lane.close()
    wave.close()


@pytest.mark.parametrize("m", ["mesh1", "fine"])
def test_tracers_vs_reference(m, golden):
    g = golden(m)
    mesh = pf.load_mesh(m)
    sim = stokes(mesh, "food", dt=0.01, nu=1.0)
    sim.ctx.set_field(L.F_TRACERS, g["tracer0"])
    import ctypes as ct

    u = np.ascontiguousarray(g["u_swirl"])
    L.check(sim.ctx.L.pucfem_tracer_step(sim.ctx.h, L.dptr(u), 0.01, 10), sim.ctx.h)
    pts = sim.ctx.get_field(L.F_TRACERS, g["tracer10"].shape)
    st = sim.ctx.get_field(L.F_STATUS, (len(pts),))
    assert np.array_equal(np.isnan(pts), np.isnan(g["tracer10"]))
    ok = ~np.isnan(g["tracer10"])
    np.testing.assert_allclose(pts[ok], g["tracer10"][ok], rtol=0, atol=1e-12)
    assert np.array_equal(st.astype(int), g["tracer10_status"])
    sim.close()


@pytest.mark.parametrize("path", ["auto", "iterative"])
@pytest.mark.parametrize("m", ["mesh1", "mesh21", "fine"])
def test_poisson_vs_reference(m, path, golden):
    """poisson.py end to end: ||f_ref - f_hip||_inf < 1e-10 (north_star).  The small meshes take the dense
    path by default (the literal operator's inverse, factorised once); "iterative" forces the BiCGStab
    kernels of the large-mesh path onto them."""
    g = golden(m)
    f = pf.poisson_solve(pf.load_mesh(m), tol=S.Tolerances(solver_path=path))
    np.testing.assert_allclose(f, g["poisson_f"], rtol=0, atol=1e-10)


@pytest.mark.parametrize("path", ["auto", "iterative"])
@pytest.mark.parametrize("m", ["mesh1", "mesh21", "fine"])
def test_heat_vs_reference(m, path, golden):
    """heatEq.py: u after 1, 10, 600 backward-Euler steps, 1e-10 vs the reference (dense inverse by
    default on these meshes, BiCGStab with solver_path="iterative")."""
    g = golden(m)
    h = pf.HeatSimulation(pf.load_mesh(m), dt=0.02, tol=S.Tolerances(solver_path=path))
    done = 0
    for k in (1, 10, 600):
        h.step(k - done)
        done = k
        np.testing.assert_allclose(h.u, g[f"heat_u{k}"], rtol=0, atol=1e-10)
    h.close()


@pytest.mark.parametrize("m", ["mesh1", "fine"])
def test_stokes_steps_vs_oracle_and_reference(m, golden):
    """Contract (ii): full steps vs the oracle (same pressure restatement) <= 1e-6;
    contract (iii): vs the literal reference at its LU noise floor (1e-2)."""
    g = golden(m)
    mesh = pf.load_mesh(m)
    ref = O.StokesRef(mesh.coords, mesh.markers, mesh.triangles, 0.05, 0.1, -2.0, 0.0, "color")
    u, c = ref.initial()
    sim = stokes(mesh, tol=S.Tolerances(rtol_visc=1e-14, rtol_pres=1e-13))
    np.testing.assert_array_equal(sim.u, u)
    for k in range(3):
        st = sim.step(1)[0]
        out = ref.step(u, c)
        u, c = out["u"], out["c"]
        for name, f, shp in (("u_star", L.F_USTAR, 2), ("div_u_star", L.F_DIV_STAR, 1), ("final_div", L.F_FINAL_DIV, 1)):
            got = sim.field(f, shp)
            assert np.abs(got - out[name]).max() < 1e-6 * max(1.0, np.abs(out[name]).max()), (k, name)
        assert np.abs(sim.u - u).max() < 1e-6, k
        assert np.abs(sim.c - c).max() < 1e-6, k
        assert abs(st.max_div_star - np.abs(out["div_u_star"]).max()) < 1e-6
        I, mu, var = out["mixing"]
        assert abs(st.mix_var - var) < 1e-9 and abs(st.mix_mu - mu) < 1e-12
        # literal reference (dense LU, ill-posed pressure)
        assert np.abs(sim.u - g[f"color_s{k}_u"]).max() < 1e-2
    sim.close()


def test_food_pusher_steps_vs_oracle(golden):
    g = golden("mesh1")
    mesh = pf.load_mesh("mesh1")
    ref = O.StokesRef(mesh.coords, mesh.markers, mesh.triangles, 0.01, 1.0, -2.0, -5.0, "food")
    u, _ = ref.initial()
    pts = O.tracer_init()
    status = np.zeros(len(pts), dtype=int)
    sim = stokes(mesh, "food", dt=0.01, nu=1.0, B2=-5.0, tol=S.Tolerances(rtol_visc=1e-14, rtol_pres=1e-13))
    for k in range(3):
        st = sim.step(1)[0]
        out = ref.step(u, tracers=pts, status=status)
        u, pts, status = out["u"], out["tracers"], out["status"]
        assert np.abs(sim.u - u).max() < 1e-6
        got = sim.tracers
        assert np.array_equal(np.isnan(got), np.isnan(pts))
        ok = ~np.isnan(pts)
        assert np.abs(got[ok] - pts[ok]).max() < 1e-6
        assert st.eaten == status.sum()
        assert np.abs(sim.u - g[f"food_s{k}_u"]).max() < 1e-2
    sim.close()


def test_refined_mesh_step_properties():
    """Size-independent properties on a refined (L3, ~70k node) mesh: finite, BCs exact, the
    projection reduces the divergence, dye stays in [0, 1], CG converges."""
    mesh = pf.load_mesh("fine", refine=3)
    sim = stokes(mesh, tol=S.Tolerances(rtol_pres=1e-10))
    st = sim.step(2)
    u = sim.u
    assert np.isfinite(u).all()
    pairs, nodes, vals = S.stokes_setup(mesh, S.SquirmerBC())
    np.testing.assert_array_equal(u[nodes], vals)
    c = sim.c
    assert c.min() >= -1e-12 and c.max() <= 1 + 1e-12
    # step 0: u^n is zero in the interior and A_visc has its Dirichlet columns zeroed
    # (StokesColor.py:474), so u* = u^n exactly and the viscous CG needs 0 iterations
    assert st[0].it_visc == 0 and st[1].it_visc > 0
    assert all(s.it_p > 0 and s.it_p2 > 0 for s in st)
    sim.close()


@pytest.mark.parametrize("single", [False, True])
def test_mg_pressure_solve_matches_oracle(golden, single):
    """Geometric-multigrid-preconditioned CG (pressure) on mesh_fine refined twice vs the oracle;
    single: the fp32 V-cycle inside the fp64 CG (the attainable accuracy is the CG's)."""
    mesh = pf.load_mesh("fine", refine=2)
    sim = stokes(mesh, tol=S.Tolerances(precond="mg", mg_single=single))
    assert sim.ctx.precond == "mg"
    X, T = mesh.coords, mesh.triangles
    ps = O.PressureSolver(O.stiffness(X, T), O.lumped_mass(X, T), sim.pairs)
    b = -20.0 * O.divergence(X, T, np.random.default_rng(3).standard_normal((mesh.N, 2)))
    p_ref = ps.solve(b)
    p, it = sim.ctx.solve(L.OP_PRES, b, rtol=1e-12)
    p = p - p[ps.free].mean()
    assert rel(p, p_ref) < 1e-8
    assert it < 40, it
    sim.close()


@pytest.mark.parametrize("order", ["3", "4", "5", "6", "7"])
def test_viscous_extrapolated_start_same_steps(monkeypatch, order):
    """The viscous solve starts from u^n plus an extrapolation of the last viscous increments (order 5
    by default) instead of u^n: only the start changes, so 16 steps equal the plain warm-started run to
    the solve's tolerance (rtol 1e-12), with fewer viscous iterations once the increments exist."""
    mesh = pf.load_mesh("fine", refine=2)
    monkeypatch.setenv("PUCFEM_VISC_EXTRAP", order)  # read when a context is created
    a = stokes(mesh)
    assert a.ctx.path_info()["visc_extrap_order"] == 0  # no increments yet
    monkeypatch.setenv("PUCFEM_VISC_EXTRAP", "0")
    b = stokes(mesh)
    sa, sb = a.step(16), b.step(16)
    assert np.abs(a.u - b.u).max() < 1e-9
    assert np.abs(a.c - b.c).max() < 1e-9
    assert sum(x.it_visc for x in sa[4:]) < sum(x.it_visc for x in sb[4:])
    assert a.ctx.path_info()["visc_extrap_order"] == int(order)
    a.close()
    b.close()


def test_viscous_chebyshev_post_check(monkeypatch):
    """The Chebyshev viscous solve takes its step count from the a-priori residual bound of its interval;
    the last step of each solve also reduces the residual of the iterate it starts from, and the next
    solve checks it against that bound.  With the true interval the check never fires; with a
    deliberately short one (PUCFEM_VISC_R_SCALE) it fires and the viscous solves switch to the CG."""
    mesh = pf.load_mesh("fine", refine=2)
    a = stokes(mesh)
    monkeypatch.setenv("PUCFEM_VISC_R_SCALE", "0.3")  # read when the operators are built
    b = stokes(mesh)
    a.step(12)
    b.step(12)
    pa, pb = a.ctx.path_info(), b.ctx.path_info()
    assert pa["viscous_iteration"] == "chebyshev" and not pa["visc_check_failed"]
    assert pb["visc_check_failed"] and pb["viscous_iteration"] == "cg"
    assert np.isfinite(b.u).all()
    a.close()
    b.close()


@pytest.mark.parametrize("mesh_name,refine", [("fine", 3), ("fine", 5), ("synthetic", 6)], ids=["3", "5", "synthetic-6"])
@pytest.mark.parametrize("knob,key", [("PUCFEM_VISC_PAIR", "visc_step_pairs"), ("PUCFEM_MG_PAIR", "mg_step_pairs")])
def test_step_pairs_equal_single_steps(monkeypatch, mesh_name, refine, knob, key):
    """Two Chebyshev steps in one pass on the face interiors (x_{a+1} in LDS, the skeleton rows in their
    own launches): the viscous solve's (k_vcheb_pair) and the finest multigrid level's smoothing
    (k_cheb_pair) do k_vcheb's / k_cheb's operations row by row, so the production run at L3 / L5 with
    step pairs is bit-identical to the one that runs every step as its own launch.  On `fine` every face
    is one work item; the synthetic 24-face mesh at lattice size 64 has two items per face, whose windows
    overlap and whose x_{a+1} halos come from the neighbouring item's rows."""
    mesh = synthetic_mesh(refine) if mesh_name == "synthetic" else pf.load_mesh("fine", refine=refine)
    a = stokes(mesh, tol=S.Tolerances.production())
    monkeypatch.setenv(knob, "0")
    b = stokes(mesh, tol=S.Tolerances.production())
    sa, sb = a.step(8), b.step(8)
    assert a.ctx.path_info()[key] and not b.ctx.path_info()[key]
    assert [(s.it_visc, s.it_p, s.it_p2) for s in sa] == [(s.it_visc, s.it_p, s.it_p2) for s in sb]
    assert np.array_equal(a.u, b.u) and np.array_equal(a.c, b.c)
    a.close()
    b.close()


@pytest.mark.parametrize("refine,shared", [(3, True), (3, False), (5, True)])
def test_pending_pressure_directions_equal_stored(monkeypatch, refine, shared):
    """The projection's new direction left pending after a pressure solve (v = y - x0 and A v = r0 - r_final
    formed by the next solve's k_mdot2 / k_pcomb instead of stored by k_diff2_fin) and the gradient projection
    gathering the solution y through the merged slave -> master tables (instead of p = y with the slaves
    copied) compute the same values: the production run is bit-identical to the stored form, over step()
    calls of several sizes (a pending direction is stored at the end of every call), including the
    pressure fields read back."""
    mesh = pf.load_mesh("fine", refine=refine)
    a = stokes(mesh, tol=S.Tolerances.production(proj_shared=shared))
    monkeypatch.setenv("PUCFEM_P_FROM_Y", "0")
    b = stokes(mesh, tol=S.Tolerances.production(proj_shared=shared))
    assert a.ctx.path_info()["pending_pressure_directions"] and not b.ctx.path_info()["pending_pressure_directions"]
    sa, sb = [], []
    for k in (1, 3, 5):
        sa += a.step(k)
        sb += b.step(k)
    assert [(s.it_visc, s.it_p, s.it_p2) for s in sa] == [(s.it_visc, s.it_p, s.it_p2) for s in sb]
    assert np.array_equal(a.u, b.u) and np.array_equal(a.c, b.c)
    assert np.array_equal(a.field(L.F_P), b.field(L.F_P))
    assert np.array_equal(a.field(L.F_P2), b.field(L.F_P2))
    a.close()
    b.close()


@pytest.mark.parametrize("refine", [3, 5])
def test_pressure_rhs_in_projection_pass_equals_separate(monkeypatch, refine):
    """The pressure right-hand side (StokesColor.py:554, restated: slaves merged into masters, the mean over the free
    rows removed) formed inside the projection's first pass (k_mdot2) on projected solves is bit-identical to the
    separate k_pres_rhs pass, over step() calls of several sizes including solves that pass at their guess; the
    pressure fields read back agree too."""
    mesh = pf.load_mesh("fine", refine=refine)
    a = stokes(mesh, tol=S.Tolerances.production())
    monkeypatch.setenv("PUCFEM_RHS_FUSE", "0")
    b = stokes(mesh, tol=S.Tolerances.production())
    sa, sb = [], []
    for k in (1, 5, 14):
        sa += a.step(k)
        sb += b.step(k)
    assert [(s.it_visc, s.it_p, s.it_p2) for s in sa] == [(s.it_visc, s.it_p, s.it_p2) for s in sb]
    assert np.array_equal(a.u, b.u) and np.array_equal(a.c, b.c)
    assert np.array_equal(a.field(L.F_P), b.field(L.F_P))
    assert np.array_equal(a.field(L.F_P2), b.field(L.F_P2))
    a.close()
    b.close()


@pytest.mark.parametrize("records", ["0", "1"])
def test_knn_radii_device_equals_host(monkeypatch, records):
    """The semi-Lagrangian fast-accept radii (k-NN distances of every centroid and vertex) are built on
    the device (k_knn_radius2) as the host's knn_radius2 builds them: 6 StokesColor steps at L3 with
    either table are bit-identical, with the lattice locator and with the record locator."""
    mesh = pf.load_mesh("fine", refine=3)
    monkeypatch.setenv("PUCFEM_SL_RECORDS", records)
    a = stokes(mesh, tol=S.Tolerances.production())
    monkeypatch.setenv("PUCFEM_KNN_HOST", "1")
    b = stokes(mesh, tol=S.Tolerances.production())
    assert a.ctx.path_info()["sl_locator"] == ("records" if records == "1" else "lattice")
    sa, sb = a.step(6), b.step(6)
    assert np.array_equal(a.u, b.u) and np.array_equal(a.c, b.c)
    assert [s.sl_notfound for s in sa] == [s.sl_notfound for s in sb]
    a.close()
    b.close()


@pytest.mark.parametrize("shared", [False, True])
def test_projected_pressure_guess_same_steps(shared):
    """Successive-RHS projection (Fischer) only changes the pressure CG's initial guess: 24 steps with
    a 3-vector basis (several restarts) equal the warm-started run to the CG tolerance, and once the
    flow is steady the projected guesses need fewer iterations -- with a basis per pressure solve and
    with one basis shared by both solves of a step."""
    mesh = pf.load_mesh("fine", refine=2)
    a = stokes(mesh, tol=S.Tolerances(rtol_pres=1e-12, precond="mg", proj_k=3, proj_shared=shared))
    b = stokes(mesh, tol=S.Tolerances(rtol_pres=1e-12, precond="mg", proj_k=0))
    sa, sb = a.step(24), b.step(24)
    assert np.abs(a.u - b.u).max() < 1e-8
    assert np.abs(a.c - b.c).max() < 1e-8
    assert sum(x.it_p + x.it_p2 for x in sa[12:]) < sum(x.it_p + x.it_p2 for x in sb[12:])
    a.close()
    b.close()


@pytest.mark.parametrize("single", [False, True])
def test_mg_and_jacobi_steps_agree(single):
    """The two pressure preconditioners give the same Stokes steps (tolerance-limited)."""
    mesh = pf.load_mesh("fine", refine=2)
    a = stokes(mesh, tol=S.Tolerances(rtol_pres=1e-12, precond="mg", mg_single=single))
    b = stokes(mesh, tol=S.Tolerances(rtol_pres=1e-12, precond="jacobi"))
    sa, sb = a.step(3), b.step(3)
    assert np.abs(a.u - b.u).max() < 1e-7
    assert np.abs(a.c - b.c).max() < 1e-7
    assert all(x.it_p < 40 for x in sa) and all(x.it_p > 200 for x in sb)
    a.close()
    b.close()


@pytest.mark.parametrize("refine", [3, 5])
def test_mg_lmax_device_equals_host(refine):
    """The multigrid smoothing interval [lmax / ratio, lmax] (the preconditioner of the pressure solves that
    replace np.linalg.solve at StokesColor.py:555,569): every level's device power iteration (fp64 on the finest
    level, the fp32 V-cycle values below it) gives the host fp64 power iteration's quotient on the same level
    operator, and lmax = min(Gershgorin, 1.1 x quotient)."""
    mesh = pf.load_mesh("fine", refine=refine)
    sim = stokes(mesh, tol=S.Tolerances.production())
    levels = sim.ctx.info()["mg_levels"]
    assert levels == refine + 1
    for lv in range(levels):
        d = sim.ctx.mg_lmax(lv)
        if lv == 0:  # the coarsest level is solved densely; its interval comes from the host estimate
            assert d["lam_device"] == 0.0
            lam = d["lam_host"]
        else:
            lam = d["lam_device"]
            assert abs(lam - d["lam_host"]) <= 1e-5 * d["lam_host"], (lv, d)
        assert abs(d["lmax"] - min(d["gershgorin"], 1.1 * lam)) <= 1e-12 * d["lmax"], (lv, d)
        assert 1.0 < d["lmax"] <= d["gershgorin"] + 1e-12
    sim.close()


@pytest.mark.timeout(300)
def test_projection_basis_holds_below_the_guess_floor_L7():
    """Regression (round 5): with the projection's new direction formed as y - x0 from the two stored fp64
    vectors, A v from the CG's residuals did not match it once the guesses reached ~1e-7 of b on L7 (the rounding
    of y and x0 has an A-norm comparable to the correction), the basis decayed and a solve at rtol 5e-8 went from
    0-1 to 6 iterations from step ~110 on.  The CG now accumulates v itself: 20 steps past the transient at
    rtol 5e-8 take at most 2 iterations per solve on average."""
    mesh = pf.load_mesh("fine", refine=7)
    sim = stokes(mesh, tol=S.Tolerances.production(rtol_pres=5e-8))
    sim.step(100)
    st = sim.step(20)
    its = sum(s.it_p + s.it_p2 for s in st)
    print(f"L7 steps 100-119 at rtol 5e-8: {its} pressure iterations over 40 solves")
    assert its <= 80, [(s.it_p, s.it_p2) for s in st]
    sim.close()


@pytest.mark.parametrize("refine", [3, 5])
def test_single_reduction_pcg_matches_standard(monkeypatch, refine):
    """The Chronopoulos-Gear form of the pressure PCG (one all-reduce per iteration: the multi-rank solves of
    StokesColor.py:555,569) forced on one rank solves the same systems as the standard form: 12 production steps
    agree to the solves' tolerance and take the same iteration counts up to one per solve."""
    mesh = pf.load_mesh("fine", refine=refine)
    a = stokes(mesh, tol=S.Tolerances.production())
    monkeypatch.setenv("PUCFEM_CGCG", "1")
    b = stokes(mesh, tol=S.Tolerances.production())
    sa, sb = a.step(12), b.step(12)
    assert np.abs(a.u - b.u).max() < 1e-7
    assert np.abs(a.c - b.c).max() < 1e-6
    for x, y in zip(sa, sb):
        assert abs(x.it_p - y.it_p) <= 1 and abs(x.it_p2 - y.it_p2) <= 1, (x.it_p, x.it_p2, y.it_p, y.it_p2)
    a.close()
    b.close()


def test_single_reduction_recurrence_needs_a_resolved_estimate():
    """k_cgcg_coef: the one-step recurrence rho_(it+1) = rho - 2 alpha rs + alpha^2 ss only ends a solve
    when the estimate is resolved -- positive and above its rounding floor (~eps (rho + 2 |alpha rs| + alpha^2 ss));
    a cancelled (zero, negative or rounding-level) estimate leaves the decision to the next iteration's exact rho.
    State: alpha_(it-1) = gamma_(it-1) = 1, gamma = 1, delta = 2, so beta = 1 and alpha = 1."""
    mesh = pf.load_mesh("fine")
    sim = stokes(mesh)

    def coef(rho, rw, ww, tol2, b2=1.0):
        red8 = np.array([rho, 0.0, 0.0, 1.0, 2.0, rw, ww, 0.0])  # rho, rs_old, ss_old, gamma, delta, rw, ww, ws
        sc = np.array([0.0, 0.0, 0.0, 1.0, 1.0])
        ctl = np.zeros(2, dtype=np.int32)
        out = np.zeros(5)
        L.check(sim.ctx.L.pucfem_cgcg_coef_probe(sim.ctx.h, L.dptr(red8), float(b2), L.dptr(sc), float(tol2), 1, 100,
                                                 1.0, L.iptr(ctl), L.dptr(out)), sim.ctx.h)
        if not (ctl[0] == 1 and ctl[1] == 1):  # (an exact pass returns before the scalars)
            assert out[0] == 1.0 and out[1] == 1.0  # alpha, beta
        return tuple(int(v) for v in ctl)

    # rho1 = rho - 2 rw + ww
    assert coef(1.0, 0.5, 0.0, 1e-14) == (0, 0)        # cancels to exactly 0: not accepted
    assert coef(1.0, 0.5, -1e-3, 1e-14) == (0, 0)      # negative: not accepted
    assert coef(1.0, 0.5, 1e-15, 1e-14) == (0, 0)      # 1e-15, below the rounding floor of 1: not accepted
    assert coef(2.0, 0.5, 0.0, 1.0) == (1, 2)          # 1.0 <= tol2 b2, resolved: the update of it = 1 completes
    assert coef(2.0, 0.25, 0.0, 1.0) == (0, 0)         # 1.5 > tol2 b2: continue
    assert coef(1e-15, 0.0, 0.0, 1e-14) == (1, 1)      # the exact rho passes: converged at it = 1
    sim.close()
