"""CPU tests of the V-cycle reference (tests/mg_reference.py) and of the synthetic mesh the multigrid GPU tests
run on, and the refusals of pucfem_mg_probe where it cannot run.

The reference is the yardstick of tests/test_gpu_mg_cycle.py, so it is checked on its own here: the cycle it
restates is a symmetric positive operator (equal pre- and post-smoothing), its fp32 restatement stays within the
cap the device bound relies on (8 x 1e-6), and one wrong matrix entry moves its result far beyond that bound.
The synthetic mesh extends test_lattice_host's hierarchy to lattice size n = 64, where a face has more rows
than one work item of the face kernels takes.
"""
import ctypes as ct

import numpy as np
import pytest

import mg_reference as R
from test_lattice_host import close, interior_count, lat_apply

L, S = R.L, R.S

E_REF_CAP = 1e-6  # the fp32 restatement's deviation from the fp64 reference, every configuration


@pytest.fixture(scope="module", params=[2, 3, 6])
def synth(request):
    lv = request.param
    mesh = R.synthetic_mesh(lv)
    ctx = R.mg_context(mesh, R.config_tol("d3p3"))
    yield lv, mesh, ctx
    ctx.close()


def test_synthetic_base_mesh():
    m = R.synthetic_base()
    assert (m.N, m.T) == (24, 24)
    assert (m.markers == R.M.INNER_BOUNDARY_MARKER).sum() == 8
    X, T = m.coords, m.triangles
    a, b, c = X[T[:, 0]], X[T[:, 1]], X[T[:, 2]]
    area = 0.5 * ((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0]))
    assert (area > 0).all() and abs(area.sum() - 0.75) < 1e-15  # counter-clockwise, the square minus the hole


def test_synthetic_hierarchy_builds(synth):
    lv, mesh, ctx = synth
    n = 2 ** lv
    assert mesh.N == {2: 240, 3: 864, 6: 49920}[lv]
    assert ctx.path_info()["lattice"]
    assert ctx.info()["n_pairs"] == n * 4 - 1
    assert [ctx.mg_level_size(l) for l in range(lv + 1)] == [R.synthetic_mesh(l).N if l else 24 for l in range(lv + 1)]
    # every face interior is a face row: F = (n - 1)(n - 2) / 2 on each of the 24 faces
    assert R.face_rows(ctx, lv).sum() == 24 * interior_count(n)


def test_synthetic_face_stencils_agree_with_the_csr(synth):
    """The host face stencils (finest K, gradient, A_visc; the merged pressure operator and the transfers of every
    level) against the host CSRs, as test_lattice_host checks them on `fine` at n = 4 and 8."""
    lv, mesh, ctx = synth
    rng = np.random.default_rng(11)
    x = rng.standard_normal(mesh.N)
    n, err = close(lat_apply(ctx, lv, 0, x, mesh.N), ctx.host_csr(L.OP_K) @ x)
    assert n == 24 * interior_count(2 ** lv) and err < 1e-12, err
    u = rng.standard_normal((mesh.N, 2))
    Gx, Gy = ctx.host_csr(L.OP_GX), ctx.host_csr(L.OP_GY)
    _, err = close(lat_apply(ctx, lv, 1, u, mesh.N), Gx @ u[:, 0] + Gy @ u[:, 1])
    assert err < 1e-12, err
    Av = ctx.host_csr(L.OP_VISC)
    s = 1.0 / np.sqrt(Av.diagonal())
    _, err = close(lat_apply(ctx, lv, 2, x, mesh.N), s * (Av @ (s * x)))
    assert err < 1e-12, err
    for l in range(1, lv + 1):
        nf, nc = ctx.mg_level_size(l), ctx.mg_level_size(l - 1)
        A, Pr, Rs = (R.level_csr(ctx, l, k) for k in range(3))
        xf, xc = rng.standard_normal(nf), rng.standard_normal(nc)
        if interior_count(2 ** l):
            n, err = close(lat_apply(ctx, l, 3, xf, nf), A @ xf)
            assert n == 24 * interior_count(2 ** l) and err < 1e-12, (l, err)
            _, err = close(lat_apply(ctx, l, 5, xc, nf), Pr @ xc)
            assert err < 1e-15, (l, err)
        if interior_count(2 ** (l - 1)):
            _, err = close(lat_apply(ctx, l, 6, xf, nc), Rs @ xf)
            assert err < 1e-14, (l, err)


def test_level_operators_are_what_the_reference_assumes(synth):
    """Slave rows of A_l are identity rows and slave rows of P_l are empty (so arbitrary values on slave rows are
    covered by the reference), R_l = P_l^T, A_l is symmetric."""
    lv, mesh, ctx = synth
    for l in range(1, lv + 1):
        A, Pr, Rs = (R.level_csr(ctx, l, k) for k in range(3))
        assert abs(A - A.T).max() < 1e-12 * abs(A).max()
        assert abs(Rs - Pr.T).max() == 0.0
        slave = np.diff(Pr.indptr) == 0
        assert slave.sum() == 2 ** l * 4 - 1
        rows = A[slave]
        assert (np.diff(rows.indptr) == 1).all() and (rows.data == 1.0).all()
        assert (rows.indices == np.flatnonzero(slave)).all()


@pytest.fixture(scope="module", params=[3, 6])
def refs(request):
    lv = request.param
    ctx = R.mg_context(R.synthetic_mesh(lv), R.config_tol("d3p3"))
    ref = R.Reference(ctx, lv, R.config_tol("d3p3"))
    ctx.close()
    return lv, ref


def test_cheb_coefs_are_chebyshev():
    """The restated step coefficients give the Chebyshev residual polynomial: after k steps on the scalar problem
    lam x = 1 from x = 0 the residual is T_k((theta - lam) / delta) / T_k(sigma)."""
    lmax, ratio = 1.9, 15.0
    lmin = lmax / ratio
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    for lam in (lmin, 0.7, lmax):
        x = d = 0.0
        for k, (c1, c2) in enumerate(R.cheb_coefs(lmax, ratio, 1, 5), 1):
            d = c1 * d + c2 * (1.0 - lam * x)
            x += d
            tk = np.polynomial.chebyshev.Chebyshev.basis(k)
            assert abs((1.0 - lam * x) - tk((theta - lam) / delta) / tk(theta / delta)) < 1e-13
    # fourth kind (Lottes 2022): the first step is 4 / (3 lmax), and the residual stays below 1 on (0, lmax]
    c = R.cheb_coefs(lmax, ratio, 4, 3)
    assert c[0] == (0.0, 4.0 / (3.0 * lmax)) and c[1] == (1.0 / 5.0, 12.0 / (5.0 * lmax))
    for lam in np.linspace(0.05, lmax, 9):
        x = d = 0.0
        for c1, c2 in c:
            d = c1 * d + c2 * (1.0 - lam * x)
            x += d
        assert abs(1.0 - lam * x) < 1.0


@pytest.mark.parametrize("name", ["d1p0", "d2p0", "d3p3", "kind4"])
def test_reference_is_symmetric_and_positive(refs, name):
    lv, base = refs
    ref = R.Reference(None, lv, R.config_tol(name), np.float64, None, base.shared)
    x, y = R.level_vectors(ref, lv, 5)
    mx, my = ref.precondition(x), ref.precondition(y)
    assert abs(y @ mx - x @ my) <= 1e-15 * np.linalg.norm(x) * np.linalg.norm(my)
    assert x @ mx > 0 and y @ my > 0
    r32 = ref.other(np.float32)
    d32 = abs(y @ r32.precondition(x).astype(np.float64) - x @ r32.precondition(y).astype(np.float64))
    assert d32 <= 1e-7 * np.linalg.norm(x) * np.linalg.norm(my)  # (fp32 rounding: eps = 6e-8 per operation)


@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_fp32_restatement_stays_within_the_cap(refs, name):
    lv, base = refs
    tol = R.config_tol(name)
    ref = R.Reference(None, lv, tol, np.float64, None, base.shared)
    r32 = ref.other(np.float32)
    x, _ = R.level_vectors(ref, lv, 6)
    e_ref = R.relmax(r32.precondition(x), ref.precondition(x))
    print(f"refine {lv} {name}: e_ref = {e_ref:.3e}")
    assert 0 < e_ref < E_REF_CAP
    for l in range(1, lv + 1):  # the pieces, level by level
        b, v = R.level_vectors(ref, l, 7)
        for a32, a64 in ((r32.resid(l, b, v), ref.resid(l, b, v)), (r32.smooth0(l, b), ref.smooth0(l, b)),
                         (r32.smoothx(l, b, v), ref.smoothx(l, b, v)), (r32.restrict(l, v), ref.restrict(l, v))):
            assert R.relmax(a32, a64) < E_REF_CAP


def test_one_wrong_entry_shows(refs):
    """A 1e-3 relative error in one diagonal entry of the finest operator moves z by far more than the device
    bound 8 e_ref <= 8e-6: the comparison catches a single wrong coefficient."""
    lv, ref = refs
    x, _ = R.level_vectors(ref, lv, 8)
    z = ref.precondition(x)
    row = int(np.flatnonzero(ref.shared["face"][lv])[ref.n[lv] // 3])
    moved = R.relmax(ref.other(np.float64, planted=(lv, row, 1e-3)).precondition(x), z)
    assert moved > 20 * 8 * E_REF_CAP, moved


def test_mg_probe_refusals():
    """pucfem_mg_probe needs a device and a hierarchy: a host-only context is PUCFEM_ESTATE, a context without a
    hierarchy PUCFEM_EINVAL, each with a message; before the build it is PUCFEM_ESTATE like every other call."""
    lib = L.lib()
    z = np.zeros(8)
    rz = ct.c_double()
    prz = ct.cast(ct.byref(rz), ct.POINTER(ct.c_double))
    p = ct.c_void_p()
    L.check(lib.pucfem_ctx_create(L.HOST_ONLY, ct.byref(p)))
    assert lib.pucfem_mg_probe(p, 0, 1, L.dptr(z), L.dptr(z), L.dptr(z), prz) == -4
    assert b"build" in lib.pucfem_last_error(p)
    L.check(lib.pucfem_ctx_destroy(p))
    mesh = R.synthetic_mesh(2)
    ctx = R.mg_context(mesh, R.config_tol("d3p3"))  # host-only, with a hierarchy
    b = np.zeros(mesh.N)
    assert lib.pucfem_mg_probe(ctx.h, 0, 2, L.dptr(b), L.dptr(b), L.dptr(b), prz) == -4
    assert b"device" in lib.pucfem_last_error(ctx.h)
    with pytest.raises(Exception, match="device"):
        ctx.mg_probe("cycle", 2, b=b)
    ctx.close()
    plain = S.Context(L.HOST_ONLY)  # no hierarchy
    plain.upload(mesh)
    pairs, nodes, vals = S.stokes_setup(mesh, S.SquirmerBC())
    plain.set_pairs(0, pairs)
    plain.set_pairs(1, pairs)
    plain.set_dirichlet(nodes, vals)
    plain.build("color", 0.05, 0.1, S.Tolerances(precond="jacobi"))
    assert lib.pucfem_mg_probe(plain.h, 6, 2, L.dptr(b), None, L.dptr(b), prz) == -1
    assert b"hierarchy" in lib.pucfem_last_error(plain.h)
    with pytest.raises(Exception, match="multigrid"):
        plain.mg_probe("cycle", 2, b=b)
    plain.close()
