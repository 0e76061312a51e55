"""The pressure multigrid's V-cycle on the GPU, piece by piece, against the fp64 reference of tests/mg_reference.py.

The outer pressure solver is an fp64 PCG: with a slightly wrong preconditioner (one wrong stencil coefficient, a
prolongation missing a parity case, a smoother reading a stale neighbour across a work-item boundary) it still
converges, so whole-run parity cannot see such an error.  Here pucfem_mg_probe runs the cycle's own launch sites --
residual, both smoothing calls, restriction, prolongation, coarse solve, the cycle from every level, and
precondition() as the PCG calls it -- on given vectors, and every result is compared row by row (max norm, scaled
by max |reference|) with the reference.

Shapes: the synthetic 24-face mesh at lattice sizes n = 8 (one work item per face), 64 (two items per face: the
windows and halos of k_cheb_pair), 256 (= VP_HALO, 32 items per face, 768 items: the XCD-grouped item order), and
the unstructured `fine` mesh at n = 8 (1,700 faces).

Tolerances: the fp64 cycle agrees with the reference to 1e-12 (summation order, and face stencil coefficients that
agree with the CSR rows to ~2e-15).  For the fp32 cycle each case computes e_ref, the deviation of the reference's
own fp32 restatement from the fp64 reference, and requires the device's deviation e_dev <= 8 e_ref: both round the
same operands through the same number of dependent operations per row and differ in the summation order within a
row (<= 7 terms on face rows, <= ~14 on skeleton rows); tests/test_mg_reference_host.py caps e_ref at 1e-6 and
shows that one wrong matrix entry moves the result by > 20 x 8e-6.
"""
import numpy as np
import pytest

import mg_reference as R
from conftest import has_gpu

pytestmark = pytest.mark.gpu

pf, L, S = R.pf, R.L, R.S

FACTOR = 8.0     # e_dev <= FACTOR * e_ref (fp32 cycle)
TOL64 = 1e-12    # fp64 cycle against the fp64 reference


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not has_gpu():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def mesh_of(key):
    return pf.load_mesh("fine", refine=3) if key == "fine3" else R.synthetic_mesh(int(key[1:]))


class World:
    """Device contexts and references, built once per (mesh, configuration, precision) and shared by the tests (the
    probe leaves a context as it found it)."""

    def __init__(self):
        self.hier, self.ctxs = {}, {}

    def get(self, key, name="d3p3", single=True):
        k = (key, name, single)
        if k not in self.ctxs:
            mesh = mesh_of(key)
            tol = R.config_tol(name, single)
            ctx = R.mg_context(mesh, tol, device=0)
            if key not in self.hier:
                self.hier[key] = R.read_hierarchy(ctx, mesh.levels)
            ref = R.Reference(ctx, mesh.levels, tol, np.float64, None, self.hier[key])
            self.ctxs[k] = (ctx, ref, ref.other(np.float32) if single else None)
        return self.ctxs[k]

    def drop(self, key):
        for k in [k for k in self.ctxs if k[0] == key]:
            self.ctxs.pop(k)[0].close()
        self.hier.pop(key, None)

    def close(self):
        for ctx, _, _ in self.ctxs.values():
            ctx.close()
        self.ctxs.clear()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


RATIOS = {}  # test -> the largest e_dev / e_ref it saw (printed; DESIGN.md records them)


def check(what, dev, ref64, ref32, tag):
    """dev against the fp64 reference value ref64: 1e-12 for the fp64 cycle (ref32 None); for the fp32 cycle within
    FACTOR times the deviation of the reference's fp32 restatement ref32."""
    assert np.isfinite(dev).all(), what
    e_dev = R.relmax(dev, ref64)
    if ref32 is None:
        print(f"{what}: e_dev = {e_dev:.3e} (fp64)")
        assert e_dev <= TOL64, (what, e_dev)
        return
    e_ref = R.relmax(ref32, ref64)
    ratio = e_dev / e_ref if e_ref > 0 else (0.0 if e_dev == 0 else np.inf)
    RATIOS[tag] = max(RATIOS.get(tag, 0.0), ratio)
    print(f"{what}: e_dev = {e_dev:.3e}, e_ref = {e_ref:.3e}, ratio = {ratio:.2f}")
    assert e_dev <= FACTOR * e_ref, (what, e_dev, e_ref)


def both(ref, r32, f):
    return f(ref), (None if r32 is None else f(r32))


# ---- a. each piece, each level, both precisions
@pytest.mark.parametrize("single", [True, False], ids=["fp32", "fp64"])
@pytest.mark.parametrize("key", ["s3", "s6", "fine3"])
def test_pieces_every_level(world, key, single):
    ctx, ref, r32 = world.get(key, "d3p3", single)
    lv = ref.levels
    tag = f"pieces[{key}]"
    for l in range(1, lv + 1):
        b, x = R.level_vectors(ref, l, 1)
        xc, _ = R.level_vectors(ref, l - 1, 2)
        w = f"{key} level {l} "
        check(w + "resid", ctx.mg_probe("resid", l, b=b, x=x), *both(ref, r32, lambda r: r.resid(l, b, x)), tag)
        check(w + "smooth0", ctx.mg_probe("smooth0", l, b=b), *both(ref, r32, lambda r: r.smooth0(l, b)), tag)
        check(w + "smoothx", ctx.mg_probe("smoothx", l, b=b, x=x), *both(ref, r32, lambda r: r.smoothx(l, b, x)), tag)
        check(w + "restrict", ctx.mg_probe("restrict", l, x=x), *both(ref, r32, lambda r: r.restrict(l, x)), tag)
        check(w + "prolong", ctx.mg_probe("prolong", l, b=xc, x=x),
              *both(ref, r32, lambda r: r.prolong_add(l, xc, x)), tag)
    b0, _ = R.level_vectors(ref, 0, 3)
    check(f"{key} coarse", ctx.mg_probe("coarse", 0, b=b0), *both(ref, r32, lambda r: r.coarse(b0)), tag)
    print(f"largest e_dev / e_ref, {tag}: {RATIOS.get(tag, 0.0):.2f}")


# ---- b. the whole cycle and precondition
def check_precondition(ctx, ref, r32, what, tag):
    r, _ = R.level_vectors(ref, ref.levels, 4)
    z, rz = ctx.mg_probe("precondition", ref.levels, b=r)
    check(what + " z", z, *both(ref, r32, lambda q: q.precondition(r)), tag)
    # <r, z>: an fp64 reduction of the device's own z, only the summation order differs
    want = float(np.dot(r, z))
    assert abs(rz - want) <= 1e-13 * abs(want), (what, rz, want)
    return r, z


@pytest.mark.parametrize("single", [True, False], ids=["fp32", "fp64"])
@pytest.mark.parametrize("key", ["s3", "s6", "s8"])
def test_cycle_and_precondition(world, key, single):
    ctx, ref, r32 = world.get(key, "d3p3", single)
    tag = f"cycle[{key}]"
    for l in range(0, ref.levels + 1):
        b, _ = R.level_vectors(ref, l, 5)
        check(f"{key} cycle from level {l}", ctx.mg_probe("cycle", l, b=b), *both(ref, r32, lambda q: q.cycle(l, b)),
              tag)
    check_precondition(ctx, ref, r32, f"{key} precondition", tag)
    n = 2 ** ref.levels
    items = 24 * -(-((n - 1) * (n - 2) // 2) // 1024)
    assert ctx.path_info()["mg_step_pairs"] == single, "step pairs run on the fp32 cycle's finest level"
    assert items == {"s3": 24, "s6": 48, "s8": 768}[key]
    print(f"largest e_dev / e_ref, {tag}: {RATIOS.get(tag, 0.0):.2f}")
    if key == "s8":
        world.drop("s8")


def test_precondition_past_the_pair_halo(world):
    """Lattice size 512 > VP_HALO (3.1M nodes): the production cycle falls back to single steps on the finest
    level, 128 work items per face."""
    ctx, ref, r32 = world.get("s9", "d3p3", True)
    lv = ref.levels
    tag = "cycle[s9]"
    b, x = R.level_vectors(ref, lv, 5)
    check("s9 smooth0", ctx.mg_probe("smooth0", lv, b=b), *both(ref, r32, lambda q: q.smooth0(lv, b)), tag)
    check("s9 smoothx", ctx.mg_probe("smoothx", lv, b=b, x=x), *both(ref, r32, lambda q: q.smoothx(lv, b, x)), tag)
    check_precondition(ctx, ref, r32, "s9 precondition", tag)
    assert not ctx.path_info()["mg_step_pairs"]
    print(f"largest e_dev / e_ref, {tag}: {RATIOS.get(tag, 0.0):.2f}")
    world.drop("s9")


# ---- c. the smoother's branches (fp32 cycle, two work items per face)
@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_smoother_configurations(world, name):
    ctx, ref, r32 = world.get("s6", name, True)
    lv = ref.levels
    tag = f"config[{name}]"
    b, x = R.level_vectors(ref, lv, 6)
    check(f"{name} smooth0", ctx.mg_probe("smooth0", lv, b=b), *both(ref, r32, lambda q: q.smooth0(lv, b)), tag)
    check(f"{name} smoothx", ctx.mg_probe("smoothx", lv, b=b, x=x), *both(ref, r32, lambda q: q.smoothx(lv, b, x)), tag)
    check(f"{name} cycle from level {lv - 1}", ctx.mg_probe("cycle", lv - 1, b=R.level_vectors(ref, lv - 1, 6)[0]),
          *both(ref, r32, lambda q: q.cycle(lv - 1, R.level_vectors(ref, lv - 1, 6)[0])), tag)
    check_precondition(ctx, ref, r32, f"{name} precondition", tag)
    info = ctx.info()
    assert info["mg_f16_vals"] == (name == "f16")  # (the finest level's values; "coarse" keeps them fp32)
    assert not (name == "idx32" and info["index16_Pp"])
    # pairs run wherever two steps are left that do not write z: every configuration but the one-step ones
    assert ctx.path_info()["mg_step_pairs"] == (name not in ("d1p0",))
    print(f"largest e_dev / e_ref, {tag}: {RATIOS.get(tag, 0.0):.2f}")


# ---- d. pairs against single steps, piece by piece
@pytest.mark.parametrize("key,name", [("s6", "d3p5"), ("s6", "d5p4"), ("s8", "d3p5")])
def test_pair_pieces_equal_single_steps(monkeypatch, key, name):
    """k_cheb_pair's claim (bit-identical to two k_cheb launches) where work items share a face: both smoothing
    calls of the finest level and the whole cycle, with pairs and with every step as its own launch.  V(3,5): the
    pre-smoothing is one mode-2 pair, the post-smoothing a pair after a pair; V(5,4): a general pair in the
    pre-smoothing, whose result the post-smoothing's pair then starts from."""
    mesh = mesh_of(key)
    tol = R.config_tol(name)
    a = R.mg_context(mesh, tol, device=0)
    monkeypatch.setenv("PUCFEM_MG_PAIR", "0")
    b = R.mg_context(mesh, tol, device=0)
    rng = np.random.default_rng(7)
    r, x = rng.standard_normal(mesh.N), rng.standard_normal(mesh.N)
    lv = mesh.levels
    for piece, kw in (("smooth0", dict(b=r)), ("smoothx", dict(b=r, x=x)), ("cycle", dict(b=r)),
                      ("precondition", dict(b=r))):
        ya, yb = a.mg_probe(piece, lv, **kw), b.mg_probe(piece, lv, **kw)
        if piece == "precondition":
            assert ya[1] == yb[1]
            ya, yb = ya[0], yb[0]
        assert np.abs(ya).max() > 0
        assert np.array_equal(ya, yb), (piece, int((ya != yb).sum()), R.relmax(ya, yb))
    assert a.path_info()["mg_step_pairs"] and not b.path_info()["mg_step_pairs"]
    a.close()
    b.close()


# ---- e. the operator the PCG needs: symmetric and positive
@pytest.mark.parametrize("name,single", [(n, True) for n in sorted(R.CONFIGS) if n not in ("d3p5", "d5p4")] +
                         [("d3p3", False)])
def test_preconditioner_is_symmetric_positive(world, name, single):
    """<y, M^-1 x> = <x, M^-1 y> within 8 times the defect of the reference's restatement in the cycle's precision
    (floor 1e-12 for the fp64 cycle), and <x, M^-1 x> > 0.  (Unequal pre- and post-smoothing is not symmetric by
    construction: those configurations are not here.)"""
    ctx, ref, r32 = world.get("s6", name, single)
    x, y = R.level_vectors(ref, ref.levels, 8)
    mx, _ = ctx.mg_probe("precondition", ref.levels, b=x)
    my, _ = ctx.mg_probe("precondition", ref.levels, b=y)
    q = r32 if single else ref
    rx, ry = q.precondition(x).astype(np.float64), q.precondition(y).astype(np.float64)
    scale = np.linalg.norm(x) * np.linalg.norm(my)
    d_dev = abs(y @ mx - x @ my) / scale
    d_ref = abs(y @ rx - x @ ry) / scale
    print(f"{name} {'fp32' if single else 'fp64'}: symmetry defect device {d_dev:.3e}, restatement {d_ref:.3e}")
    assert d_dev <= max(FACTOR * d_ref, 0.0 if single else 1e-12), (d_dev, d_ref)
    assert x @ mx > 0 and y @ my > 0


# ---- f. the lattice operators through pucfem_apply
@pytest.mark.parametrize("key", ["s6", "fine3"])
def test_lattice_operators_against_the_csr(world, key):
    ctx, ref, _ = world.get(key, "d3p3", True)
    assert ctx.path_info()["lattice"]
    N = ref.n[-1]
    rng = np.random.default_rng(9)
    x, u = rng.standard_normal(N), rng.standard_normal((N, 2))
    K, Av = ctx.host_csr(L.OP_K), ctx.host_csr(L.OP_VISC)
    Gx, Gy = ctx.host_csr(L.OP_GX), ctx.host_csr(L.OP_GY)
    s = 1.0 / (ctx.host_csr(L.OP_ASUM).diagonal() + 1e-12)  # the lumped scaling (StokesColor.py:130-165, 224-263)
    want = {
        "K": (L.OP_K, x, K @ x),
        "pressure": (L.OP_PRES, x, ref.shared["A"][-1] @ x),
        "A_visc": (L.OP_VISC, x, Av @ x),
        "divergence": (L.OP_DIV, u, s * (Gx @ u[:, 0] + Gy @ u[:, 1])),
        "gradient": (L.OP_GRAD, x, np.stack([s * (Gx @ x), s * (Gy @ x)], 1)),
        "curl": (L.OP_CURL, u, s * (Gx @ u[:, 1] - Gy @ u[:, 0])),
    }
    for name, (op, v, w) in want.items():
        e = R.relmax(ctx.apply(op, v, w.shape), w)
        print(f"{key} {name}: {e:.3e}")
        assert e <= 1e-12, (name, e)


# ---- g. the probe leaves a run as it found it
def test_probe_does_not_disturb_a_run():
    mesh = pf.load_mesh("fine", refine=3)
    tol = S.Tolerances.production()
    a = S.StokesSimulation(mesh, S.SquirmerBC(nu=0.1), 0.05, "color", 0, tol)
    b = S.StokesSimulation(mesh, S.SquirmerBC(nu=0.1), 0.05, "color", 0, tol)
    lv = mesh.levels
    sizes = [a.ctx.mg_level_size(l) for l in range(lv + 1)]
    rng = np.random.default_rng(10)
    sa, sb = [], []
    for _ in range(3):
        sa += a.step(2)
        sb += b.step(2)
        for l in range(1, lv + 1):
            v, w, vc = rng.standard_normal(sizes[l]), rng.standard_normal(sizes[l]), rng.standard_normal(sizes[l - 1])
            a.ctx.mg_probe("resid", l, b=v, x=w)
            a.ctx.mg_probe("smooth0", l, b=v)
            a.ctx.mg_probe("smoothx", l, b=v, x=w)
            a.ctx.mg_probe("restrict", l, x=w)
            a.ctx.mg_probe("prolong", l, b=vc, x=w)
            a.ctx.mg_probe("cycle", l, b=v)
        a.ctx.mg_probe("coarse", 0, b=rng.standard_normal(sizes[0]))
        a.ctx.mg_probe("precondition", lv, b=rng.standard_normal(sizes[lv]))
    assert [(s.it_visc, s.it_p, s.it_p2) for s in sa] == [(s.it_visc, s.it_p, s.it_p2) for s in sb]
    assert np.array_equal(a.u, b.u) and np.array_equal(a.c, b.c)
    assert np.array_equal(a.field(L.F_P), b.field(L.F_P))
    a.close()
    b.close()
