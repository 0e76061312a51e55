"""Round trips through the entry points' numbering-and-transfer layer (Ctx::put / Ctx::get, Ctx::formed and the shared
tracer I/O of pucfem_api.hip): what is set is read back bit for bit, on the dense path (mesh1, 331 nodes), on SELL rows
(fine, 1067 nodes) and on a refined lattice where the step keeps p in y (fine x2, production tolerances); the fields
formed when read come out the same twice and forming them for a sampler leaves the run alone; an ensemble's members
are planes of the same layer; two ranks serve their owned windows.  tests/test_numbering_host.py checks the host
helpers underneath against a restatement."""
import os
import threading

import numpy as np
import pytest

from conftest import has_gpu, load_pkg

pytestmark = pytest.mark.gpu

pf = load_pkg()
from importlib import import_module  # noqa: E402

L = import_module("puc-fluidsimulation-project_amd._lib")
S = import_module("puc-fluidsimulation-project_amd.solver")

MESHES = ["mesh1", "fine", "lat"]
FORMED = [("p", L.F_P), ("p2", L.F_P2), ("div_star", L.F_DIV_STAR), ("final_div", L.F_FINAL_DIV), ("vorticity", L.F_VORTICITY)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not has_gpu():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def make_sim(name, steps=2):
    if name == "lat":
        mesh, tol = pf.load_mesh("fine", refine=2), S.Tolerances.production()
    else:
        mesh, tol = pf.load_mesh(name), None
    sim = S.StokesSimulation(mesh, S.SquirmerBC(), 0.05, "color", 0, tol=tol)
    sim.step(steps)
    return sim


def check_paths(name, sim):
    info = sim.ctx.path_info()
    assert info["pending_pressure_directions"] == (name == "lat")  # (p_from_y: p and p2 are formed when read)
    assert info["lattice"] == (name == "lat")
    assert info["pressure"] == ("mg-pcg" if name == "lat" else "dense")  # (mesh1 and fine: dense solves, SELL rows)


@pytest.fixture(scope="module")
def twins():
    """Per mesh, two identical runs after two steps (the second stays untouched by the samplers)."""
    d = {n: (make_sim(n), make_sim(n)) for n in MESHES}
    for n, (a, _) in d.items():
        check_paths(n, a)
    yield d
    for a, b in d.values():
        a.close()
        b.close()


def bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("name", MESHES)
def test_formed_fields_read_the_same_twice(twins, name):
    a, b = twins[name]
    for fname, f in FORMED:
        x, y = a.field(f), a.field(f)
        assert x.shape == (a.mesh.N,) and np.isfinite(x).all(), fname
        assert bits(x) == bits(y), fname
        assert bits(x) == bits(b.field(f)), fname
    assert np.abs(a.field(L.F_P)).max() > 0 and np.abs(a.field(L.F_VORTICITY)).max() > 0.1


@pytest.mark.parametrize("name", MESHES)
def test_sampling_formed_fields_leaves_the_run_alone(twins, name):
    a, b = twins[name]
    names = tuple(n for n, _ in FORMED)
    img = a.raster(31, 23, fields=names)
    vals, tri = a.sample(a.mesh.coords[::7] * 0.999 + 0.0005, fields=names)
    assert list(img) == list(names) and (tri >= 0).sum() > 10
    for n, f in FORMED:  # the nodal field at (almost) the nodes: the samplers read what get_field reads
        assert np.nanmax(np.abs(vals[n])) <= np.abs(a.field(f)).max() * (1 + 1e-12), n
    a.step(1)
    b.step(1)
    assert bits(a.u) == bits(b.u) and bits(a.c) == bits(b.c)
    assert bits(a.field(L.F_P)) == bits(b.field(L.F_P)) and bits(a.field(L.F_P2)) == bits(b.field(L.F_P2))


@pytest.mark.parametrize("name", MESHES)
def test_set_then_get_is_bit_identical(name):
    sim = make_sim(name, steps=1)
    try:
        check_paths(name, sim)
        N, ctx = sim.mesh.N, sim.ctx
        rng = np.random.default_rng(11)
        for f, shape in ((L.F_U, (N, 2)), (L.F_USTAR, (N, 2)), (L.F_C, (N,))):
            x = rng.standard_normal(shape)
            ctx.set_field(f, x)
            assert bits(ctx.get_field(f, shape)) == bits(x), f
        d = rng.standard_normal((3, N))
        sim.dyes = d
        assert bits(sim.dyes) == bits(d)
        one = rng.standard_normal(N)
        ctx.set_field(L.F_DYE0 + 1, one)  # one channel alone, its neighbours untouched
        assert bits(ctx.get_field(L.F_DYE0 + 1, (N,))) == bits(one)
        d[1] = one
        assert bits(sim.dyes) == bits(d)
        assert bits(ctx.get_field(L.F_DYE0 + 2, (N,))) == bits(d[2])
        for n in (0, 1, 257):
            pts = 0.1 + 0.8 * rng.random((n, 2))
            ctx.set_field(L.F_TRACERS, pts)
            assert bits(ctx.get_field(L.F_TRACERS, (n, 2))) == bits(pts), n
            assert bits(ctx.get_field(L.F_STATUS, (n,))) == bits(np.zeros(n)), n
            assert bits(ctx.get_field(L.F_CAPTURE_STEP, (n,))) == bits(np.full(n, -1.0)), n
            st = (rng.random(n) < 0.5).astype(np.float64)
            ctx.set_field(L.F_STATUS, st)
            assert bits(ctx.get_field(L.F_STATUS, (n,))) == bits(st), n
    finally:
        sim.close()


def test_heat_scalar_round_trip():
    sim = S.HeatSimulation(pf.load_mesh("mesh1"))
    try:
        x = np.random.default_rng(12).standard_normal(sim.mesh.N)
        sim.ctx.set_field(L.F_SCALAR, x)
        assert bits(sim.u) == bits(x)
    finally:
        sim.close()


def test_ensemble_members_are_planes():
    mesh = pf.load_mesh("mesh1")
    N, M = mesh.N, 3
    ens = S.StokesEnsemble(mesh, [S.SquirmerBC(B1=-2.0, B2=b2) for b2 in (0.0, -5.0, 5.0)], 0.05, "color")
    try:
        ens.step(1)
        rng = np.random.default_rng(13)
        for f, nc in ((L.F_U, 2), (L.F_USTAR, 2), (L.F_P, 1), (L.F_P2, 1), (L.F_C, 1)):
            shape = (N, 2) if nc == 2 else (N,)
            x = rng.standard_normal((M,) + shape)
            ens.set(f, x)  # member = -1
            assert bits(ens.get(f, nc)) == bits(x), f
            one = rng.standard_normal(shape)
            ens.set(f, one, member=1)
            assert bits(ens.get(f, nc, member=1)) == bits(one), f
            x[1] = one
            assert bits(ens.get(f, nc)) == bits(x), f  # the other members' bits are as they were
    finally:
        ens.close()
    food = S.StokesEnsemble(mesh, [S.SquirmerBC(B1=-2.0, B2=b2, nu=1.0) for b2 in (0.0, -5.0, 5.0)], 0.01, "food",
                            tracers=0.2 + 0.6 * np.random.default_rng(14).random((257, 2)))
    try:
        food.step(1)
        rng = np.random.default_rng(15)
        t = 0.2 + 0.6 * rng.random((M, 257, 2))
        food.set(L.F_TRACERS, t)
        assert bits(food.tracers) == bits(t)
        st = (rng.random((M, 257)) < 0.5).astype(np.float64)
        food.set(L.F_STATUS, st)
        one = 0.2 + 0.6 * rng.random((257, 2))
        food.set(L.F_TRACERS, one, member=2)  # resets member 2 alone
        t[2], st[2] = one, 0.0
        assert bits(food.tracers) == bits(t) and bits(food.get(L.F_TRACERS, 1, member=2)) == bits(one)
        assert bits(food.get(L.F_STATUS)) == bits(st)
        assert bits(food.get(L.F_CAPTURE_STEP)) == bits(np.full((M, 257), -1.0))
    finally:
        food.close()


def test_two_ranks_serve_their_owned_windows():
    """PUCFEM-LOCALCOMM, two host threads, fine x2 (built as test_gpu_vorticity's two-rank case): the ranks' owned rows
    of U and of P together equal the single-rank fields bit for bit.  The comparison is of the transfer, so it is made
    on a state all three contexts hold exactly -- U set from one array, P as the build leaves it (formed from y where
    the step keeps it there): after a step the ranks differ from a single rank by their summation order
    (tests/test_gpu_multirank.py).  Every stage waits under its own time limit."""
    mesh = pf.load_mesh("fine", refine=2)
    tol = pf.Tolerances(rtol_pres=1e-12, rtol_visc=1e-13)
    x = np.random.default_rng(16).standard_normal((mesh.N, 2))
    world = 2
    uid = b"PUCFEM-LOCALCOMM" + os.urandom(112)
    stages = ("build", "set", "read")
    done = {s: [threading.Event() for _ in range(world)] for s in stages}
    out, errs = [dict() for _ in range(world)], []

    def read(sim):
        got = {}
        for k, f, shape in (("u", L.F_U, (mesh.N, 2)), ("p", L.F_P, (mesh.N,))):
            v = np.full(shape, np.nan)
            L.check(sim.ctx.L.pucfem_get_field(sim.ctx.h, f, L.dptr(v), v.size), sim.ctx.h)
            got[k] = v
        return got

    def worker(r):
        sim = None
        try:
            sim = pf.StokesSimulation(mesh, pf.SquirmerBC(), 0.05, "color", device=0, tol=tol, dist=(r, world, uid))
            done["build"][r].set()
            sim.u = x
            done["set"][r].set()
            out[r].update(read(sim), info=sim.ctx.info())
        except Exception as e:  # reported below
            errs.append((r, repr(e)))
        finally:
            for s in stages:  # (a failed rank keeps nobody waiting)
                done[s][r].set()
            if sim is not None and not errs:
                sim.close()

    th = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for s, limit in zip(stages, (120, 60, 60)):
        for r in range(world):
            assert done[s][r].wait(timeout=limit), f"rank {r}: stage {s!r} did not finish in {limit} s"
            assert not errs, errs
    for t in th:
        t.join(timeout=60)
        assert not t.is_alive()
    assert not errs, errs
    single = pf.StokesSimulation(mesh, pf.SquirmerBC(), 0.05, "color", device=0, tol=tol)
    try:
        single.u = x
        ref = read(single)
    finally:
        single.close()
    assert bits(ref["u"]) == bits(x)
    own = [~np.isnan(o["p"]) for o in out]
    assert np.array_equal(own[0], ~own[1]) and [int(m.sum()) for m in own] == [o["info"]["n_own"] for o in out]
    for k in ("u", "p"):
        for o, m in zip(out, own):
            assert np.array_equal(~np.isnan(o[k]).reshape(mesh.N, -1).any(axis=1), m), k
        whole = np.where(own[0].reshape((-1,) + (1,) * (ref[k].ndim - 1)), out[0][k], out[1][k])
        assert bits(whole) == bits(ref[k]), k
