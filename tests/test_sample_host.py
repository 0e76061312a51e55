"""Sampling and rasterising, host side (no device): the brute-force restatement of the samplers' semantics that the
GPU tests compare with bit for bit (tests/test_gpu_sample.py imports it from here), the recorder's raster mode on a
stub simulation, and the refusal of the three calls on a host-only context.

Semantics (include/pucfem.h, pucfem_sample.hpp): for a point q, among ALL triangles that pass the reference's
weight test (|det| >= 1e-14, w1, w2, w3 >= 0 formed as StokesColor.py:325-333) the one with the smallest
(squared centroid distance, triangle id); the value is the reference's interpolation with periodic x differences
(StokesColor.py:374-386); no passing triangle: NaN, triangle -1.  Every expression below is written in the
library's operation order, so with its unfused fp64 arithmetic the two agree to the bit."""
import ctypes as ct
import os

import numpy as np
import pytest

import oracle as O
from conftest import load_pkg

pf = load_pkg()
from importlib import import_module  # noqa: E402

L = import_module("puc-fluidsimulation-project_amd._lib")
F = import_module("puc-fluidsimulation-project_amd.frames")


def _pdx(a, b):
    d = a - b
    d = np.where(d > 0.5, d - 1.0, d)
    return np.where(d < -0.5, d + 1.0, d)


def brute_locate(X, T, P, chunk=512):
    """Triangle of every point of P (n, 2) by the weight test over all triangles, min (d^2, id); -1: none.
    Also the number of passing triangles and the located triangle's smallest weight.
    The only shortcut: the points are taken in strips of `chunk` (by y, then x), and a strip skips the triangles
    whose bounding box is more than 1e-6 away from the strip's -- a point that passes a triangle's weight test
    lies in it up to rounding (~1e-14 here), so none of those can pass.  The kept triangles stay in id order."""
    x1, y1, x2, y2, x3, y3 = (X[T[:, 0], 0], X[T[:, 0], 1], X[T[:, 1], 0], X[T[:, 1], 1], X[T[:, 2], 0],
                              X[T[:, 2], 1])
    txlo, txhi = np.minimum(np.minimum(x1, x2), x3), np.maximum(np.maximum(x1, x2), x3)
    tylo, tyhi = np.minimum(np.minimum(y1, y2), y3), np.maximum(np.maximum(y1, y2), y3)
    tri = -np.ones(len(P), dtype=np.int32)
    npass = np.zeros(len(P), dtype=np.int64)
    wmin = np.full(len(P), np.inf)
    fin = np.where(np.isfinite(P).all(axis=1))[0]  # (a non-finite point passes nowhere)
    fin = fin[np.lexsort((P[fin, 0], P[fin, 1]))]
    eps = 1e-6
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for s in range(0, len(fin), chunk):
            idx = fin[s:s + chunk]
            qx, qy = P[idx, 0:1], P[idx, 1:2]
            k = np.where((txhi >= qx.min() - eps) & (txlo <= qx.max() + eps) & (tyhi >= qy.min() - eps) &
                         (tylo <= qy.max() + eps))[0]
            if len(k) == 0:
                continue
            a1, b1, a2, b2, a3, b3 = x1[k], y1[k], x2[k], y2[k], x3[k], y3[k]
            det = (a2 - a1) * (b3 - b1) - (a3 - a1) * (b2 - b1)
            w1 = ((a2 - qx) * (b3 - qy) - (a3 - qx) * (b2 - qy)) / det
            w2 = ((a3 - qx) * (b1 - qy) - (a1 - qx) * (b3 - qy)) / det
            w3 = 1.0 - w1 - w2
            ps = (np.abs(det) >= 1e-14) & (w1 >= 0.0) & (w2 >= 0.0) & (w3 >= 0.0)
            dx, dy = (a1 + a2 + a3) / 3.0 - qx, (b1 + b2 + b3) / 3.0 - qy
            d = np.where(ps, dx * dx + dy * dy, np.inf)
            best = np.argmin(d, axis=1)  # the first minimum: the smallest id among equal distances
            found = ps.any(axis=1)
            tri[idx] = np.where(found, k[best], -1)
            npass[idx] = ps.sum(axis=1)
            rows = np.arange(len(best))
            wmin[idx] = np.where(found, np.minimum(np.minimum(w1[rows, best], w2[rows, best]), w3[rows, best]), np.inf)
    return tri, npass, wmin


def brute_value(X, T, P, tri, f):
    """The reference's interpolation of the nodal field f (N,) in triangle tri[e] at P[e]; NaN where tri < 0."""
    t = np.where(tri >= 0, tri, 0)
    a, b, d = T[t, 0], T[t, 1], T[t, 2]
    x1, y1, x2, y2, x3, y3 = X[a, 0], X[a, 1], X[b, 0], X[b, 1], X[d, 0], X[d, 1]
    xb, yb = P[:, 0], P[:, 1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        det = _pdx(x2, x1) * (y3 - y1) - _pdx(x3, x1) * (y2 - y1)
        w1 = (_pdx(x2, xb) * (y3 - yb) - _pdx(x3, xb) * (y2 - yb)) / det
        w2 = (_pdx(x3, xb) * (y1 - yb) - _pdx(x1, xb) * (y3 - yb)) / det
        w3 = 1.0 - w1 - w2
        v = w1 * f[a] + w2 * f[b] + w3 * f[d]
    return np.where(tri >= 0, v, np.nan)


def brute_sample(X, T, P, fields):
    """({name: values}, tri) of nodal fields {name: (N,) or (N, 2)} at P, as Context.sample returns them."""
    tri, _, _ = brute_locate(X, T, P)
    out = {}
    for k, f in fields.items():
        f = np.asarray(f, dtype=np.float64)
        out[k] = brute_value(X, T, P, tri, f) if f.ndim == 1 else np.stack(
            [brute_value(X, T, P, tri, np.ascontiguousarray(f[:, q])) for q in range(f.shape[1])], 1)
    return out, tri


@pytest.mark.parametrize("name", ["mesh1", "fine"])
def test_brute_force_against_the_oracle(name):
    """The helper against oracle.locate_bary + oracle.plane_coefficients at the 48 x 40 pixel centres of the unit
    window: the same found mask and triangles (1540 found, 380 not; no centre passes in two triangles, so the
    min-key rule is idle here), values within 1e-12 of the plane form for a field of O(1) -- different arithmetic,
    so a sanity bound on the helper, not on the device."""
    mesh = pf.load_mesh(name)
    X, T = mesh.coords, mesh.triangles
    P = pf.pixel_centres(48, 40)
    assert P.shape == (1920, 2) and P[0, 0] == 0.5 / 48 and P[0, 1] == 0.5 / 40 and P[1, 1] == P[0, 1]
    tri, npass, wmin = brute_locate(X, T, P)
    ref = O.locate_bary(X, T, P[:, 0], P[:, 1])
    assert np.array_equal(tri >= 0, ref >= 0)
    assert int((tri >= 0).sum()) == 1540 and int((tri < 0).sum()) == 380
    assert npass.max() == 1
    assert np.array_equal(tri, ref.astype(np.int32))
    assert wmin.min() > 1e-6
    z = np.sin(3.0 * X[:, 0]) + np.cos(2.0 * X[:, 1])
    val = brute_value(X, T, P, tri, z)
    pc = O.plane_coefficients(X, T, z)
    hit = tri >= 0
    plane = pc[tri[hit], 0] * P[hit, 0] + pc[tri[hit], 1] * P[hit, 1] + pc[tri[hit], 2]
    assert np.all(np.isnan(val[~hit]))
    assert np.abs(val[hit] - plane).max() <= 1e-12


def test_brute_force_min_key_on_shared_vertices():
    """Two triangles sharing an edge, the second listed twice (dyadic coordinates: every weight below is exact).
    The edge's midpoint passes in all three and takes the nearer centroid, not the smaller id; equal distances
    take the smaller id; NaN and outside points find none."""
    X = np.array([[0.0, 0.0], [0.375, 0.0], [0.0, 0.375], [0.375, 0.75]])
    T = np.array([[1, 3, 2], [0, 1, 2], [0, 1, 2]], dtype=np.int32)
    P = np.array([[0.1875, 0.1875], [0.125, 0.125], [0.25, 0.375], [2.0, 2.0], [np.nan, 0.5]])
    tri, npass, _ = brute_locate(X, T, P)
    assert list(npass) == [3, 2, 1, 0, 0]
    assert list(tri) == [1, 1, 0, -1, -1]
    v = brute_value(X, T, P, tri, X[:, 0] + 2.0 * X[:, 1])
    assert v[0] == 0.5625 and abs(v[1] - 0.375) < 1e-15 and abs(v[2] - 1.0) < 1e-15
    assert np.isnan(v[3]) and np.isnan(v[4])


class RasterSim:
    """The StokesSimulation surface the recorder's raster mode uses; the images encode the step index."""

    scheme = "color"

    def __init__(self):
        self.step_count = 0
        self.calls = []
        self.rasters = []

    def step(self, n):
        self.calls.append(n)
        self.step_count += n
        return [object()] * n

    @property
    def c(self):
        raise AssertionError("the raster mode reads no nodal field")

    u = c

    def raster(self, width, height, fields=("c", "u"), window=None):
        self.rasters.append((width, height, tuple(fields), window))
        k = float(self.step_count - 1)
        x = (np.arange(width, dtype=np.float32) + 0.5) / width
        c = np.tile(x, (height, 1)) * np.float32(0.5) + np.float32(k / 1000.0)
        c[height // 2, width // 2] = np.nan  # (a pixel inside the swimmer)
        u = np.stack([np.full((height, width), k, dtype=np.float32), np.tile(x, (height, 1))])
        u[:, height // 2, width // 2] = np.nan
        return {"c": c, "u": u}


def test_recorder_raster_mode(tmp_path):
    sim = RasterSim()
    win = (0.25, 0.25, 0.75, 0.75)
    rec = pf.FrameRecorder(None, interval=50, raster=(16, 12), window=win)
    st = rec.run(sim, 120)
    assert len(st) == 120 and rec.steps == [0, 50, 100] and sim.calls == [1, 50, 50, 19]
    assert sim.rasters == [(16, 12, ("c", "u"), win)] * 3
    for k, c, u in zip(rec.steps, rec.dye, rec.vel):
        assert c.dtype == np.float32 and c.shape == (12, 16) and u.dtype == np.float32 and u.shape == (2, 12, 16)
        assert np.nanmin(u[0]) == k and np.nanmax(u[0]) == k
    p = str(tmp_path / "raster.npz")
    pf.save_npz(rec, p)
    d = pf.load_npz(p)
    assert sorted(d) == ["dye", "steps", "vel", "window"]
    np.testing.assert_array_equal(d["steps"], [0, 50, 100])
    np.testing.assert_array_equal(d["window"], win)
    assert d["dye"].dtype == np.float32 and d["vel"].dtype == np.float32
    np.testing.assert_array_equal(d["dye"], np.stack(rec.dye))
    np.testing.assert_array_equal(d["vel"], np.stack(rec.vel))
    # the unit window is written out when none was given
    rec0 = pf.FrameRecorder(None, interval=1, raster=(4, 3))
    rec0.run(RasterSim(), 1)
    pf.save_npz(rec0, p)
    np.testing.assert_array_equal(pf.load_npz(p)["window"], [0.0, 0.0, 1.0, 1.0])


def test_recorder_default_mode_untouched(tmp_path):
    """Without raster= the recorder reads sim.c / sim.u and writes the mesh, as before."""
    mesh = pf.load_mesh("mesh1")

    class Sim:
        scheme = "color"
        step_count = 0

        def step(self, n):
            self.step_count += n
            return [None] * n

        c = property(lambda s: np.full(mesh.N, 0.25))
        u = property(lambda s: np.full((mesh.N, 2), float(s.step_count - 1)))

        def raster(self, *a, **k):
            raise AssertionError("the default mode does not rasterise")

    rec = pf.FrameRecorder(mesh, interval=2)
    assert rec.raster is None and rec.window is None
    rec.run(Sim(), 5)
    assert rec.steps == [0, 2, 4] and rec.dye[0].shape == (mesh.N,) and rec.vel[1].shape == (mesh.N, 2)
    assert rec.dye[0].dtype == np.float32 and np.all(rec.vel[2] == 4.0)
    p = str(tmp_path / "nodal.npz")
    pf.save_npz(rec, p)
    d = pf.load_npz(p)
    assert sorted(d) == ["coords", "dye", "steps", "triangles", "vel"]
    assert d["dye"].shape == (3, mesh.N) and d["vel"].shape == (3, mesh.N, 2)


def test_render_raster_frames(tmp_path):
    pytest.importorskip("matplotlib")
    rec = pf.FrameRecorder(None, interval=1, raster=(16, 12))
    sim = RasterSim()
    rec.run(sim, 2)
    assert len(rec) == 2
    pngs = pf.render(rec, str(tmp_path / "png"), dpi=60)
    assert len(pngs) == 2 and all(os.path.getsize(q) > 1000 for q in pngs)


def test_host_only_context_refuses():
    """No device: the three calls fail with PUCFEM_ENODEV (there is no CPU fallback)."""
    lib = L.lib()
    p = ct.c_void_p()
    L.check(lib.pucfem_ctx_create(L.HOST_ONLY, ct.byref(p)))
    try:
        fields = np.array([L.F_C], dtype=np.int32)
        xy = np.array([[0.1, 0.1]])
        out = np.zeros(1)
        tri = np.zeros(1, dtype=np.int32)
        img = np.zeros((1, 2, 2), dtype=np.float32)
        assert lib.pucfem_sample_points(p, 1, L.iptr(fields), 1, L.dptr(xy), L.dptr(out), L.iptr(tri)) == -7
        assert b"host-only" in lib.pucfem_last_error(p)
        assert lib.pucfem_raster(p, 1, L.iptr(fields), 2, 2, None, L.fptr(img)) == -7
        assert lib.pucfem_ens_raster(p, 1, L.iptr(fields), -1, 2, 2, None, L.fptr(img)) == -7
    finally:
        L.check(lib.pucfem_ctx_destroy(p))
