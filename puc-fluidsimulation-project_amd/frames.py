"""Frame / field export for visualisation (scripts/good_visualization2.py:536-571,
:724-747).  Host side only: the fields are copied off the GPU at the recorded steps.

The reference keeps a copy of the dye and the velocity every ``frame_interval`` (50) steps, then
animates a gouraud ``tripcolor`` of the dye (magma, [0, 1]) under a ``quiver`` of every ``skip``-th
node's velocity, titled "Fluid Simulation - Step k", and saves it with ffmpeg at 20 fps, 150 dpi.
``FrameRecorder`` does the same around a ``StokesSimulation``; ``render`` writes the animation with
ffmpeg when it is installed, else an animated GIF (Pillow) or a PNG sequence; ``save_npz`` /
``load_npz`` keep the raw frames and ``write_vtk`` writes one frame as a legacy VTK unstructured grid
(ParaView / VisIt), which needs no plotting stack at all.

``FrameRecorder(mesh, interval, raster=(W, H))`` records images rasterised on the device instead
(``StokesSimulation.raster``): no field leaves the GPU, and ``render`` draws them with ``imshow`` -- the
way to frames of a mesh whose triangles no plotting library draws (L7: 28M).

``FrameRecorder(..., streamlines=dict(seeds=..., h=..., nsteps=...))`` also records the streamlines of every
recorded frame (``StokesSimulation.streamlines``, integrated on the device); ``render`` draws them over the dye.
"""
from __future__ import annotations

import os
import shutil

import numpy as np

from ._lib import LOADS_KEYS


class FrameRecorder:
    """Record (step, dye, velocity) every `interval` steps of a simulation (fp32 copies by default,
    half the host memory of the reference's fp64 lists).

    raster=(W, H): record W x H images instead of the nodal fields -- ``sim.raster`` rasterises the dye and the
    velocity of `window` = (x0, y0, x1, y1) (None: the unit square) on the device, so a frame costs its pixels
    at any mesh size and the fields are never copied.  ``dye`` then holds float32 (H, W) images and ``vel``
    (2, H, W) ones (row 0 the lowest y, NaN inside the swimmer).

    vorticity=True: each frame also appends the vorticity to ``vort`` -- the reference's second panel
    (scripts/good_visualization.py:578-584), formed on the device: the (H, W) raster of "vorticity" in raster
    mode, else the nodal field ``sim.vorticity``.

    streamlines=dict(seeds=..., h=..., nsteps=..., **options of StokesSimulation.streamlines): each frame also
    appends the lines' points (lines, nsteps + 1, 2) to ``lines`` and their point counts to ``lines_npts`` -- the
    reference's streamplot (stokes_flow.py:536) of the frame's velocity.  Off by default.

    dyes=True: each frame also appends the simulation's dye channels (``StokesSimulation.dyes``) to ``dyes``, the way
    the dye is recorded: a copy (K, N) of the channels, or in raster mode one image per channel (K, H, W), rasterised
    as "dye0" .. in the frame's raster call.  dyes= may also name the channels to record ("dye0", 2, ...).

    loads=True: each frame also appends the swimmer's ten loads of the frame's state (``sim.swimmer_loads()``: one
    launch, ten doubles copied) to ``loads``, in LOADS_KEYS' order.  Off by default."""

    def __init__(self, mesh, interval=50, dtype=np.float32, raster=None, window=None, vorticity=False,
                 streamlines=None, dyes=False, loads=False):
        self.mesh = mesh
        self.interval = int(interval)
        self.dtype = dtype
        self.raster = None if raster is None else (int(raster[0]), int(raster[1]))
        self.window = None if window is None else tuple(float(v) for v in window)
        self.steps: list[int] = []
        self.dye: list[np.ndarray] = []
        self.vel: list[np.ndarray] = []
        self.vorticity = bool(vorticity)
        self.vort: list[np.ndarray] = []
        self.streamlines = None
        if streamlines is not None:
            opts = dict(streamlines)
            missing = [k for k in ("seeds", "h", "nsteps") if k not in opts]
            if missing:
                raise ValueError(f"streamlines= needs seeds, h and nsteps (missing: {missing})")
            if opts.get("fields"):
                raise ValueError("the recorder keeps the lines' points, not fields along them")
            opts["seeds"] = np.array(opts["seeds"], dtype=np.float64).reshape(-1, 2)
            self.streamlines = opts
        self.lines: list[np.ndarray] = []
        self.lines_npts: list[np.ndarray] = []
        # True: every channel of the simulation; else the recorded channels' indices
        self.dye_channels = dyes if isinstance(dyes, bool) else _dye_indices(dyes)
        self.dyes: list[np.ndarray] = []
        self.record_swimmer_loads = bool(loads)
        self.loads: list[np.ndarray] = []

    def _channels(self, sim):
        """The indices of the channels to record from `sim`."""
        if self.dye_channels is True:
            return list(range(sim.dyes_info()[0]))
        return list(self.dye_channels or ())

    def record_lines(self, sim):
        """The streamlines of `sim`'s current velocity, for the frame just recorded."""
        sl = sim.streamlines(**self.streamlines)
        self.lines.append(np.array(sl.points, dtype=np.float64, copy=True))
        self.lines_npts.append(np.array(sl.npts, dtype=np.int32, copy=True))

    def record(self, step, c, u, vort=None):
        self.steps.append(int(step))
        self.dye.append(np.array(c, dtype=self.dtype, copy=True) if c is not None else None)
        self.vel.append(np.array(u, dtype=self.dtype, copy=True))
        if vort is not None:
            self.vort.append(np.array(vort, dtype=self.dtype, copy=True))

    def record_raster(self, step, sim):
        """One raster frame of `sim` (its dye only under scheme 'color')."""
        W, H = self.raster
        color = sim.scheme == "color"
        fields = (("c", "u") if color else ("u",)) + (("vorticity",) if self.vorticity else ())
        chans = [f"dye{k}" for k in self._channels(sim)] if self.dye_channels else []
        img = sim.raster(W, H, fields=fields + tuple(chans), window=self.window)
        if self.dye_channels:
            self.dyes.append(np.stack([np.asarray(img[f], dtype=np.float32) for f in chans]) if chans
                             else np.zeros((0, H, W), dtype=np.float32))
        self.steps.append(int(step))
        self.dye.append(np.asarray(img["c"], dtype=np.float32) if color else None)
        self.vel.append(np.asarray(img["u"], dtype=np.float32))
        if self.vorticity:
            self.vort.append(np.asarray(img["vorticity"], dtype=np.float32))

    def run(self, sim, steps):
        """Step `sim` (a StokesSimulation) `steps` times, recording the state after every step whose
        index is a multiple of `interval` (good_visualization2.py:724).  Steps between two recorded
        ones run in one call (no host synchronisation per step).  Returns the per-step stats."""
        stats = []
        end = sim.step_count + steps
        while sim.step_count < end:
            k0 = sim.step_count
            r = -(-k0 // self.interval) * self.interval  # next recorded step index
            n = min(end, r + 1) - k0
            stats += sim.step(n)
            if sim.step_count - 1 == r:
                if self.raster is not None:
                    self.record_raster(r, sim)
                else:
                    self.record(r, sim.c if sim.scheme == "color" else None, sim.u,
                                sim.vorticity if self.vorticity else None)
                    if self.dye_channels:
                        self.dyes.append(np.array(sim.dyes[self._channels(sim)], dtype=self.dtype, copy=True))
                if self.streamlines is not None:
                    self.record_lines(sim)
                if self.record_swimmer_loads:
                    d = sim.swimmer_loads()
                    self.loads.append(np.array([d[k] for k in LOADS_KEYS]))
        return stats

    def __len__(self):
        return len(self.steps)


def _dye_indices(dyes):
    """The channel indices named by a recorder's dyes= list ("dye3" or 3)."""
    from .solver import dye_field
    from . import _lib

    out = []
    for f in ([dyes] if isinstance(dyes, (str, int, np.integer)) else list(dyes)):
        if isinstance(f, str):
            e = dye_field(f)
            if e is None:
                raise ValueError(f"unknown dye channel {f!r}: 'dye0' .. 'dye{_lib.MAX_DYES - 1}'")
            out.append(e - _lib.F_DYE0)
        else:
            if not 0 <= int(f) < _lib.MAX_DYES:
                raise ValueError(f"dye channel index {f} outside 0 .. {_lib.MAX_DYES - 1}")
            out.append(int(f))
    return out


def save_npz(rec: FrameRecorder, path):
    """The raw frames.  Raster frames: `vel` (frames, 2, H, W), `dye` (frames, H, W) and `window`
    (x0, y0, x1, y1) instead of the mesh.  A recorder with vorticity frames adds `vort` (frames, H, W) or
    (frames, N); one with streamlines `lines` (frames, lines, nsteps + 1, 2) and `lines_npts` (frames, lines); one
    with dye channels `dyes` (frames, K, N) or (frames, K, H, W); one with loads `loads` (frames, 10)."""
    if getattr(rec, "raster", None) is not None:
        W, H = rec.raster
        d = dict(steps=np.array(rec.steps), window=np.array(rec.window or (0.0, 0.0, 1.0, 1.0), dtype=np.float64),
                 vel=np.stack(rec.vel) if rec.vel else np.zeros((0, 2, H, W), dtype=np.float32))
    else:
        d = dict(steps=np.array(rec.steps), coords=rec.mesh.coords, triangles=rec.mesh.triangles,
                 vel=np.stack(rec.vel) if rec.vel else np.zeros((0, rec.mesh.N, 2)))
    if rec.dye and rec.dye[0] is not None:
        d["dye"] = np.stack(rec.dye)
    if getattr(rec, "vort", None):
        d["vort"] = np.stack(rec.vort)
    if getattr(rec, "lines", None):
        d["lines"] = np.stack(rec.lines)
        d["lines_npts"] = np.stack(rec.lines_npts)
    if getattr(rec, "dyes", None):
        d["dyes"] = np.stack(rec.dyes)
    if getattr(rec, "loads", None):
        d["loads"] = np.stack(rec.loads)
    np.savez_compressed(path, **d)


def load_npz(path):
    d = np.load(path)
    return {k: d[k] for k in d.files}


def write_vtk(path, coords, triangles, point_data: dict):
    """One frame as a legacy binary VTK unstructured grid: triangles (cell type 5), point scalars
    (1-component fields) and vectors (2-component fields, z = 0)."""
    X = np.asarray(coords, dtype=np.float64)
    T = np.asarray(triangles, dtype=np.int64)
    N, M = len(X), len(T)
    with open(path, "wb") as f:
        f.write(b"# vtk DataFile Version 3.0\npucfem frame\nBINARY\nDATASET UNSTRUCTURED_GRID\n")
        f.write(f"POINTS {N} double\n".encode())
        pts = np.zeros((N, 3), dtype=">f8")
        pts[:, :2] = X
        f.write(pts.tobytes())
        f.write(f"\nCELLS {M} {4 * M}\n".encode())
        cells = np.empty((M, 4), dtype=">i4")
        cells[:, 0] = 3
        cells[:, 1:] = T
        f.write(cells.tobytes())
        f.write(f"\nCELL_TYPES {M}\n".encode())
        f.write(np.full(M, 5, dtype=">i4").tobytes())
        f.write(f"\nPOINT_DATA {N}\n".encode())
        for name, a in point_data.items():
            a = np.asarray(a, dtype=np.float64)
            if a.ndim == 1:
                f.write(f"SCALARS {name} double 1\nLOOKUP_TABLE default\n".encode())
                f.write(a.astype(">f8").tobytes())
            else:
                v = np.zeros((N, 3), dtype=">f8")
                v[:, :2] = a
                f.write(f"VECTORS {name} double\n".encode())
                f.write(v.tobytes())
            f.write(b"\n")


def read_vtk_header(path):
    """(n_points, n_cells, field names) of a file written by write_vtk (tests, tools)."""
    with open(path, "rb") as f:
        data = f.read()
    n_pts = n_cells = None
    names = []
    i = 0
    while i < len(data):
        j = data.find(b"\n", i)
        line = data[i:j if j >= 0 else len(data)]
        tok = line.split()
        step = 0
        if tok[:1] == [b"POINTS"]:
            n_pts = int(tok[1])
            step = n_pts * 24
        elif tok[:1] == [b"CELLS"]:
            n_cells = int(tok[1])
            step = int(tok[2]) * 4
        elif tok[:1] == [b"CELL_TYPES"]:
            step = int(tok[1]) * 4
        elif tok[:1] == [b"SCALARS"]:
            names.append(tok[1].decode())
            j = data.find(b"\n", j + 1)  # LOOKUP_TABLE line
            step = n_pts * 8
        elif tok[:1] == [b"VECTORS"]:
            names.append(tok[1].decode())
            step = n_pts * 24
        if j < 0:
            break
        i = j + 1 + step
    return n_pts, n_cells, names


def render(rec: FrameRecorder, out, fps=20, dpi=150, skip=None):
    """Animate the recorded frames as the reference does (tripcolor of the dye + quiver of the
    velocity, good_visualization2.py:536-571).  out ending in .mp4 uses ffmpeg (if installed), .gif
    Pillow; a directory name writes frame_00000.png ...  Returns the written path(s).
    Raster frames are drawn with imshow (magma, [0, 1], origin lower, the window as extent) under a quiver
    of every `skip`-th pixel's velocity.  With vorticity frames (``rec.vort``) a second panel beside it shows them
    as the reference does (good_visualization.py:578-584: coolwarm, limits symmetric about 0 at the largest
    |vorticity| of the frames).  Recorded streamlines (``rec.lines``) are drawn over the dye panel, cut at the
    periodic wraps (streamline_segments)."""
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import matplotlib.tri as mtri
    from matplotlib import animation
    from matplotlib.collections import LineCollection

    from .solver import streamline_segments

    vort = getattr(rec, "vort", None) or None
    if vort:
        fig, (ax, ax2) = plt.subplots(1, 2, figsize=(16, 8))
        vmax = max(float(np.nanmax(np.abs(v))) for v in vort) + 1e-9
    else:
        fig, ax = plt.subplots(figsize=(8, 8))
    if getattr(rec, "raster", None) is not None:
        # raster frames: the dye image under a quiver of the velocity image on a coarse pixel stride; the
        # swimmer's NaN pixels stay transparent (the axes' grey shows) and carry no arrows
        W, H = rec.raster
        x0, y0, x1, y1 = rec.window or (0.0, 0.0, 1.0, 1.0)
        skip = skip or max(1, max(W, H) // 40)
        ax.set_facecolor("0.5")
        dye0 = rec.dye[0] if rec.dye and rec.dye[0] is not None else np.zeros((H, W), dtype=np.float32)
        tpc = ax.imshow(dye0, cmap="magma", vmin=0, vmax=1.0, origin="lower", extent=(x0, x1, y0, y1),
                        interpolation="nearest")
        px = x0 + (np.arange(W)[skip // 2::skip] + 0.5) * (x1 - x0) / W
        py = y0 + (np.arange(H)[skip // 2::skip] + 0.5) * (y1 - y0) / H

        def arrows(i):
            v = rec.vel[i][:, skip // 2::skip, skip // 2::skip]
            return np.ma.masked_invalid(v[0]), np.ma.masked_invalid(v[1])

        qv = ax.quiver(*np.meshgrid(px, py), *arrows(0), color="white", scale=20.0)
        ax.set_xlim(x0, x1)
        ax.set_ylim(y0, y1)
        if vort:
            ax2.set_facecolor("0.5")
            tpv = ax2.imshow(vort[0], cmap="coolwarm", vmin=-vmax, vmax=vmax, origin="lower", extent=(x0, x1, y0, y1),
                             interpolation="nearest")
    else:
        X, T = rec.mesh.coords, rec.mesh.triangles
        skip = skip or max(1, len(X) // 1500)
        tri = mtri.Triangulation(X[:, 0], X[:, 1], T)
        dye0 = rec.dye[0] if rec.dye and rec.dye[0] is not None else np.zeros(len(X))
        tpc = ax.tripcolor(tri, dye0, shading="gouraud", cmap="magma", vmin=0, vmax=1.0)
        qv = ax.quiver(X[::skip, 0], X[::skip, 1], rec.vel[0][::skip, 0], rec.vel[0][::skip, 1], color="white",
                       scale=20.0)
        ax.set_xlim(0, 1)
        ax.set_ylim(0, 1)
        if vort:
            tpv = ax2.tripcolor(tri, vort[0], shading="gouraud", cmap="coolwarm", vmin=-vmax, vmax=vmax)
            ax2.set_xlim(0, 1)
            ax2.set_ylim(0, 1)

        def arrows(i):
            return rec.vel[i][::skip, 0], rec.vel[i][::skip, 1]

    lines = getattr(rec, "lines", None) or None
    if lines:
        lc = LineCollection(streamline_segments(lines[0]), colors="cyan", linewidths=0.8, zorder=3)
        ax.add_collection(lc)
    fig.colorbar(tpc, ax=ax, label="Dye concentration")
    ax.set_aspect("equal")
    title = ax.set_title(f"Fluid Simulation - Step {rec.steps[0]}")
    if vort:
        fig.colorbar(tpv, ax=ax2, label="Vorticity")
        ax2.set_aspect("equal")
        ax2.set_title("Vorticity (Flow Curl)")

    def update(i):
        if rec.dye[i] is not None:
            tpc.set_array(rec.dye[i])
        qv.set_UVC(*arrows(i))
        if vort:
            tpv.set_array(vort[i])
        if lines:
            lc.set_segments(streamline_segments(lines[i]))
        title.set_text(f"Fluid Simulation - Step {rec.steps[i]}")
        return tpc, qv, title

    out = str(out)
    if out.endswith(".mp4") and shutil.which("ffmpeg"):
        ani = animation.FuncAnimation(fig, update, frames=len(rec), interval=50, blit=False)
        ani.save(out, writer="ffmpeg", fps=fps, dpi=dpi)
        written = [out]
    elif out.endswith(".gif") or out.endswith(".mp4"):
        if out.endswith(".mp4"):  # no ffmpeg on this machine
            out = out[:-4] + ".gif"
        ani = animation.FuncAnimation(fig, update, frames=len(rec), interval=50, blit=False)
        ani.save(out, writer=animation.PillowWriter(fps=fps), dpi=dpi // 2)
        written = [out]
    else:
        os.makedirs(out, exist_ok=True)
        written = []
        for i in range(len(rec)):
            update(i)
            p = os.path.join(out, f"frame_{i:05d}.png")
            fig.savefig(p, dpi=dpi // 2)
            written.append(p)
    plt.close(fig)
    return written
