"""Cost of a streamline picture: pucfem_streamlines against the same integration as a Python loop over sim.sample.

For mesh_fine and its L5 and L7 refinements (Tolerances.production(), 20 steps first): 4096 seeds on a 64 x 64 grid,
1000 midpoint steps in unit mode, h = half the mesh's shortest edge.  The in-kernel loop: 3 warm-up calls, then the
median and min-max of 10 calls on the host clock around the synchronised call (kernel + the lines' copy to the host),
and the kernel's own time between two HIP events (pucfem_streamlines_probe: 5 back-to-back launches, the lines left
on the device).  The baseline is what the library offered before: the same loop in numpy, one synchronised
sim.sample call per integrator stage (2001 calls) -- it yields the same bits, which is asserted before anything is
timed -- 1 warm-up run, then the median and min-max of 3.
The locator's hint, A/B: the probe with PUCFEM_SLN_HINT=0 (every locate from scratch) and with the hint, three
alternating rounds of 5 launches each.  Lines per wave, A/B: the probe with PUCFEM_SLN_LANES = 1 .. 64 against the
library's own choice, the same rounds.
An ensemble of 8 on mesh_fine: pucfem_ens_streamlines of all members against 8 single-member calls.
--sweep: how the lines-per-wave rule does away from 4096 lines -- the probe (200 steps, median of 3 x 5 launches) for
256 to 65536 lines on mesh_fine and L5, and the ensemble's all-member call (median of 4), each by lines per wave.
Writes profiles/streamline_rate.json and prints the DESIGN.md tables.

    python tools/streamline_bench.py [--levels 0 5 7] [--sweep] [--out profiles/streamline_rate.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pf = importlib.import_module("puc-fluidsimulation-project_amd")
S = importlib.import_module("puc-fluidsimulation-project_amd.solver")

GRID, NSTEPS = 64, 1000
WARMUP, CALLS, PROBE_ITERS, AB_ROUNDS = 3, 10, 5, 3
HINT, LANES = "PUCFEM_SLN_HINT", "PUCFEM_SLN_LANES"
LANE_COUNTS = (1, 2, 4, 8, 16, 32, 64)


def timed_ms(call, warmup=WARMUP, calls=CALLS):
    """median, min, max in ms of `calls` synchronised calls after `warmup` untimed ones"""
    for _ in range(warmup):
        call()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        t.append(1e3 * (time.perf_counter() - t0))
    return dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))


def grid_seeds(n=GRID):
    g = (np.arange(n, dtype=np.float64) + 0.5) / n
    gx, gy = np.meshgrid(g, g)
    return np.ascontiguousarray(np.stack([gx.ravel(), gy.ravel()], 1))


def shortest_edge(mesh):
    """of the refined mesh: red refinement halves every edge, so the base mesh's shortest edge / 2^levels"""
    base = mesh.base if getattr(mesh, "base", None) is not None else mesh
    X, T = base.coords, base.triangles
    e = np.concatenate([X[T[:, 0]] - X[T[:, 1]], X[T[:, 1]] - X[T[:, 2]], X[T[:, 2]] - X[T[:, 0]]])
    return float(np.sqrt((e * e).sum(1)).min()) / 2 ** (mesh.levels if base is not mesh else 0)


def sample_loop(sim, seeds, h, nsteps, vmin=0.0):
    """pucfem_streamlines' loop (unit mode, midpoint) with one sim.sample call per stage: (points, status, npts).
    Ended lines stay in the calls as NaN points, so every call samples len(seeds) points."""
    n = len(seeds)
    pts = np.full((n, nsteps + 1, 2), np.nan)
    status = np.zeros(n, dtype=np.int32)
    npts = np.zeros(n, dtype=np.int32)
    hh = 0.5 * h

    def sample(P):
        got, tri = sim.sample(P, fields=("u",))
        return got["u"], tri >= 0

    def direction(v, alive):
        ax, ay = np.abs(v[:, 0]), np.abs(v[:, 1])
        moving = (ax > vmin) | (ay > vmin)
        status[alive & ~moving] = 2
        m = np.where(ax > ay, ax, ay)
        return v / m[:, None], alive & moving

    with np.errstate(invalid="ignore", divide="ignore"):
        p = seeds.copy()
        v, alive = sample(p)
        status[~alive] = 3
        pts[alive, 0] = p[alive]
        npts[alive] = 1
        for s in range(1, nsteps + 1):
            d, alive = direction(v, alive)
            q = np.stack([np.mod(p[:, 0] + hh * d[:, 0], 1.0), p[:, 1] + hh * d[:, 1]], 1)
            q[~alive] = np.nan
            vq, found = sample(q)
            status[alive & ~found] = 1
            alive = alive & found
            d, alive = direction(vq, alive)
            pn = np.stack([np.mod(p[:, 0] + h * d[:, 0], 1.0), p[:, 1] + h * d[:, 1]], 1)
            pn[~alive] = np.nan
            v, found = sample(pn)
            status[alive & ~found] = 1
            alive = alive & found
            p = np.where(alive[:, None], pn, np.nan)
            pts[alive, s] = pn[alive]
            npts[alive] = s + 1
    return pts, status, npts


def hint_ab(ctx, seeds, h):
    """kernel ms with and without the locator's hint, alternating"""
    on, off = [], []
    for _ in range(AB_ROUNDS):
        os.environ[HINT] = "0"
        off.append(ctx.streamlines_probe(seeds, h, NSTEPS, iters=PROBE_ITERS)["kernel_ms"])
        del os.environ[HINT]
        on.append(ctx.streamlines_probe(seeds, h, NSTEPS, iters=PROBE_ITERS)["kernel_ms"])
    return dict(hint_ms=on, no_hint_ms=off, hint_median_ms=statistics.median(on),
                no_hint_median_ms=statistics.median(off))


def lanes_ab(ctx, seeds, h):
    """kernel ms by lines per wave ("auto": the library's choice), alternating"""
    t = {str(k): [] for k in LANE_COUNTS + ("auto",)}
    for _ in range(AB_ROUNDS):
        for k in LANE_COUNTS:
            os.environ[LANES] = str(k)
            t[str(k)].append(ctx.streamlines_probe(seeds, h, NSTEPS, iters=PROBE_ITERS)["kernel_ms"])
        del os.environ[LANES]
        t["auto"].append(ctx.streamlines_probe(seeds, h, NSTEPS, iters=PROBE_ITERS)["kernel_ms"])
    return {k: dict(ms=v, median_ms=statistics.median(v)) for k, v in t.items()}


def level_rows(level, loop_runs=3):
    mesh = pf.load_mesh("fine", refine=level) if level else pf.load_mesh("fine")
    sim = S.StokesSimulation(mesh, S.SquirmerBC(), 0.05, "color", 0, tol=S.Tolerances.production())
    ctx = sim.ctx
    sim.step(20)
    path = ctx.path_info()
    seeds = grid_seeds()
    h = 0.5 * shortest_edge(mesh)
    got = sim.streamlines(seeds, h, NSTEPS)
    ref = sample_loop(sim, seeds, h, NSTEPS)
    same = (np.array_equal(got.points, ref[0], equal_nan=True) and np.array_equal(got.status, ref[1]) and
            np.array_equal(got.npts, ref[2]))
    if not same:
        raise RuntimeError(f"level {level}: the kernel's lines differ from the sample loop's")
    call = timed_ms(lambda: sim.streamlines(seeds, h, NSTEPS))
    probe = ctx.streamlines_probe(seeds, h, NSTEPS, iters=PROBE_ITERS)
    loop = timed_ms(lambda: sample_loop(sim, seeds, h, NSTEPS), warmup=1, calls=loop_runs)
    ab = hint_ab(ctx, seeds, h)
    lab = lanes_ab(ctx, seeds, h)
    sim.close()
    locates = int(2 * (got.npts[got.npts > 0] - 1).sum() + (got.npts > 0).sum())
    return dict(level=level, N=mesh.N, T=mesh.T, sl_locator=path["sl_locator"], h=h, seeds=len(seeds), nsteps=NSTEPS,
                status_counts=np.bincount(got.status, minlength=4).tolist(), stored_points=int(got.npts.sum()),
                locates_at_least=locates, call=call, kernel_ms=probe["kernel_ms"], output_bytes=probe["output_bytes"],
                sample_loop=loop, sample_calls=1 + 2 * NSTEPS, equal_bits=True, hint_ab=ab, lanes_ab=lab)


def ensemble_rows(M=8):
    mesh = pf.load_mesh("fine")
    bcs = [S.SquirmerBC(B2=-5.0 + 10.0 * k / max(1, M - 1)) for k in range(M)]
    ens = S.StokesEnsemble(mesh, bcs, 0.05, "color", 0)
    ens.step(20, stats=False)
    seeds = grid_seeds()
    h = 0.5 * shortest_edge(mesh)
    allm = ens.streamlines(seeds, h, NSTEPS)
    for m in range(M):
        one = ens.streamlines(seeds, h, NSTEPS, member=m)
        if not np.array_equal(allm.points[m], one.points, equal_nan=True):
            raise RuntimeError(f"member {m}: the all-member call differs from its own")
    r = timed_ms(lambda: ens.streamlines(seeds, h, NSTEPS))
    g = timed_ms(lambda: [ens.streamlines(seeds, h, NSTEPS, member=m) for m in range(M)])
    ens.close()
    return dict(members=M, N=mesh.N, h=h, seeds=len(seeds), nsteps=NSTEPS, all_members=r, single_calls=g)


def set_lanes(k):
    if k == "auto":
        os.environ.pop(LANES, None)
    else:
        os.environ[LANES] = str(k)


def sweep_rows(nsteps=200):
    out = dict(nsteps=nsteps, single=[], ensemble=[])
    for level in (0, 5):
        mesh = pf.load_mesh("fine", refine=level) if level else pf.load_mesh("fine")
        sim = S.StokesSimulation(mesh, S.SquirmerBC(), 0.05, "color", 0, tol=S.Tolerances.production())
        sim.step(20)
        h = 0.5 * shortest_edge(mesh)
        for g in (16, 32, 128, 256):
            seeds = grid_seeds(g)
            row = dict(level=level, sl_locator=sim.ctx.path_info()["sl_locator"], lines=g * g, kernel_ms={})
            for k in LANE_COUNTS + ("auto",):
                set_lanes(k)
                t = [sim.ctx.streamlines_probe(seeds, h, nsteps, iters=PROBE_ITERS)["kernel_ms"] for _ in range(3)]
                row["kernel_ms"][str(k)] = statistics.median(t)
            out["single"].append(row)
        sim.close()
    mesh = pf.load_mesh("fine")
    ens = S.StokesEnsemble(mesh, [S.SquirmerBC(B2=-5.0 + 10.0 * k / 7) for k in range(8)], 0.05, "color", 0)
    ens.step(20, stats=False)
    seeds = grid_seeds()
    h = 0.5 * shortest_edge(mesh)
    for _ in range(2):
        for k in LANE_COUNTS + ("auto",):
            set_lanes(k)
            r = timed_ms(lambda: ens.streamlines(seeds, h, NSTEPS), warmup=1, calls=4)
            r["lanes"] = str(k)
            out["ensemble"].append(r)
    set_lanes("auto")
    ens.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, nargs="*", default=[0, 5, 7])
    ap.add_argument("--ensemble", type=int, default=8, help="members of the ensemble row (0: none)")
    ap.add_argument("--sweep", action="store_true", help="also the lines-per-wave sweep over other line counts")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "streamline_rate.json"))
    a = ap.parse_args()
    if pf.device_count() < 1:
        raise RuntimeError("no HIP device visible: the streamline costs are measured on the GPU")
    out = dict(seed_grid=GRID, nsteps=NSTEPS, mode="unit, midpoint", warmup_calls=WARMUP, calls=CALLS,
               probe_iters=PROBE_ITERS, steps_before=20, tolerances="production", levels=[], ensembles=[])
    if os.path.exists(a.out):  # (levels measured by an earlier call are kept)
        with open(a.out) as f:
            old = json.load(f)
        out["levels"] = [d for d in old.get("levels", []) if d["level"] not in a.levels]
        out["ensembles"] = old.get("ensembles", []) if not a.ensemble else []
        if "lanes_sweep" in old:
            out["lanes_sweep"] = old["lanes_sweep"]

    def flush():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        out["levels"].sort(key=lambda d: d["level"])
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    for lv in a.levels:
        out["levels"].append(level_rows(lv))
        flush()
        print(f"level {lv} done", flush=True)
    if a.ensemble:
        out["ensembles"].append(ensemble_rows(a.ensemble))
        flush()
    if a.sweep:
        out["lanes_sweep"] = sweep_rows()
        flush()
    print("| mesh | N | locator | h | streamlines call ms (min-max) | kernel ms | sample loop ms (min-max) | loop / call | "
          "kernel ms without hint | with hint |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for d in out["levels"]:
        c, lp, ab = d["call"], d["sample_loop"], d["hint_ab"]
        print(f"| mesh_fine x{d['level']} | {d['N']} | {d['sl_locator']} | {d['h']:.3g} | {c['median_ms']:.2f} "
              f"({c['min_ms']:.2f}-{c['max_ms']:.2f}) | {d['kernel_ms']:.2f} | {lp['median_ms']:.0f} "
              f"({lp['min_ms']:.0f}-{lp['max_ms']:.0f}) | {lp['median_ms'] / c['median_ms']:.1f} | "
              f"{ab['no_hint_median_ms']:.2f} ({min(ab['no_hint_ms']):.2f}-{max(ab['no_hint_ms']):.2f}) | "
              f"{ab['hint_median_ms']:.2f} ({min(ab['hint_ms']):.2f}-{max(ab['hint_ms']):.2f}) |")
    print()
    print("| mesh | kernel ms by lines per wave: " + " | ".join(str(k) for k in LANE_COUNTS) + " | library's choice |")
    print("|---|" + "---|" * (len(LANE_COUNTS) + 1))
    for d in out["levels"]:
        lab = d["lanes_ab"]
        print(f"| mesh_fine x{d['level']} | " + " | ".join(f"{lab[str(k)]['median_ms']:.2f}" for k in LANE_COUNTS) +
              f" | {lab['auto']['median_ms']:.2f} |")
    print()
    print("| M | ens_streamlines, all members ms (min-max) | M single-member calls ms (min-max) |")
    print("|---|---|---|")
    for e in out["ensembles"]:
        r, g = e["all_members"], e["single_calls"]
        print(f"| {e['members']} | {r['median_ms']:.2f} ({r['min_ms']:.2f}-{r['max_ms']:.2f}) | "
              f"{g['median_ms']:.2f} ({g['min_ms']:.2f}-{g['max_ms']:.2f}) |")
    sw = out.get("lanes_sweep")
    if sw:
        print()
        print(f"| mesh | lines | kernel ms ({sw['nsteps']} steps) by lines per wave: " +
              " | ".join(str(k) for k in LANE_COUNTS) + " | library's choice |")
        print("|---|---|" + "---|" * (len(LANE_COUNTS) + 1))
        for r in sw["single"]:
            print(f"| mesh_fine x{r['level']} ({r['sl_locator']}) | {r['lines']} | " +
                  " | ".join(f"{r['kernel_ms'][str(k)]:.2f}" for k in LANE_COUNTS) + f" | {r['kernel_ms']['auto']:.2f} |")
        print()
        print("| ensemble of 8, all-member call ms by lines per wave (two rounds) | " +
              " | ".join(str(k) for k in LANE_COUNTS) + " | library's choice |")
        print("|---|" + "---|" * (len(LANE_COUNTS) + 1))
        for i in range(0, len(sw["ensemble"]), len(LANE_COUNTS) + 1):
            print("| median | " + " | ".join(f"{r['median_ms']:.1f}" for r in sw["ensemble"][i:i + len(LANE_COUNTS) + 1]) + " |")


if __name__ == "__main__":
    main()
