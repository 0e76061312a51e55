"""Cost of a time-dependent stroke: its kernel, the step rate with it on, and what it does to the dye.

For mesh_fine and its L5 and L7 refinements (scheme 'color', B1 = 1, B2 = 2, nu = 0.1, dt = 0.05;
Tolerances.production() on the refined meshes), after 150 Stokes steps (bench.py's steady window starts at 100):

(a) steps/s of the run with no stroke, with Stroke.constant(B1, B2), and with no stroke again: pucfem_step over `steps`
    steps on the host clock after 2 untimed steps, REPEATS times each: median and min-max, with the launches per step
    of each leg (pucfem_counters).  The constant table imposes the static values' bits, so the flow and the solves'
    iterations stay the plain run's: the difference is the launch itself and, on the small mesh, the step leaving its
    captured graph.  "off" is measured first.
(b) ms per k_stroke_bc launch (pucfem_stroke_probe: one untimed launch, then `--iters` launches between two events),
    REPEATS times, for K = 2 and K = 8: median and min-max.
(c) --ensembles: mesh1 and mesh_fine ensembles of M = 1, 8, 64, 256 members, member-steps/s with no member stroked,
    with every member on the constant table, and with none again.
(d) --mixing N: on mesh_fine with advection="maccormack", N steps of the steady neutral swimmer, the steady pusher, the
    steady puller and a blinking pusher / puller (period --period): the dye's mixing progress 1 - var / var0 of c
    (StokesColor.py:586) and of the three dye_patterns channels, at N / 4, N / 2 and N steps.

Writes profiles/stroke_rate.json (--out).

    python tools/stroke_bench.py [--levels 0 5 7] [--ensembles] [--mixing 400] [--out FILE]
"""
import argparse
import ctypes as ct
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPEATS, SETTLE = 5, 150
STEPS = {0: 400, 5: 60, 7: 20}  # timed steps per repeat (the small mesh steps in ~0.1 ms)
ENS_M, ENS_STEPS = (1, 8, 64, 256), 64
B1, B2 = 1.0, 2.0


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, nargs="*", default=[0, 5, 7])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--ensembles", action="store_true")
    ap.add_argument("--mixing", type=int, default=0)
    ap.add_argument("--period", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "stroke_rate.json"))
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    pf = importlib.import_module("puc-fluidsimulation-project_amd")
    S = importlib.import_module("puc-fluidsimulation-project_amd.solver")
    L = importlib.import_module("puc-fluidsimulation-project_amd._lib")
    if pf.device_count() < 1:
        raise RuntimeError("no HIP device visible: the stroke rates are measured on the GPU")
    run = dict(repeats=REPEATS, probe_iters=a.iters, rows=[], ensembles=[], mixing=[])
    if os.path.exists(a.out):  # (one process per table: the tables a call does not make are kept)
        with open(a.out) as f:
            old = json.load(f)
        for key, made in (("rows", bool(a.levels)), ("ensembles", a.ensembles), ("mixing", bool(a.mixing))):
            if not made:
                run[key] = old.get(key, [])

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(run, f, indent=1)
            f.write("\n")

    bc = S.SquirmerBC(B1=B1, B2=B2, nu=0.1)
    const = pf.Stroke.constant(B1, B2)
    for lv in a.levels:
        mesh = pf.load_mesh("fine", refine=lv) if lv else pf.load_mesh("fine")
        tol = S.Tolerances.production() if lv else S.Tolerances()
        sim = S.StokesSimulation(mesh, bc, 0.05, "color", 0, tol=tol)
        ctx = sim.ctx
        sim.step(SETTLE)  # (past the start-up transient: the solves of a settled Stokes flow start converged)
        row = dict(level=lv, N=mesh.N, viscous=ctx.path_info()["viscous"], steps_per_s={}, launches_per_step={}, kernel={})
        n = STEPS.get(lv, 20)
        stats = (L.StepStats * n)()

        def rate(label, stroke):
            sim.stroke = stroke
            rates, launches = [], []
            for _ in range(REPEATS):
                ctx._c(ctx.L.pucfem_step(ctx.h, 2, None))
                n0 = ctx.counters()[0]
                t = time.perf_counter()
                ctx._c(ctx.L.pucfem_step(ctx.h, n, ct.cast(stats, ct.POINTER(L.StepStats))))
                rates.append(n / (time.perf_counter() - t))
                launches.append((ctx.counters()[0] - n0) / n)
            row["steps_per_s"][label] = spread(rates)
            row["launches_per_step"][label] = spread(launches)

        rate("off", None)
        rate("constant", const)
        rate("off_again", None)
        for K in (2, 8):
            sim.stroke = pf.Stroke(np.full((50, K), 0.5))
            r = [ctx.stroke_probe(a.iters) for _ in range(REPEATS)]
            row["kernel"][f"K{K}"] = dict(ms=spread([x["kernel_ms"] for x in r]), algo_bytes=r[0]["algo_bytes"],
                                          driven=sim.stroke_info()["nodes"])
        sim.stroke = None
        run["rows"].append(row)
        flush()
        print(f"L{lv} N={mesh.N} {row['viscous']}: steps/s "
              + ", ".join(f"{k}: {v['median']:.1f} ({v['min']:.1f}-{v['max']:.1f})" for k, v in row["steps_per_s"].items())
              + "; launches/step " + ", ".join(f"{k}: {v['median']:.2f}" for k, v in row["launches_per_step"].items())
              + "; k_stroke_bc " + ", ".join(f"{k} ({v['driven']} entries): {1e3 * v['ms']['median']:.2f} us "
                                             f"({1e3 * v['ms']['min']:.2f}-{1e3 * v['ms']['max']:.2f})"
                                             for k, v in row["kernel"].items()), flush=True)
        sim.close()

    if a.ensembles:
        for name in ("mesh1", "fine"):
            mesh = pf.load_mesh(name)
            for M in ENS_M:
                ens = S.StokesEnsemble(mesh, [bc] * M, 0.05, "color")
                ens.step(5, stats=False)
                row = dict(mesh=name, N=mesh.N, M=M, member_steps_per_s={})

                def erate(label, stroke):
                    ens.set_stroke(stroke)
                    rates = []
                    for _ in range(REPEATS):
                        ens.step(2, stats=False)
                        t = time.perf_counter()
                        ens.step(ENS_STEPS, stats=False)
                        rates.append(M * ENS_STEPS / (time.perf_counter() - t))
                    row["member_steps_per_s"][label] = spread(rates)

                erate("off", None)
                erate("constant", const)
                erate("off_again", None)
                run["ensembles"].append(row)
                flush()
                print(f"{name} M={M}: member-steps/s "
                      + ", ".join(f"{k}: {v['median']:.0f} ({v['min']:.0f}-{v['max']:.0f})"
                                  for k, v in row["member_steps_per_s"].items()), flush=True)
                ens.close()

    if a.mixing:
        mesh = pf.load_mesh("fine")
        swimmers = {"steady neutral": (0.0, None), "steady pusher": (-B2, None), "steady puller": (B2, None),
                    "blinking pusher/puller": (B2, pf.Stroke.blinking(a.period, (B1, -B2), (B1, B2)))}
        marks = sorted({max(1, a.mixing // 4), max(1, a.mixing // 2), a.mixing})
        for label, (b2, stroke) in swimmers.items():
            sim = S.StokesSimulation(mesh, S.SquirmerBC(B1=B1, B2=b2, nu=0.1), 0.05, "color", 0,
                                     advection="maccormack", stroke=stroke)
            sim.dyes = pf.dye_patterns(mesh)
            var0 = [S._mixing0(mesh, sim)[2]] + sim.dye_mixing()[:, 2].tolist()
            row = dict(swimmer=label, steps=[], progress_c=[], progress_dyes=[])
            done = 0
            for m in marks:
                st = sim.step(m - done)
                done = m
                var = [st[-1].mix_var] + sim.dye_mixing()[:, 2].tolist()
                prog = [1.0 - v / (v0 + 1e-16) for v, v0 in zip(var, var0)]
                row["steps"].append(m)
                row["progress_c"].append(prog[0])
                row["progress_dyes"].append(prog[1:])
            run["mixing"].append(row)
            flush()
            print(f"{label}: " + "; ".join(f"step {m}: c {pc:.4f}, dyes " + " ".join(f"{v:.4f}" for v in pd)
                                           for m, pc, pd in zip(row["steps"], row["progress_c"], row["progress_dyes"])),
                  flush=True)
            sim.close()


if __name__ == "__main__":
    main()
