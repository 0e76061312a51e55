"""Member-steps per second of StokesEnsemble.step against the single-context StokesSimulation.step rate.

For mesh.1 and mesh_fine and M in {1, 8, 64, 256}: 5 warm-up calls (they capture the one-step and the 8-step
graph), then `--reps` timed calls of `--steps` (>= 2000) steps each through the C ABI without step records
(pucfem_ens_step / pucfem_step with stats = NULL; both return after a stream synchronise, so the host clock
around a call times the device work).  The single-context rate is measured in the same process on the same
device, before and after the ensembles.  Writes profiles/ensemble_rate.json and prints the DESIGN.md table.

    python tools/ensemble_bench.py [--steps 2000] [--reps 3] [--out profiles/ensemble_rate.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pf = importlib.import_module("puc-fluidsimulation-project_amd")
S = importlib.import_module("puc-fluidsimulation-project_amd.solver")

MEMBERS = (1, 8, 64, 256)


def timed(call, steps, reps):
    """median and extremes of steps / second over `reps` synchronised calls"""
    rates = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call(steps)
        rates.append(steps / (time.perf_counter() - t0))
    return statistics.median(rates), min(rates), max(rates)


def single_rate(mesh, steps, reps):
    sim = S.StokesSimulation(mesh, S.SquirmerBC(), 0.05, "color", 0)
    ctx = sim.ctx

    def call(n):
        ctx._c(ctx.L.pucfem_step(ctx.h, n, None))

    for _ in range(5):
        call(16)
    r = timed(call, steps, reps)
    sim.close()
    return r


def ensemble_rate(mesh, M, steps, reps):
    # a B2 sweep from pusher to puller (README.md:43-45 of the reference: B2 = -5, 0, +5)
    bcs = [S.SquirmerBC(B2=-5.0 + 10.0 * k / max(1, M - 1)) for k in range(M)]
    ens = S.StokesEnsemble(mesh, bcs, 0.05, "color", 0)
    info = ens.info()
    for _ in range(5):
        ens.step(16, stats=False)
    r = timed(lambda n: ens.step(n, stats=False), steps, reps)
    ens.close()
    return r, info


def dense_bytes(n, M, tile):
    """algorithmic bytes of the three dense products of one ensemble step: each matrix once per tile of members,
    the viscous product's 2-component input and output and the pressure products' input and output per member"""
    tiles = (M + tile - 1) // tile
    return tiles * 3 * 8 * n * n + M * (2 * 16 * n + 2 * 2 * 8 * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_rate.json"))
    a = ap.parse_args()
    if a.steps < 2000:
        ap.error("--steps must be at least 2000")
    if pf.device_count() < 1:
        raise RuntimeError("no HIP device visible: the rates are measured on the GPU")
    out = {"steps_per_call": a.steps, "reps": a.reps, "warmup_calls": 5, "scheme": "color", "dt": 0.05, "meshes": {}}
    for name in ("mesh1", "fine"):
        mesh = pf.load_mesh(name)
        s0 = single_rate(mesh, a.steps, a.reps)
        rows = []
        for M in MEMBERS:
            (med, lo, hi), info = ensemble_rate(mesh, M, a.steps, a.reps)
            rows.append(dict(members=M, member_tile=info["member_tile"], state_bytes=info["state_bytes"],
                             ensemble_steps_per_s=med, ensemble_steps_per_s_min=lo, ensemble_steps_per_s_max=hi,
                             member_steps_per_s=med * M,
                             dense_bytes_per_step=dense_bytes(mesh.N, M, info["member_tile"])))
        s1 = single_rate(mesh, a.steps, a.reps)
        single = 0.5 * (s0[0] + s1[0])
        for r in rows:
            r["speedup_vs_single_steps"] = r["member_steps_per_s"] / single
            r["dense_GBps"] = r["dense_bytes_per_step"] * r["ensemble_steps_per_s"] / 1e9
        out["meshes"][name] = dict(N=mesh.N, single_steps_per_s=single, single_before=s0, single_after=s1, rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("| mesh | N | M | ensemble steps/s (min-max) | member-steps/s | x single | dense bytes/step | dense GB/s |")
    print("|---|---|---|---|---|---|---|---|")
    for name, d in out["meshes"].items():
        print(f"| {name} | {d['N']} | single | {d['single_steps_per_s']:.0f} | {d['single_steps_per_s']:.0f} | 1.0 | | |")
        for r in d["rows"]:
            print(f"| {name} | {d['N']} | {r['members']} | {r['ensemble_steps_per_s']:.0f} "
                  f"({r['ensemble_steps_per_s_min']:.0f}-{r['ensemble_steps_per_s_max']:.0f}) | "
                  f"{r['member_steps_per_s']:.0f} | {r['speedup_vs_single_steps']:.1f} | "
                  f"{r['dense_bytes_per_step'] / 1e6:.1f} MB | {r['dense_GBps']:.0f} |")


if __name__ == "__main__":
    main()
