"""Cost of the vorticity pass: pucfem_flow_info and a vorticity frame against the copy of u they replace.

On mesh_fine's L7 refinement (14.2M nodes, Tolerances.production(), 5 steps first), in one process:
  (a) flow_info(): the minimum (and median, maximum) of 20 calls after 3 untimed ones on the host clock around the
      synchronous call -- one launch of the curl form of k_div with its four reductions and one 32-byte copy;
  (b) raster(("vorticity",)) at 1920 x 1080, timed the same way (the curl pass storing the field, the raster
      kernel, the image's copy);
  (c) for scale, what the same picture needed before: sim.u, the copy of the velocity to the host;
  (d) sample(one point, ("vorticity",)): the curl pass storing the field with no reduction in the launch, one
      point located and two small copies -- beside (a), what the four in-kernel reductions and the rows' own u cost;
  and the time per launch of k_div itself in the same process (timing class 11: HIP events around the step's own
  launches over 5 further steps) with its algorithmic bytes per launch.  The flow pass moves a k_div launch's
  bytes plus 16 B per row (the row's own u); the pass of (b) stores the field instead, 8 B per row.
Writes profiles/vorticity_rate.json and prints the DESIGN.md table.

    python tools/vorticity_bench.py [--level 7] [--out profiles/vorticity_rate.json]
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

WARMUP, CALLS = 3, 20
W, H = 1920, 1080


def timed_ms(call, warmup=WARMUP, calls=CALLS):
    """min, median, max in ms of `calls` synchronous calls after `warmup` untimed ones"""
    for _ in range(warmup):
        call()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        t.append(1e3 * (time.perf_counter() - t0))
    return dict(min_ms=min(t), median_ms=statistics.median(t), max_ms=max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vorticity_rate.json"))
    a = ap.parse_args()
    if pf.device_count() < 1:
        raise RuntimeError("no HIP device visible: the costs are measured on the GPU")
    mesh = pf.load_mesh("fine", refine=a.level) if a.level else pf.load_mesh("fine")
    sim = S.StokesSimulation(mesh, S.SquirmerBC(), 0.05, "color", 0, tol=S.Tolerances.production())
    ctx = sim.ctx
    sim.step(5)
    out = dict(level=a.level, N=mesh.N, T=mesh.T, warmup_calls=WARMUP, calls=CALLS, steps_before=5,
               tolerances="production", lattice=ctx.path_info()["lattice"])
    out["flow_info"] = timed_ms(sim.flow_info)
    out["flow_info"]["values"] = sim.flow_info()
    out["raster_vorticity"] = dict(timed_ms(lambda: sim.raster(W, H, fields=("vorticity",))), width=W, height=H)
    out["copy_u"] = dict(timed_ms(lambda: sim.u, calls=5), bytes=16 * mesh.N)
    out["probe_vorticity"] = timed_ms(lambda: sim.sample([[0.25, 0.25]], fields=("vorticity",)))
    # k_div as the step launches it, in the same process
    ctx.timing(2)
    sim.step(5)
    ctx.sync()
    ms, n, b = ctx.timing_get(11)
    ctx.timing(0)
    out["k_div"] = dict(launches=n, ms_per_launch=ms / max(1, n), bytes_per_launch=b)
    sim.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    fi, ra, cu, kd, pr = out["flow_info"], out["raster_vorticity"], out["copy_u"], out["k_div"], out["probe_vorticity"]
    print("| mesh | N | flow_info ms min (median, max) | vorticity raster 1920 x 1080 ms min (median, max) | "
          "copy of u ms min (median, max) | one-point vorticity probe ms min (median, max) | "
          "k_div ms / launch (class 11) | k_div bytes / launch |")
    print("|---|---|---|---|---|---|---|---|")
    print(f"| mesh_fine x{a.level} | {mesh.N} | {fi['min_ms']:.3f} ({fi['median_ms']:.3f}, {fi['max_ms']:.3f}) | "
          f"{ra['min_ms']:.2f} ({ra['median_ms']:.2f}, {ra['max_ms']:.2f}) | "
          f"{cu['min_ms']:.1f} ({cu['median_ms']:.1f}, {cu['max_ms']:.1f}) | "
          f"{pr['min_ms']:.3f} ({pr['median_ms']:.3f}, {pr['max_ms']:.3f}) | {kd['ms_per_launch']:.3f} | "
          f"{kd['bytes_per_launch']:.3e} |")


if __name__ == "__main__":
    main()
