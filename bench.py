#!/usr/bin/env python3
"""Benchmark: Stokes timesteps/s (and CG iterations/s) of the StokesColor operator-split step.

Workload (BASELINE.json configs[4], the metric's ~10M-node case; it fits one GPU, so N=1 runs it
too): the neutral-squirmer StokesColor step (B1=-2, B2=0, nu=0.1, DT=0.05, StokesColor.py:32-44)
on mesh_fine red-refined 7 times (L7 = 14,230,528 nodes, 28,409,856 triangles), synthetic but
deterministic (no RNG: initial state is the reference's u=0+squirmer BC, c=1[x<0.5]).  A "step"
is one full pass of StokesColor.py:537-586: 2-RHS viscous CG, two periodic-merged pressure CGs
(rtol --rtol-pres), three divergences, two gradient projections, BCs, semi-Lagrangian dye
advection and the mixing index.  Strong scaling: the mesh is fixed and partitioned into y-slabs.

  python bench.py [--gpus N --steps K --warmup W --level 7] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints the headline; --dump-outputs DIR writes
u, p, c after the last timed step as DIR/<name>.npy; --full adds the per-kernel / roofline figures,
the steady-state leg, the secondary workloads and the CPU baseline.

Prints ONE JSON line on rank 0.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: the reference's StokesColor run is 5000 steps; 20 warm-up steps leave the impulsive
    # start (whose steps are reported separately as "startup") so the timed steps are typical ones
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--level", type=int, default=7, help="red refinements of mesh_fine (7 -> 14.2M nodes)")
    ap.add_argument("--rtol-pres", type=float, default=None,
                    help="pressure CG rtol (default: Tolerances.production(), checked by tests/test_gpu_production.py)")
    ap.add_argument("--mg-double", action="store_true", help="fp64 V-cycle instead of the fp32 one")
    ap.add_argument("--mg-vals", default="f32", choices=["f16", "f32", "coarse-f16"],
                    help="fp32 V-cycle operator storage: fp16 on every level, fp32, or fp16 below the finest level")
    ap.add_argument("--index32", action="store_true", help="int32 SELL columns instead of int16 deltas")
    ap.add_argument("--mg-pre", type=int, default=3, help="Chebyshev pre-smoothing degree")
    ap.add_argument("--mg-post", type=int, default=3, help="Chebyshev post-smoothing degree")
    ap.add_argument("--mg-ratio", type=float, default=15.0, help="Chebyshev interval [lmax / ratio, lmax]")
    ap.add_argument("--mg-kind", type=int, default=1, choices=[1, 4], help="Chebyshev smoother of the first / fourth kind")
    ap.add_argument("--proj-separate", action="store_true",
                    help="a projection basis per pressure solve instead of one shared by both")
    ap.add_argument("--proj-k", type=int, default=32,
                    help="pressure initial guess: A-projection onto the last K solutions (0: warm start only)")
    ap.add_argument("--proj-k-visc", type=int, default=0, help="the same for the viscous solve (0: warm start)")
    ap.add_argument("--precond", default="mg", choices=["mg", "jacobi"],
                    help="pressure CG preconditioner: geometric multigrid over the refinement levels, or Jacobi")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline figure: per-launch kernel events on the last timed steps and "
                         "the roofline kernel, the back-to-back kernel table, the steady-state leg, the L5 / StokesFood / "
                         "mesh_fine / heat legs and the CPU baseline (the options below select among these and act "
                         "only with --full)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the state the last timed step left (u, p, c at a fixed seeded "
                         "sample of nodes) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--kernel-table", action="store_true",
                    help="per-launch events on every kernel class (default: the roofline kernel only)")
    ap.add_argument("--no-kernel-timing", action="store_true",
                    help="time the steps without per-launch kernel events (no roofline block)")
    ap.add_argument("--kernel-timing-steps", type=int, default=5,
                    help="per-launch kernel events on the last N of the timed steps (each timed launch costs a few "
                         "us of dispatch: events on all 20 steps slowed the step by ~2 %%, r10i)")
    ap.add_argument("--no-secondary", action="store_true")
    ap.add_argument("--fine-steps", type=int, default=2000)  # (~0.2 s of replays: 200 steps timed ~18 ms, +-10 %)
    ap.add_argument("--steady-after", type=int, default=100,
                    help="steady-state leg: the same run continued to this step, then --steady-steps timed (0: off)")
    ap.add_argument("--steady-steps", type=int, default=20)
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if not a.full:  # a plain run: set up, warm up, time the steps, print the headline
        a.no_cpu_baseline = a.no_secondary = a.no_kernel_timing = True
        a.steady_after = 0
    return a


def main():
    a = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("PUCFEM_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    dist = None
    if world > 1:
        # control plane only (rendezvous, barriers, max-over-ranks timing); the data path uses RCCL
        # from libpucfem on the GPU stream.  torch is imported BEFORE libpucfem is loaded so the
        # process has a single HIP runtime.
        import torch
        import torch.distributed as td

        td.init_process_group("gloo", rank=rank, world_size=world)
    pf = importlib.import_module("puc-fluidsimulation-project_amd")
    L = importlib.import_module("puc-fluidsimulation-project_amd._lib")
    if world > 1:
        import ctypes as ct

        uid = (ct.c_uint8 * 128)()
        if rank == 0:
            L.check(L.lib().pucfem_rccl_unique_id(uid))
        obj = [bytes(uid)]
        td.broadcast_object_list(obj, src=0)
        dist = (rank, world, obj[0])

    def barrier():
        if world > 1:
            td.barrier()

    def allmax(x):
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64)
        td.all_reduce(t, op=td.ReduceOp.MAX)
        return float(t.item())

    def allsum(x):
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64)
        td.all_reduce(t, op=td.ReduceOp.SUM)
        return float(t.item())

    t_setup = time.time()
    mesh = pf.load_mesh("fine", refine=a.level)
    # the production settings (the configuration tests/test_gpu_production.py checks against the
    # oracle), with the measurement knobs below overriding single fields
    tol = pf.Tolerances.production(precond=a.precond, mg_single=not a.mg_double,
                                   mg_f16_vals={"f16": True, "f32": False, "coarse-f16": "coarse"}[a.mg_vals],
                                   index16=not a.index32, mg_degree=a.mg_pre, mg_post=a.mg_post, mg_ratio=a.mg_ratio,
                                   mg_kind=a.mg_kind, proj_k=a.proj_k, proj_k_visc=a.proj_k_visc,
                                   proj_shared=not a.proj_separate)
    if a.rtol_pres is not None:
        tol.rtol_pres = a.rtol_pres
    a.rtol_pres = tol.rtol_pres
    sim = pf.StokesSimulation(mesh, pf.SquirmerBC(), 0.05, "color", device=local, tol=tol, dist=dist)
    info = sim.ctx.info()
    t_setup = time.time() - t_setup
    log = (lambda *m: print(*m, file=sys.stderr, flush=True)) if rank == 0 else (lambda *m: None)
    log(f"[bench] setup {t_setup:.1f}s: {info}")
    startup = []  # wall time of warm-up steps 1..3 (the impulsive start's transient; step 0 has u* = u^n)
    for k in range(a.warmup):
        t = time.perf_counter()
        st = sim.step(1)[0]  # returns the step's stats: synchronous
        if 1 <= k <= 3:
            startup.append((time.perf_counter() - t, st.it_p + st.it_p2))
        log(f"[bench] warmup step {k}: CG visc/p/p2 = {st.it_visc}/{st.it_p}/{st.it_p2}")
    # per-launch events on the roofline kernel only (each timed launch costs a few us of dispatch);
    # --kernel-table times every kernel class of the table below
    kt_mode = 0 if a.no_kernel_timing else (1 if a.kernel_table or a.precond != "mg" else 2)
    kt_steps = min(a.steps, max(1, a.kernel_timing_steps)) if kt_mode else 0
    barrier()
    sim.ctx.sync()
    n0, b0 = sim.ctx.counters()
    cls0 = [sim.ctx.class_counters(k) for k in range(16)]
    t0 = time.perf_counter()
    stats = list(sim.step(a.steps - kt_steps)) if a.steps > kt_steps else []
    if kt_steps:  # the last kt_steps timed steps carry the per-launch events (pucfem_timing_enable syncs)
        sim.ctx.timing(kt_mode)
        stats += list(sim.step(kt_steps))
    sim.ctx.sync()
    barrier()
    dt_local = time.perf_counter() - t0
    n1, b1 = sim.ctx.counters()
    cls1 = [sim.ctx.class_counters(k) for k in range(16)]
    elapsed = allmax(dt_local)
    log(f"[bench] timed {a.steps} steps in {elapsed:.2f}s")
    if a.dump_outputs:  # before anything steps the simulation further
        out = dump_outputs(sim)
        if world > 1:  # u, p: every rank fills its owned rows (the others 0); c is replicated
            for k in ("u", "p"):
                t = torch.from_numpy(out[k])
                td.all_reduce(t, op=td.ReduceOp.SUM)
        if rank == 0:
            import numpy as np

            os.makedirs(a.dump_outputs, exist_ok=True)
            for k, v in out.items():
                np.save(os.path.join(a.dump_outputs, k + ".npy"), v)
            log(f"[bench] wrote {', '.join(out)} to {a.dump_outputs}")
    names = ["k_cheb (MG smoother, finest level)", "k_cg_dir", "k_cg_upd", "k_grad_proj", "k_sl",
             "k_resid (MG residual, finest level)", "k_transfer (restriction from finest)",
             "k_transfer (prolongation to finest)", "k_sl_wq (SL second pass: general locate + rank count)",
             "k_vcheb (viscous Chebyshev step, whole grid)", "k_cheb_pair (two MG smoothing steps, finest level)",
             "k_div (divergence + pressure rhs)", "k_vcheb_pair (two viscous Chebyshev steps, face rows)",
             "k_visc_prep (viscous rhs + extrapolated start)", "k_mdot2 (projection multi-dot)",
             "k_pcomb (projection combination)"]
    ktab = {}
    for k, nm in enumerate(names):
        ms, n, b = sim.ctx.timing_get(k)
        if n:
            gbs = b / (ms / n * 1e-3) / 1e9
            # the class over the WHOLE timed window: its launches and algorithmic bytes there (every launch,
            # pucfem_class_counters) at the rate its timed launches ran
            wn, wb = cls1[k][0] - cls0[k][0], cls1[k][1] - cls0[k][1]
            ktab[nm] = {"launches_timed": n, "avg_launch_ms": ms / n, "bytes_per_launch": b,
                        "achieved_GBps": gbs, "window_launches": wn,
                        "window_ms_est": wb / (gbs * 1e9) * 1e3 if gbs > 0 else 0.0}
    sim.ctx.timing(False)
    # the same kernels launched back to back outside the step (pucfem_bench_kernel): per-launch time
    # of a batch between two events, and the average of per-launch dispatch events
    batch = {}
    if a.full and sim.ctx.precond == "mg" and not a.mg_double:
        import ctypes as ct

        for kid, nm in ((0, "k_cheb"), (1, "k_resid"), (2, "k_cg_dir"), (16 * 8, "k_cheb+8 coarse launches"),
                        (256, "k_cheb, idle GPU at each launch"), (3, "k_cheb face rows only"),
                        (4, "k_cheb skeleton (SELL) rows only"), (5, "k_cg_dir face rows only"),
                        (6, "k_cg_dir skeleton (SELL) rows only"), (7, "k_div (as in the step: interleaved u)"),
                        (8, "k_div face rows only"), (9, "k_div skeleton (SELL) rows only"),
                        (10, "k_div on a viscous (x, y) buffer"), (11, "k_div interleaved, face rows only"),
                        (12, "k_cheb_pair<1> (face rows)"), (13, "k_cheb_pair<2> (face rows)"),
                        (14, "k_vcheb_pair (face rows)"), (15, "k_reseed (projection basis re-seed)")):
            mb, me, by = ct.c_double(), ct.c_double(), ct.c_double()
            L.check(L.lib().pucfem_bench_kernel(sim.ctx.h, kid, 20, ct.byref(mb), ct.byref(me), ct.byref(by)),
                    sim.ctx.h)
            batch[nm] = {"ms_batch": mb.value, "ms_each_event": me.value, "bytes": by.value,
                         "GBps_batch": by.value / (mb.value * 1e-3) / 1e9}
    # CG iterations: the two pressure PCGs (+ the viscous solve when it is a 2-RHS CG); the production
    # viscous solve is a Chebyshev iteration, whose steps are reported apart
    path = sim.ctx.path_info()
    visc_cheb = path["viscous_iteration"] == "chebyshev"
    cg_iters = sum(s.it_p + s.it_p2 + (0 if visc_cheb else 2 * s.it_visc) for s in stats)
    visc_steps = sum(s.it_visc for s in stats)
    steps_per_s = a.steps / elapsed
    launches_per_step = (n1 - n0) / a.steps
    bytes_per_step = allsum(b1 - b0) / a.steps
    rec = {
        "metric": "Stokes timesteps/sec (and CG iters/sec) on mesh_fine & 10M-node mesh, 1/2/4/8 GPU",
        "value": steps_per_s,
        "unit": "timesteps/s",
        "n_gpus": world,
        "steps": a.steps,
        "warmup": a.warmup,
        "ms_per_step": 1e3 * elapsed / a.steps,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f64",
        "precond_dtype": "f64" if a.mg_double or a.precond != "mg" else {
            "f16": "f32 (fp16-stored operators)", "f32": "f32",
            "coarse-f16": "f32 (fp16-stored coarse operators)"}[a.mg_vals],
        "storage": {"index16": [info.get("index16_P"), info.get("index16_Pp")],
                    "mg_vals": a.mg_vals, "finest_f16": info.get("mg_f16_vals")},
        "data": "synthetic (deterministic red-refined mesh_fine, reference initial state)",
        "config": {
            "workload": f"StokesColor neutral squirmer step, mesh_fine refined x{a.level}",
            "nodes": info["N"] if world == 1 else mesh.N, "triangles": mesh.T,
            "dt": 0.05, "nu": 0.1, "B1": -2.0, "B2": 0.0,
            "rtol_pres": a.rtol_pres, "rtol_visc": 1e-12, "pressure_precond": sim.ctx.precond,
            "mg_cheb": {"kind": a.mg_kind, "pre": a.mg_pre, "post": a.mg_post, "ratio": a.mg_ratio},
            "pressure_guess": (f"projection onto up to {a.proj_k} solution directions"
                               + (" per solve" if a.proj_separate else " shared by both solves")) if a.proj_k else "previous solution",
            "viscous_guess": f"projection onto up to {a.proj_k_visc} solution directions" if a.proj_k_visc else "u^n",
            "parallelism": (f"y-slab domain decomposition x{world} (RCCL halo + all-reduce)" if world > 1
                            else "single GPU (the y-slab partition has one part; no RCCL)"),
        },
        "cg_iters_per_s": cg_iters / elapsed,
        "cg_iters_counted": "pressure PCG iterations (both solves)" + ("" if visc_cheb else " + 2 x viscous CG iterations"),
        "visc_cheb_steps_per_s": visc_steps / elapsed if visc_cheb else None,
        "cg_iters_per_step": {("visc_cheb_steps" if visc_cheb else "visc_2rhs"): [s.it_visc for s in stats],
                              "p": [s.it_p for s in stats], "p2": [s.it_p2 for s in stats]},
        "launches_per_step": launches_per_step,
        "diagnostics": {"max_div_star": stats[-1].max_div_star, "max_final_div": stats[-1].max_final_div,
                        "mix_var": stats[-1].mix_var},
        "setup_s": t_setup,
        "startup": {"steps": "warm-up steps 1-3 after the impulsive start (single rank timing)",
                    "ms_per_step": [1e3 * s for s, _ in startup], "pressure_cg_iters": [i for _, i in startup]}
        if startup else None,
    }
    # roofline of the dominant kernel: the timed class with the largest share of the timed region (every
    # class with a share of the step is timed with per-launch events: viscous Chebyshev steps and pairs,
    # divergence, semi-Lagrangian, the finest smoother, the PCG kernels, the projection passes).  Algorithmic
    # bytes per launch are the library's own counts: vectors once per row read or
    # written, stored operators per entry; timed with HIP events taken by each launch's dispatch on the
    # stream it runs on.
    # The dominant class is chosen over the whole timed window: each class's window bytes at its timed rate
    # (the per-launch events cover only the last steps, which past the transient under-weigh the solves)
    dom = max(ktab, key=lambda k: ktab[k]["window_ms_est"]) if ktab else None
    ms_step = 1e3 * elapsed / a.steps
    for k in ktab:  # share of the timed region (the dye stream's kernels overlap the main stream's)
        ktab[k]["ms_per_step"] = ktab[k]["launches_timed"] * ktab[k]["avg_launch_ms"] / kt_steps
        ktab[k]["share"] = ktab[k]["ms_per_step"] / ms_step
        ktab[k]["share_window"] = ktab[k]["window_ms_est"] / (1e3 * elapsed)
    if dom in ktab:
        kd = ktab[dom]
        traffic = None
        pmc = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(pmc):
            try:
                pj = json.load(open(pmc))
                traffic = pj.get(f"L{a.level}_n{world}", {}).get(dom.split()[0])
                ratio = pj.get(f"L{a.level}_n{world}_ratio", {}).get(dom.split()[0])
                if ratio is not None:  # basis-size dependent passes: PMC / algorithmic ratio x these launches' bytes
                    traffic = ratio * kd["bytes_per_launch"]
            except Exception:
                traffic = None
        rec["roofline"] = {"bound": "hbm", "kernel": dom.split()[0], "kernel_share": kd["share_window"],
                           "kernel_choice": "the class with the largest estimated time over the whole timed window "
                                            "(its window bytes at its timed rate)",
                           "achieved": kd["achieved_GBps"],
                           "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": kd["achieved_GBps"] / HBM_PEAK_GBS,
                           "traffic": traffic, "bytes_per_launch": kd["bytes_per_launch"],
                           "avg_launch_ms": kd["avg_launch_ms"], "launches_timed": kd["launches_timed"]}
    # step roofline: the algorithmic bytes of EVERY kernel of the timed steps (the library's per-launch
    # counts, pucfem_counters; all ranks) / the step time -- the step's distance from its HBM floor
    step_gbs = bytes_per_step / (1e-3 * rec["ms_per_step"]) / 1e9
    rec.setdefault("roofline", {"bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s"})["step"] = {
        "bytes_per_step": bytes_per_step, "ms_per_step": rec["ms_per_step"], "achieved": step_gbs,
        "frac": step_gbs / HBM_PEAK_GBS / world, "floor_ms_per_step": bytes_per_step / (HBM_PEAK_GBS * 1e9 * world) * 1e3,
        "counted": "every kernel's algorithmic bytes (vectors once per row read or written, stored operators per entry)"}
    rec["projection"] = sim.ctx.proj_info()  # re-seeds, guess-monitor restarts, last guess residuals
    rec["kernels"] = ktab
    rec["kernels_timed_steps"] = f"the last {kt_steps} of the {a.steps} timed steps" if kt_steps else None
    rec["kernel_batch"] = batch
    if a.steady_after > 0:
        rec["steady"] = steady_leg(sim, a.warmup + a.steps, a.steady_after, a.steady_steps, barrier, allmax, allsum,
                                   world)
    sim.close()
    if rank == 0 and world == 1 and not a.no_secondary and a.level > 5:
        rec["l5"] = gpu_l5(pf, tol)
    if rank == 0 and world == 1 and not a.no_secondary:
        rec["food_l5"] = gpu_food_l5(pf, tol)
    if rank == 0 and world == 1 and not a.no_cpu_baseline:
        rec["cpu_baseline"] = cpu_baseline(pf, a.level, stats, rec.get("l5"))
    if rank == 0 and world == 1 and not a.no_secondary:
        rec["mesh_fine"] = secondary_fine(pf, a.fine_steps)
        rec["heat_fine"] = heat_fine(pf)
    if rank == 0 and world == 1 and a.full:
        # the GPU / CPU ratios measured on this host on BOTH sides (north_star's target: >= 50x the CPU numpy
        # path on mesh_fine)
        cb, fine = rec.get("cpu_baseline"), rec.get("mesh_fine")
        rec["vs_cpu_measured"] = {
            "same_config_L5": cb["same_config"]["ratio"] if cb and "same_config" in cb else None,
            "mesh_fine_vs_cpu_port": fine["ratio_vs_oracle"] if fine else None,
            "mesh_fine_target": 50.0,
            "note": "mesh_fine (1,067 nodes) is launch-latency bound on the GPU; the literal reference's 5.8 steps/s "
                    "(BASELINE.md) was measured on another host and is not used for these ratios"}
    if rank == 0:
        print(json.dumps(rec))
    if world > 1:
        td.destroy_process_group()


DUMP_NODES = 1 << 20  # sampled nodes: u, p, c and the node list are 40 MB in float64


def dump_outputs(sim):
    """What a caller of the timed path holds after its last step: the velocity u, the pressure p and the dye c
    (the fields solve() returns), at all nodes or, on a mesh of more than DUMP_NODES nodes, at a fixed seeded
    sample of them (`nodes`, sorted)."""
    import numpy as np

    L = importlib.import_module("puc-fluidsimulation-project_amd._lib")
    N = sim.mesh.N
    idx = np.arange(N) if N <= DUMP_NODES else np.sort(np.random.default_rng(20240607).choice(N, DUMP_NODES, replace=False))
    return {"nodes": idx.astype(np.float64),
            "u": np.ascontiguousarray(sim.u[idx]),
            "p": np.ascontiguousarray(sim.field(L.F_P)[idx]),
            "c": np.ascontiguousarray(sim.c[idx])}


def gpu_l5(pf, tol, warmup=5, steps=20):
    """The same step on the GPU at L5 (mesh_fine x5, 894,208 nodes: BASELINE configs[3]'s mesh and the
    size the CPU baseline is measured at), with the production settings and the driver's schedule
    (5 warm-up steps, 20 timed): the GPU side of a same-configuration GPU / CPU ratio."""
    m = pf.load_mesh("fine", refine=5)
    sim = pf.StokesSimulation(m, pf.SquirmerBC(), 0.05, "color", tol=tol)
    sim.step(warmup)
    sim.ctx.sync()
    n0, b0 = sim.ctx.counters()
    t = time.perf_counter()
    st = sim.step(steps)
    sim.ctx.sync()
    el = time.perf_counter() - t
    n1, b1 = sim.ctx.counters()
    sim.close()
    ms = 1e3 * el / steps
    return {"mesh": "mesh_fine x5", "nodes": m.N, "warmup": warmup, "steps": steps, "steps_per_s": steps / el,
            "ms_per_step": ms, "launches_per_step": (n1 - n0) / steps,
            "step_roofline_frac": (b1 - b0) / steps / (ms * 1e-3) / (HBM_PEAK_GBS * 1e9),
            "cg_iters_last_step": [st[-1].it_visc, st[-1].it_p, st[-1].it_p2]}


def steady_leg(sim, done, after, steps, barrier, allmax, allsum, world):
    """Past the start-up transient: the benchmarked run continued (untimed) to step `after`, then `steps`
    timed steps -- the rate of the reference's long runs (StokesColor.py:44: 6000 steps), where the
    pressure solves take 1-2 iterations.  Same schedule and tolerances as the headline; no kernel events."""
    if after > done:
        sim.step(after - done)
    barrier()
    sim.ctx.sync()
    n0, b0 = sim.ctx.counters()
    t = time.perf_counter()
    st = sim.step(steps)
    sim.ctx.sync()
    barrier()
    el = allmax(time.perf_counter() - t)
    n1, b1 = sim.ctx.counters()
    ms = 1e3 * el / steps
    return {"after_steps": max(after, done), "steps": steps, "steps_per_s": steps / el, "ms_per_step": ms,
            "projection": sim.ctx.proj_info(),
            "launches_per_step": (n1 - n0) / steps,
            "step_roofline_frac": allsum(b1 - b0) / steps / (ms * 1e-3) / (HBM_PEAK_GBS * 1e9 * world),
            "cg_iters_per_step": {"visc": [s.it_visc for s in st], "p": [s.it_p for s in st],
                                  "p2": [s.it_p2 for s in st]}}


def gpu_food_l5(pf, tol, warmup=5, steps=20):
    """BASELINE configs[3]: the StokesFood pusher (B1=-2, B2=-5, nu=1, DT=0.01; StokesFood.py:441-505, the
    488 tracers at :482-499) on L5 (894,208 nodes), production settings, 5 warm-up steps and 20 timed."""
    m = pf.load_mesh("fine", refine=5)
    sim = pf.StokesSimulation(m, pf.SquirmerBC(B2=-5.0, nu=1.0), 0.01, "food", tol=tol)
    sim.step(warmup)
    sim.ctx.sync()
    n0, b0 = sim.ctx.counters()
    t = time.perf_counter()
    st = sim.step(steps)
    sim.ctx.sync()
    el = time.perf_counter() - t
    n1, b1 = sim.ctx.counters()
    path = sim.ctx.path_info()
    sim.close()
    ms = 1e3 * el / steps
    return {"workload": "StokesFood pusher (B1=-2, B2=-5, nu=1, DT=0.01), mesh_fine x5, 488 tracers",
            "nodes": m.N, "warmup": warmup, "steps": steps, "steps_per_s": steps / el, "ms_per_step": ms,
            "launches_per_step": (n1 - n0) / steps,
            "step_roofline_frac": (b1 - b0) / steps / (ms * 1e-3) / (HBM_PEAK_GBS * 1e9),
            "viscous_iteration": path.get("viscous_iteration"), "eaten_after": st[-1].eaten,
            "cg_iters_last_step": [st[-1].it_visc, st[-1].it_p, st[-1].it_p2]}


def heat_fine(pf, steps=600):
    """BASELINE configs[1]: heatEq.py's 600 backward-Euler steps (heatEq.py:320-325) on mesh_fine, GPU
    against the oracle's HeatLiteral (scipy splu, factorised once) on this host; both end states compared."""
    import numpy as np

    import oracle as O

    mesh = pf.load_mesh("fine")
    h = pf.HeatSimulation(mesh)
    h.ctx.sync()
    t = time.perf_counter()
    h.step(steps)
    h.ctx.sync()
    gpu = steps / (time.perf_counter() - t)
    ug = h.u
    h.close()
    m32 = mesh.as_fp32()
    ref = O.HeatLiteral(m32.coords, m32.markers, m32.triangles)
    u = ref.initial()
    t = time.perf_counter()
    for _ in range(steps):
        u = ref.step(u)
    cpu = steps / (time.perf_counter() - t)
    return {"workload": f"heatEq.py backward Euler, mesh_fine ({mesh.N} nodes), {steps} steps",
            "gpu_steps_per_s": gpu, "cpu_oracle_steps_per_s": cpu, "cpu_oracle_kind": "port (scipy splu, 1 thread)",
            "ratio_vs_oracle": gpu / cpu, "max_abs_diff_u600": float(np.abs(ug - u).max())}


def cpu_baseline(pf, level, stats, l5=None):
    """The CPU sparse restatement (oracle/fem_ref.py StokesRef, the reference's step
    with scipy sparse direct solves in place of its dense LU) timed DIRECTLY on this host at L5 (mesh_fine
    x5, 894,208 nodes, BASELINE configs[3]'s mesh): one untimed step, then 2 timed steps (the bounded
    sample, ~10 s of CPU work on the GPU box's host).  The factorisation setup is reported, not timed.
    Threads: the element loops (divergence, gradient), the semi-Lagrangian k-NN query and per-node tests
    run on `cores` threads (the box's CPU share, at most 16), the two viscous SuperLU solves on two; the
    pressure SuperLU solves are single-threaded (SuperLU).  The benchmarked mesh (L7) is too large for the
    direct solves' fill-in, so `value` is the rate MEASURED at L5 (its mesh in `mesh`) -- not the
    benchmarked mesh's: a ratio against the headline must use `same_config` (GPU and CPU both at L5) or
    `extrapolated_to_benchmark_mesh` (the L5 rate scaled linearly in the node count to L7, a lower bound on
    the CPU cost: the sparse LU solves grow faster than linearly), never value / cpu_baseline.value."""
    import oracle as O

    cores = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()))
    lv = min(level, 5)
    m = pf.load_mesh("fine", refine=lv)
    t = time.perf_counter()
    ref = O.StokesRef(m.coords, m.markers, m.triangles, 0.05, 0.1, -2.0, 0.0, "color", workers=cores)
    t_setup = time.perf_counter() - t
    u, c = ref.initial()
    out = ref.step(u, c)  # first step outside the timing (warm caches)
    u, c = out["u"], out["c"]
    n = 2
    t = time.perf_counter()
    for _ in range(n):
        out = ref.step(u, c)
        u, c = out["u"], out["c"]
    sps = n / (time.perf_counter() - t)
    n_full = stats_nodes(pf, level)
    scale = m.N / n_full
    # value: the rate MEASURED on this host at L5 (the largest mesh the sparse factorisations fit); the
    # benchmarked mesh's CPU rate is only extrapolated (linear in the node count), reported apart
    rec = {"value": sps, "unit": "timesteps/s", "cores": cores, "kind": "port",
           "label": "CPU sparse restatement", "nproc": os.cpu_count(), "mesh": f"mesh_fine x{lv} ({m.N} nodes)",
           "measured": {"mesh": f"mesh_fine x{lv}", "nodes": m.N, "steps_per_s": sps, "setup_s": t_setup},
           "extrapolated_to_benchmark_mesh": {"mesh": f"mesh_fine x{level}", "steps_per_s": sps * scale,
                                              "method": f"x{scale:.5f}, the node ratio (a lower bound on the CPU "
                                                        f"cost: the sparse LU solves grow faster than linearly)"},
           "sample": (f"CPU sparse restatement (oracle StokesRef: scipy SuperLU solves, numpy element loops, "
                      f"KDTree SL; element loops / SL / viscous solves on up to {cores} threads, pressure "
                      f"SuperLU single-threaded; nproc={os.cpu_count()}) timed directly on mesh_fine x{lv} "
                      f"({m.N} nodes): {n} steps at {sps:.4f} steps/s after one untimed step, factorisation "
                      f"setup {t_setup:.1f}s excluded")}
    if l5 is not None and lv == 5:
        rec["same_config"] = {"mesh": "mesh_fine x5", "gpu_steps_per_s": l5["steps_per_s"], "cpu_steps_per_s": sps,
                              "ratio": l5["steps_per_s"] / sps}
    return rec


def stats_nodes(pf, level):
    n = {0: 1067, 5: 894208, 7: 14230528}.get(level)
    return n if n is not None else pf.load_mesh("fine", refine=level).N


def secondary_fine(pf, steps):
    """mesh_fine itself (BASELINE configs[2]): GPU steps/s vs the oracle's full step on this host.
    The literal reference measured 173 ms/step (8 threads) / 203 ms/step (1 thread) in BASELINE.md."""
    import numpy as np

    import oracle as O

    mesh = pf.load_mesh("fine")
    sim = pf.StokesSimulation(mesh, pf.SquirmerBC(), 0.05, "color", tol=pf.Tolerances(rtol_pres=1e-12))
    sim.step(20)
    sim.ctx.sync()
    t = time.perf_counter()
    st = sim.step(steps)
    sim.ctx.sync()
    gpu = steps / (time.perf_counter() - t)
    sim.close()
    ref = O.StokesRef(mesh.coords, mesh.markers, mesh.triangles, 0.05, 0.1, -2.0, 0.0, "color")
    u, c = ref.initial()
    for _ in range(3):
        out = ref.step(u, c)
        u, c = out["u"], out["c"]
    n = 20
    t = time.perf_counter()
    for _ in range(n):
        out = ref.step(u, c)
        u, c = out["u"], out["c"]
    cpu = n / (time.perf_counter() - t)
    return {"workload": "StokesColor neutral squirmer, mesh_fine (1,067 nodes), rtol_pres 1e-12",
            "gpu_steps_per_s": gpu, "cpu_oracle_steps_per_s": cpu, "cpu_oracle_kind": "port (scipy splu per step)",
            "ratio_vs_oracle": gpu / cpu, "reference_literal_steps_per_s_baseline_md": 5.8,
            "ratio_vs_reference_literal": gpu / 5.8,
            "cg_iters_last_step": [st[-1].it_visc, st[-1].it_p, st[-1].it_p2]}


if __name__ == "__main__":
    main()
