"""Member-steps per second of StokesEnsemble.step with every member's trajectory parts off, the dye's midpoint on,
the MacCormack dye along Euler paths (the yardstick: two locates in two launches), inertia with the midpoint velocity
and the midpoint dye, and everything off again.

For mesh.1 and mesh_fine and M in {1, 8, 64, 256}, one process per (mesh, M) (this script starts itself with --one):
per leg 5 warm-up calls (they capture the one-step and the 8-step graph of the leg's chain), then `--reps` timed calls
of `--steps` (>= 2000) steps each through the C ABI without step records (pucfem_ens_step with stats = NULL returns
after a stream synchronise, so the host clock around a call times the device work).  The one-pass midpoint dye runs two
locates in one launch plus k_ens_wsum, the MacCormack-with-Euler dye two locates in two launches plus k_ens_wsum:
`midpoint_vs_maccormack` says where the midpoint leg's median lies against that leg's own min-max.  The second off leg
shows whether the first leg's rate comes back once the chain is the Euler one again (`off_again_vs_first`).  Writes
profiles/ens_trajectory_rate.json and prints the DESIGN.md section 28 table.

    python tools/ens_trajectory_bench.py [--steps 2000] [--reps 3] [--members 1,8,64,256] [--meshes mesh1,fine]
                                         [--out profiles/ens_trajectory_rate.json]
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("off", "dye midpoint", "dye maccormack (euler)", "inertia+velocity and dye midpoint", "off again")


def timed(call, steps, reps):
    """median and extremes of steps / second over `reps` synchronised calls"""
    rates = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call(steps)
        rates.append(steps / (time.perf_counter() - t0))
    return statistics.median(rates), min(rates), max(rates)


def against(ref, x):
    """where the median of leg x lies against leg ref's own min-max"""
    lo, hi, v = ref["member_steps_per_s_min"], ref["member_steps_per_s_max"], x["member_steps_per_s"]
    if v < lo:
        return f"below ({100.0 * (v / lo - 1.0):.2f} %)"
    if v > hi:
        return f"above (+{100.0 * (v / hi - 1.0):.2f} %)"
    return "within"


def one(name, M, steps, reps):
    """the five legs of one ensemble, in this process"""
    pf = importlib.import_module("puc-fluidsimulation-project_amd")
    S = importlib.import_module("puc-fluidsimulation-project_amd.solver")
    L = importlib.import_module("puc-fluidsimulation-project_amd._lib")
    if pf.device_count() < 1:
        raise RuntimeError("no HIP device visible: the rates are measured on the GPU")
    mesh = pf.load_mesh(name)
    # a B2 sweep from pusher to puller (README.md:43-45 of the reference: B2 = -5, 0, +5), as tools/ensemble_bench.py
    bcs = [S.SquirmerBC(B2=-5.0 + 10.0 * k / max(1, M - 1)) for k in range(M)]
    ens = S.StokesEnsemble(mesh, bcs, 0.05, "color", 0)
    fields = L.TRJ_DYE | L.TRJ_VELOCITY
    rows = []
    try:
        for leg in LEGS:
            ens.set_inertia(leg.startswith("inertia"))
            ens.set_advection(L.ADV_DYE, "maccormack" if leg.startswith("dye maccormack") else "sl")
            ens.set_trajectory(fields, "euler")
            if leg == "dye midpoint":
                ens.set_trajectory(L.TRJ_DYE, "midpoint")
            elif leg.startswith("inertia"):
                ens.set_trajectory(fields, "midpoint")
            for _ in range(5):
                ens.step(16, stats=False)
            med, lo, hi = timed(lambda n: ens.step(n, stats=False), steps, reps)
            info = ens.trajectory_info()
            rows.append(dict(leg=leg, ensemble_steps_per_s=med, member_steps_per_s=med * M,
                             member_steps_per_s_min=lo * M, member_steps_per_s_max=hi * M,
                             state_bytes=ens.info()["state_bytes"], trajectory_bytes=int(info[0]["bytes"]),
                             dye_mid_notfound_last_launch=sum(r["dye_mid_notfound"] for r in info),
                             velocity_mid_notfound_last_launch=sum(r["velocity_mid_notfound"] for r in info)))
    finally:
        ens.close()
    return dict(members=M, legs=rows, midpoint_vs_maccormack=against(rows[2], rows[1]),
                off_again_vs_first=against(rows[0], rows[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--members", default="1,8,64,256")
    ap.add_argument("--meshes", default="mesh1,fine")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ens_trajectory_rate.json"))
    ap.add_argument("--one", nargs=2, metavar=("MESH", "M"), help="(the child's work: one ensemble, JSON on stdout)")
    a = ap.parse_args()
    if a.steps < 2000:
        ap.error("--steps must be at least 2000")
    if a.one:
        print(json.dumps(one(a.one[0], int(a.one[1]), a.steps, a.reps)))
        return
    members = [int(m) for m in a.members.split(",")]
    out = {"steps_per_call": a.steps, "reps": a.reps, "warmup_calls": 5, "scheme": "color", "dt": 0.05,
           "legs": list(LEGS), "meshes": {}}
    for name in a.meshes.split(","):
        rows = []
        for M in members:  # (a fresh process per ensemble; this one never opens the device)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--reps",
                                str(a.reps), "--one", name, str(M)], check=True, stdout=subprocess.PIPE, text=True)
            rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        N = int(importlib.import_module("puc-fluidsimulation-project_amd").load_mesh(name).N)
        out["meshes"][name] = dict(N=N, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("| mesh | N | M | " + " | ".join(f"{leg}: member-steps/s (min-max)" for leg in LEGS) +
          " | midpoint / off | inertia+both / off | midpoint against maccormack's min-max | off again against off's "
          "min-max |")
    print("|---|---|---|" + "---|" * (len(LEGS) + 4))
    for name, d in out["meshes"].items():
        for r in d["rows"]:
            g = r["legs"]
            cells = [f"{x['member_steps_per_s']:.0f} ({x['member_steps_per_s_min']:.0f}-{x['member_steps_per_s_max']:.0f})"
                     for x in g]
            off = g[0]["member_steps_per_s"]
            print(f"| {name} | {d['N']} | {r['members']} | " + " | ".join(cells) +
                  f" | {g[1]['member_steps_per_s'] / off:.2f} | {g[3]['member_steps_per_s'] / off:.2f} | "
                  f"{r['midpoint_vs_maccormack']} | {r['off_again_vs_first']} |")


if __name__ == "__main__":
    main()
