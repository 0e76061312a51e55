"""The pressure projection's two basis passes outside the step (pucfem_proj_probe): k_mdot2 and k_pcomb at a full
basis, ms per launch and TB/s of their algorithmic bytes, REPEATS repeats of 20 launches each; the k_reseed probe
(pucfem_bench_kernel 15) beside them, then the in-step rates of k_cg_upd (an fp64 streaming kernel: the rate to
compare with), k_mdot2 and k_pcomb over three more steps.  Run once per PUCFEM_LIB_VARIANT to compare two builds.
  python tools/proj_bench.py [LEVEL=7] [REPEATS=5]"""
import ctypes as ct
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from conftest import load_pkg  # noqa: E402

pf = load_pkg()
from importlib import import_module  # noqa: E402

L = import_module(pf.__name__ + "._lib")
level = int(sys.argv[1]) if len(sys.argv) > 1 else 7
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
sim = pf.StokesSimulation(pf.load_mesh("fine", refine=level), pf.SquirmerBC(), 0.05, "color", 0, pf.Tolerances.production())
path = sim.ctx.path_info()
steps = 0
while path["basis_p"] < path["proj_k"] and steps < 4 * max(1, path["proj_k"]):  # (a solve appends one direction)
    sim.step(1)
    steps += 1
    path = sim.ctx.path_info()
tag = os.environ.get("PUCFEM_LIB_VARIANT", "default")
print(f"{tag}: L{level}, {steps} steps, basis {path['basis_p']} of {path['proj_k']}, re-seeds {path['reseeds']}")
rows = {}
for _ in range(reps):
    o = (ct.c_double * 6)()
    L.check(L.lib().pucfem_proj_probe(sim.ctx.h, 20, o), sim.ctx.h)
    rows.setdefault(f"k_mdot2<{int(o[4])}>", []).append((o[0], o[2]))
    rows.setdefault(f"k_pcomb<{int(o[5])}>", []).append((o[1], o[3]))
    mb, me, by = ct.c_double(), ct.c_double(), ct.c_double()
    L.check(L.lib().pucfem_bench_kernel(sim.ctx.h, 15, 20, ct.byref(mb), ct.byref(me), ct.byref(by)), sim.ctx.h)
    rows.setdefault("k_reseed", []).append((mb.value, by.value))
for name, r in rows.items():
    ms = sorted(x[0] for x in r)
    med = ms[len(ms) // 2]
    print(f"{tag}: {name:14s} median {1e3 * med:7.1f} us  min {1e3 * ms[0]:7.1f}  max {1e3 * ms[-1]:7.1f}  "
          f"{r[0][1] / (med * 1e-3) / 1e12:5.2f} TB/s")
# the fp64 streaming kernels of the same run (the step's own launches, per-class timing): the rate to compare with
sim.ctx.timing(1)  # (per-launch events on every class)
sim.step(3)
sim.ctx.sync()
for k, name in ((2, "k_cg_upd"), (14, "k_mdot2"), (15, "k_pcomb")):
    tot, n, b = sim.ctx.timing_get(k)
    if n:
        print(f"{tag}: in-step {name:8s} {n:4d} launches  {1e3 * tot / n:7.1f} us  {b / (tot / n * 1e-3) / 1e12:5.2f} TB/s")
sim.ctx.timing(False)
sim.close()
