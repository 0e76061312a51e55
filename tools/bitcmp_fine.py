"""Hash of the mesh_fine fields and step records after K steps of the small-mesh (graph) path (compare builds or
knobs bit for bit: run once per PUCFEM_LIB_VARIANT / setting).  SCHEME: color (default) or food (StokesFood: the
tracers and their status instead of the dye).
  python tools/bitcmp_fine.py STEPS [SCHEME]"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from conftest import load_pkg  # noqa: E402

pf = load_pkg()
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
scheme = sys.argv[2] if len(sys.argv) > 2 else "color"
if scheme == "food":
    bc, dt = pf.SquirmerBC(B2=-5.0, nu=1.0), 0.01
else:
    bc, dt = pf.SquirmerBC(), 0.05
sim = pf.StokesSimulation(pf.load_mesh("fine"), bc, dt, scheme, 0, pf.Tolerances(rtol_pres=1e-12))
st = sim.step(steps)
h = hashlib.sha256()
for a in (sim.u, sim.c) if scheme == "color" else (sim.u, sim.tracers, sim.tracer_status):
    h.update(a.tobytes())
h.update(repr([(s.max_div_star, s.max_final_div, s.mix_var) for s in st]).encode())
print(os.environ.get("PUCFEM_LIB_VARIANT", "default"), f"mesh_fine {scheme} {steps} steps", h.hexdigest()[:24])
sim.close()
