"""Host time of the transfers of a run's frames on mesh_fine refined LEVEL times: sim.u and sim.c, read and written,
each timed alone in a loop of its own (every call returns after a device synchronise).  At level 5 u is 14 MB and c
7 MB, on either side of the 8 MB threshold at which Ctx::h2d / Ctx::d2h stage through pinned memory.  Run once per
PUCFEM_LIB_VARIANT, alternating, and compare the medians against the runs' own spread.
  python tools/field_io_time.py [LEVEL=5] [REPS=9]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from conftest import load_pkg  # noqa: E402

pf = load_pkg()
level = int(sys.argv[1]) if len(sys.argv) > 1 else 5
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
sim = pf.StokesSimulation(pf.load_mesh("fine", refine=level), pf.SquirmerBC(), 0.05, "color", 0, pf.Tolerances.production())
sim.step(1)
rng = np.random.default_rng(1)
c, u = rng.random(sim.mesh.N), rng.standard_normal((sim.mesh.N, 2))


def timed(f):
    ms = []
    for k in range(reps + 1):  # (the first call is the warm-up: staging buffers are allocated at first use)
        t0 = time.perf_counter()
        f()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = ms[1:]
    return dict(median=round(float(np.median(ms)), 3), min=round(min(ms), 3), max=round(max(ms), 3))


res = dict(variant=os.environ.get("PUCFEM_LIB_VARIANT", "default"), level=level, N=int(sim.mesh.N), u_bytes=int(u.nbytes),
           c_bytes=int(c.nbytes))
res["u_read_ms"] = timed(lambda: sim.u)
res["c_write_ms"] = timed(lambda: setattr(sim, "c", c))
res["c_read_ms"] = timed(lambda: sim.c)
res["u_write_ms"] = timed(lambda: setattr(sim, "u", u))
assert np.array_equal(sim.c, c) and np.array_equal(sim.u, u)
print(json.dumps(res))
sim.close()
