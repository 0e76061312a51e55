"""pucfem_proj_probe: the pressure projection's basis passes timed outside the step.

The probe launches k_mdot2 / k_pcomb on the context's own basis and vectors with every output sent to scratch, so a
run that probes between its steps must stay bit for bit the run that does not -- at a part-filled basis, at a full one
(the combination pass then takes the capacity - 1 instance) and across a re-seed.  mesh_fine x2 (14,672 nodes: more
than one block, and no multiple of 64, so the basis' last tile is part-filled) with the bench's settings and a small
capacity, so the shared basis fills and is re-seeded within a few steps.
"""
import numpy as np
import pytest

from conftest import has_gpu, load_pkg

pytestmark = pytest.mark.gpu

pf = load_pkg()
from importlib import import_module  # noqa: E402

S = import_module("puc-fluidsimulation-project_amd.solver")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not has_gpu():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _run(probe):
    mesh = pf.load_mesh("fine", refine=2)
    sim = S.StokesSimulation(mesh, S.SquirmerBC(), 0.05, "color", 0, S.Tolerances.production(proj_k=6, rtol_pres=1e-12))
    seen, its = [], []
    for _ in range(12):
        st = sim.step(1)[0]
        its.append((st.it_visc, st.it_p, st.it_p2))
        if probe:
            seen.append((sim.ctx.path_info()["basis_p"], sim.ctx.proj_probe(2)))
    out = sim.u.copy(), sim.c.copy(), its, sim.ctx.path_info()
    n_own = sim.ctx.info()["n_own"]
    sim.close()
    return out, seen, n_own


def test_probe_reports_the_basis_and_leaves_the_run_bit_for_bit():
    (u0, c0, its0, path0), _, _ = _run(False)
    (u1, c1, its1, path1), seen, n = _run(True)
    assert path0["proj_k"] == 6 and path0["reseeds"] >= 2, path0
    assert n > 256 and n % 64 != 0, n
    sizes = set()
    for m, p in seen:
        assert p["m"] == m and p["m_pcomb"] == min(m, 5), (m, p)
        assert p["mdot2_ms"] > 0.0 and p["pcomb_ms"] > 0.0, p
        assert p["mdot2_bytes"] == (4.0 * m + 44.0) * n and p["pcomb_bytes"] == (4.0 * p["m_pcomb"] + 24.0) * n, p
        sizes.add(m)
    assert 6 in sizes and len(sizes) >= 3, sizes  # a full basis and part-filled ones were probed
    assert its0 == its1 and path0 == path1
    assert np.array_equal(u0, u1) and np.array_equal(c0, c1)
