"""bench.py --dump-outputs: the arrays it writes (host side; the fields come from a stand-in simulation).

Two builds are compared output for output, so the sample of nodes must be the same from run to run, the
arrays float64, and the whole dump within 64 MB at the benchmark's mesh size."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class FakeSim:
    def __init__(self, n):
        self.mesh = types.SimpleNamespace(N=n)
        self.u = np.stack([np.arange(n, dtype=np.float64), -np.arange(n, dtype=np.float64)], 1)
        self.c = np.arange(n, dtype=np.float64) + 0.5

    def field(self, f):
        return 2.0 * np.arange(self.mesh.N, dtype=np.float64)


def test_small_mesh_dumps_every_node():
    out = bench.dump_outputs(FakeSim(1067))
    assert sorted(out) == ["c", "nodes", "p", "u"]
    assert all(v.dtype == np.float64 for v in out.values())
    assert np.array_equal(out["nodes"], np.arange(1067))
    assert out["u"].shape == (1067, 2) and out["p"].shape == (1067,) and out["c"].shape == (1067,)


def test_large_mesh_dumps_a_fixed_sample(monkeypatch):
    monkeypatch.setattr(bench, "DUMP_NODES", 100)
    a, b = bench.dump_outputs(FakeSim(1001)), bench.dump_outputs(FakeSim(1001))
    idx = a["nodes"].astype(np.int64)
    assert len(idx) == 100 and len(np.unique(idx)) == 100 and idx.min() >= 0 and idx.max() < 1001
    assert np.array_equal(idx, np.sort(idx))
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # the fields are taken at the sampled nodes
    assert np.array_equal(a["u"][:, 0], idx) and np.array_equal(a["p"], 2.0 * idx) and np.array_equal(a["c"], idx + 0.5)


def test_dump_size_at_the_benchmark_mesh():
    n = bench.DUMP_NODES  # u (n, 2), p, c and the node list, float64
    assert 5 * 8 * n <= 64 * 2 ** 20
