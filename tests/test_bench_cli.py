"""bench.py's --dump-outputs and --full.

CPU: _dump_outputs on a stand-in for Sim (interior points only, the seeded
sample, float64 files).  GPU: one small plain run with --dump-outputs, whose
result line has no CPU baseline and whose files match the grid asked for.
"""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


class _FakeSim:
    """Grids in Sim.grid()'s layout ([nz+2, ny+2, nx+2, nValues]); interior
    values are the flat interior index (+ component), ghosts are NaN."""
    ndims, nspecies = 3, 2

    def __init__(self, n):
        self.n = n

    def grid(self, which):
        n, nv = self.n, 3 if which == 2 else 1
        g = np.full((n + 2, n + 2, n + 2, nv), np.nan)
        g[1:-1, 1:-1, 1:-1] = (np.arange(n ** 3, dtype=np.float64).reshape(n, n, n, 1) * (which + 1)
                               + 0.25 * np.arange(nv))
        return g

    def energy(self):
        return 3.0, 4.0, np.array([1.0, 2.0])

    def count(self, s):
        return 10 + s


def test_dump_outputs_whole_grid(tmp_path):
    import bench
    n = 6
    bench._dump_outputs(_FakeSim(n), tmp_path / "d", 0)
    got = {f.name: np.load(f) for f in (tmp_path / "d").iterdir()}
    assert sorted(got) == ["E.npy", "counts.npy", "energy.npy", "phi.npy", "rho.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    flat = np.arange(n ** 3, dtype=np.float64)
    assert np.array_equal(got["rho.npy"], flat[:, None])
    assert np.array_equal(got["phi.npy"], 2 * flat[:, None])
    assert np.array_equal(got["E.npy"], 3 * flat[:, None] + 0.25 * np.arange(3))
    assert np.array_equal(got["energy.npy"], [3.0, 4.0, 1.0, 2.0])
    assert np.array_equal(got["counts.npy"], [10.0, 11.0])


def test_dump_outputs_sample_is_fixed(tmp_path, monkeypatch):
    import bench
    n = 8
    monkeypatch.setattr(bench, "DUMP_POINTS", 100)
    bench._dump_outputs(_FakeSim(n), tmp_path / "a", 0)
    bench._dump_outputs(_FakeSim(n), tmp_path / "b", 1)
    pts = np.load(tmp_path / "a" / "grid_points.npy")
    assert pts.dtype == np.float64 and pts.shape == (100,)
    assert np.all(np.diff(pts) > 0) and pts[0] >= 0 and pts[-1] < n ** 3
    assert np.array_equal(pts, np.load(tmp_path / "b" / "grid_points.rank1.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "rho.npy"), pts[:, None])
    assert np.array_equal(np.load(tmp_path / "a" / "E.npy"), 3 * pts[:, None] + 0.25 * np.arange(3))
    assert np.array_equal(np.load(tmp_path / "b" / "phi.rank1.npy"), 2 * pts[:, None])


def test_dump_at_the_default_workload_fits_64_mb():
    import bench
    # rho, phi (1 value), E (3 values) and the point list, 8 bytes each, plus .npy headers
    assert bench.DUMP_POINTS * 8 * (1 + 1 + 3 + 1) + 6 * 4096 <= 64 * 10 ** 6


@pytest.mark.gpu
def test_plain_run_dumps_and_skips_the_cpu_baseline(built, tmp_path):
    S, steps = 32, 3
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--size", str(S), "--ppc", "4", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["steps"] == steps and res["ms_per_step"] > 0
    assert abs(res["value"] - res["config"]["particles"] * 1e3 / res["ms_per_step"]) <= 1e-9 * res["value"]
    assert res["cpu_baseline"] is None
    got = {f.name: np.load(f) for f in (tmp_path / "out").iterdir()}
    assert sorted(got) == ["E.npy", "counts.npy", "energy.npy", "phi.npy", "rho.npy"]
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in got.values())
    assert got["rho.npy"].shape == got["phi.npy"].shape == (S ** 3, 1) and got["E.npy"].shape == (S ** 3, 3)
    assert got["energy.npy"][0] == res["energy"]["KE"] and got["energy.npy"][1] == res["energy"]["PE"]
    assert got["counts.npy"].sum() == res["config"]["particles"]
    assert np.abs(got["E.npy"]).max() > 0
