"""Velocity moments on two ranks (z-slabs, host transport over gloo on one
GPU, launched as tests/test_gpu_multirank.py launches its workers): 16^3
cells, 2 steps.

The halo fold across ranks is checked twice, within moments_ref's bound
(k + 8) eps sum|terms|:
  * against tests/moments_ref.py of each rank's own particles, the ghost
    planes folded into the neighbouring rank's true planes;
  * the ranks' true-node moments, concatenated along z, against a one-rank
    Sim's moments of the same particles.  The one-rank Sim is given the
    two-rank run's particles (global frame): two separately stepped runs
    agree only to the Poisson solver's tolerance (1e-9 in the velocities),
    which is not what this test is about.
"""
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import moments_ref as MR
from pinc_amd import configs

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NLOC = 8


def _cfg(nsub):
    """the bench's warm plasma (v_th = 0.05 cells/step) at 16^3, 16 particles
    per cell and species, reference layout, fused push, plain multigrid"""
    cfg = configs.bench_config("c4", size=16, ppc=16, world=nsub, mg="plain", layout="reference")
    cfg["multigrid"]["mgLevels"] = "3"
    cfg["population"]["nAlloc"] = "32 pc"
    return cfg


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_match_reference_and_one_rank(built, tmp_path):
    from pinc_amd import Sim
    ini2 = configs.write_ini(_cfg(2))
    out = tmp_path / "out"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2", PYTHONPATH=str(ROOT))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", str(ROOT / "tests" / "moments_worker.py"),
           "--ini", ini2, "--out", str(out), "--steps", "2"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    os.unlink(ini2)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    ranks = [np.load(f"{out}_r{r}.npz") for r in range(2)]

    geom_r = (16, 16, NLOC)
    for sp in range(2):
        refs = [MR.moments_reference(g[f"pos{sp}"], g[f"vel{sp}"], geom_r) for g in ranks]
        for r in range(2):
            o = refs[1 - r]                # the neighbour above and below (two periodic slabs)
            fold = {}
            for key in ("M", "A", "k"):
                a = getattr(refs[r], key).copy()
                a[1] += getattr(o, key)[NLOC + 1]
                a[NLOC] += getattr(o, key)[0]
                fold[key] = a[1:NLOC + 1]
            M = ranks[r][f"mom{sp}"]
            assert M.shape == (NLOC, 16, 16, 10)
            MR.check(M, MR.SimpleNamespace(**fold), f"rank {r}, species {sp}")

    ini1 = configs.write_ini(_cfg(1))
    try:
        with Sim(ini1, maxwell=True, perturb=False, seed=5) as s:
            s.init()
            for sp in range(2):
                pos = np.concatenate([g[f"pos{sp}"] + np.array([0.0, 0.0, r * NLOC])
                                      for r, g in enumerate(ranks)])
                vel = np.concatenate([g[f"vel{sp}"] for g in ranks])
                s.set_particles(sp, pos, vel)
            for sp in range(2):
                one = s.moments(sp)
                pos, vel = s.particles(sp)
                ref = MR.folded(MR.moments_reference(pos, vel, (16, 16, 16)), 16)
                MR.check(one, ref, f"one rank, species {sp}")
                two = np.concatenate([g[f"mom{sp}"] for g in ranks], axis=0)
                assert two.shape == one.shape == (16, 16, 16, 10)
                MR.check(two, ref, f"two ranks against the one-rank particles, species {sp}")
                lim = (2 * (ref.k[..., None] + 8) * MR.EPS * ref.A).astype(np.float64)
                assert np.all(np.abs(two - one) <= lim)
    finally:
        os.unlink(ini1)
