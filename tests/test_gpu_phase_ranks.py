"""Phase-space histograms on two ranks (z-slabs, host transport over gloo on
one GPU, launched as tests/test_gpu_moments_ranks.py launches its workers):
16^3 cells, 2 steps, axes (z, vz), so that the sharded dimension is binned.
All comparisons are exact:
  * both ranks return the same array;
  * it equals tests/phase_ref.py of the ranks' particles in the global frame
    (the worker saves local positions and its offset; they are added here in
    fp64, the addition the kernel makes);
  * it equals a one-rank Sim given those global-frame particles through
    set_particles (in that Sim's own local frame).
"""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import phase_ref as PR
from pinc_amd import configs

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
# global-frame z lies in [-0.5, 15.5); a range narrower than the data in vz
SPEC = (("z", "vz"), (64, 32), (-0.5, -0.12), (15.5, 0.12))


def _cfg(nsub):
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
    axes, bins, lo, hi = SPEC
    ini2 = configs.write_ini(_cfg(2))
    out = tmp_path / "out"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2", PYTHONPATH=str(ROOT))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", str(ROOT / "tests" / "phase_worker.py"),
           "--ini", ini2, "--out", str(out), "--steps", "2", "--spec", json.dumps(SPEC)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    os.unlink(ini2)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    ranks = [np.load(f"{out}_r{r}.npz") for r in range(2)]
    assert ranks[0]["offset"][2] != ranks[1]["offset"][2]

    ini1 = configs.write_ini(_cfg(1))
    try:
        with Sim(ini1, maxwell=True, perturb=False, seed=5) as s:
            s.init()
            for sp in range(2):
                # global frame: local + offset, in fp64
                gpos = np.concatenate([g[f"pos{sp}"] + g["offset"].astype(np.float64) for g in ranks])
                vel = np.concatenate([g[f"vel{sp}"] for g in ranks])
                h0, h1 = ranks[0][f"hist{sp}"], ranks[1][f"hist{sp}"]
                np.testing.assert_array_equal(h0, h1)
                assert ranks[0][f"outside{sp}"] == ranks[1][f"outside{sp}"]
                ref, ref_out = PR.sim_histogram(gpos, vel, (0, 0, 0), axes, bins, lo, hi)
                np.testing.assert_array_equal(h0, ref)
                assert float(ranks[0][f"outside{sp}"]) == ref_out and ref_out > 0
                assert h0.sum() + ref_out == len(gpos)
                # the one-rank Sim holds them in its own local frame
                s.set_particles(sp, gpos - s.offset.astype(np.float64), vel)
                one, one_out = s.phase_space(sp, axes, bins, lo, hi)
                np.testing.assert_array_equal(one, h0)
                assert one_out == ref_out
    finally:
        os.unlink(ini1)
