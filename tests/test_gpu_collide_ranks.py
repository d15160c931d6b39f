"""Collisions on two ranks (z-slabs, host transport over gloo on one GPU,
launched as tests/test_gpu_moments_ranks.py launches its workers): each
rank's draws come from its own key, pinc_hip_collide_key(seed, step, rank, s).

Every rank sets velocities of its own, runs op("collide") twice and saves the
velocities in between (tests/collide_worker.py).  Each collision step is
compared with tests/collide_ref.py under that rank's key at the kernel test's
tolerance, counters exactly; and the two ranks' collider sets differ.
"""
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import collide_ref as CR
from pinc_amd import configs

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
MN = 16.0 * 1836.0
SEED = 41
PARAMS = [CR.Params(nu=(0.06, 0.0), b=MN / (1.0 + MN), vth=0.02, drift=(0.0, 0.01, 0.0)),
          CR.Params(nu=(0.03, 0.05), sig=(0.0, 0.3), b=MN / (1836.0 + MN), vth=0.02, drift=(0.0, 0.01, 0.0))]


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_each_rank_draws_from_its_own_key(built, tmp_path):
    cfg = configs.bench_config("c4", size=16, ppc=8, world=2, mg="plain", layout="reference")
    cfg["multigrid"]["mgLevels"] = "3"
    cfg["population"]["nAlloc"] = "16 pc"
    cfg["collisions"] = {"elasticNu": "0.06,0.03", "cexNu": "0,0.05", "cexSigma": "0,0.3", "neutralMass": repr(MN),
                         "neutralVth": "0.02", "neutralDrift": "0,0.01,0", "seed": str(SEED)}
    ini = configs.write_ini(cfg)
    out = tmp_path / "out"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2", PYTHONPATH=str(ROOT))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", str(ROOT / "tests" / "collide_worker.py"),
           "ranks", "--ini", ini, "--out", str(out)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    os.unlink(ini)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    ranks = [np.load(f"{out}_r{r}.npz") for r in range(2)]

    hits = [[], []]
    worst = 1.0
    for r, g in enumerate(ranks):
        for sp in range(2):
            total = [0, 0]
            for step in (0, 1):
                vin, got = g[f"v{step}_{sp}"], g[f"v{step + 1}_{sp}"]
                assert len(vin) > 10000
                res = CR.collide(vin, PARAMS[sp], CR.key(SEED, step, r, sp))
                worst = min(worst, CR.min_margin(res))
                CR.check(got, vin, res, PARAMS[sp], f"rank {r}, species {sp}, step {step}")
                total = [total[k] + res.counts[k] for k in range(2)]
                if step == 0:
                    hits[r].append(res.proc >= 0)
            assert g["counts"][sp].tolist() == total, (r, sp)
    assert worst > 1e-9, worst
    for sp in range(2):
        m = min(len(hits[0][sp]), len(hits[1][sp]))
        a, b = hits[0][sp][:m], hits[1][sp][:m]
        assert a.sum() > 0 and b.sum() > 0 and np.any(a != b)
