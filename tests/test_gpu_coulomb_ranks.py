"""Coulomb collisions on two ranks (z-slabs, host transport over gloo on one
GPU, launched as tests/test_gpu_collide_ranks.py launches its workers).  After
the migration every cell belongs to one rank, so a rank pairs its own
particles alone, under its own key pinc_hip_coulomb_key(seed, step, rank, a, b).

Only the unlike pair (0, 1) has a logarithm, so an op is one launch.  Every
rank runs op("coulomb") once after the init sequence (which collided
once: call 1) and saves its particles before and after
(tests/coulomb_worker.py).  Each rank's result is compared with
tests/coulomb_ref.py on that rank's particles, its 16 x 16 x 8 true cells and
its key, at the kernel test's bound, counters and collider sets exactly; and
the momentum summed over both ranks moves by no more than the kernel test's
8 P eps sum m |w| with P = 8.
"""
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import coulomb_ref as CR
from pinc_amd import configs

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SEED = 43
T = (16, 16, 8)
LD = np.longdouble


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_each_rank_pairs_its_own_cells(built, tmp_path):
    cfg = configs.bench_config("c4", size=16, ppc=4, world=2, mg="plain", layout="reference")
    cfg["multigrid"]["mgLevels"] = "3"
    cfg["population"]["nAlloc"] = "8 pc"
    cfg["population"]["fused"] = "0"       # no move is pending after the init sequence: the op may run
    cfg["collisions"] = {"coulombLog": "0,12,12,0", "seed": str(SEED)}
    ini = configs.write_ini(cfg)
    out = tmp_path / "out"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2", PYTHONPATH=str(ROOT))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", str(ROOT / "tests" / "coulomb_worker.py"),
           "--ini", ini, "--out", str(out)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    os.unlink(ini)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    ranks = [np.load(f"{out}_r{r}.npz") for r in range(2)]

    mom, scale = np.zeros(3, dtype=LD), LD(0)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    for r, g in enumerate(ranks):
        m = g["mass"]
        assert g["K"][0] == 0 and g["K"][1] > 0 and g["K"][2] == 0
        assert g["count0"][1] > 0 and g["count1"][0] == g["count1"][2] == 0
        assert len(g["x_0"]) > 3000
        mu = m[0] * m[1] / (m[0] + m[1])
        par = CR.Params(K=float(g["K"][1]), fa=mu / m[0], fb=mu / m[1])
        res = CR.coulomb(g["x_0"], g["v0_0"], g["x_1"], g["v0_1"], par, CR.key(SEED, 1, r, 0, 1), T)
        for v in ("var", "gp", "g"):
            assert res.margins[v] > 1e-9, (r, v, res.margins)
        assert res.margins["hash_gap"] >= 1
        assert g["count1"][1] - g["count0"][1] == res.count > 0, r
        for sp in range(2):
            got, vin = g[f"v1_{sp}"], g[f"v0_{sp}"]
            changed = np.any(bits(got) != bits(vin), axis=1)
            np.testing.assert_array_equal(changed, res.collider[sp], err_msg=f"rank {r}, species {sp}")
            err = np.abs(got.astype(LD) - res.vel[sp]).astype(np.float64)
            assert np.all(err <= CR.EPS * res.bound[sp][:, None]), (r, sp)
            mom += m[sp] * (np.sum(got.astype(LD), 0) - np.sum(vin.astype(LD), 0))
            scale += m[sp] * np.sum(np.abs(vin).astype(LD))
    print("global momentum change / (eps sum m|v|):", (mom / (CR.EPS * scale)).astype(float))
    assert np.all(np.abs(mom) <= 8 * 8 * CR.EPS * scale)
    # the two ranks draw from different keys
    assert CR.key(SEED, 1, 0, 0, 1) != CR.key(SEED, 1, 1, 0, 1)
