"""Ionisation on two ranks (z-slabs of an 8 x 8 x 16 grid, host transport over
gloo on one GPU, launched as tests/test_gpu_collide_ranks.py launches its
workers): each rank's draws come from its own key,
pinc_hip_ionize_key(seed, call, rank, s).

Every rank sets velocities of its own and runs op("ionize") once
(tests/ionize_worker.py; call 1, the init sequence made call 0).  Each rank's
births are compared with tests/ionize_ref.py under that rank's key, slot for
slot at the kernel test's tolerance; the two ranks' ionisers differ; and the
global counts after the step are the sums.
"""
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ionize_ref as IR
from pinc_amd import configs

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SEED = 43
PAR = IR.Params(nu=0.06, wth=0.0, vth=0.02, drift=(0.0, 0.01, 0.0), target=1)


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_each_rank_ionises_with_its_own_key(built, tmp_path):
    cfg = configs.config("warm", true_size=(8, 8, 8), nsub=(1, 1, 2), ppc=8, nalloc_pc=16, levels=2)
    cfg["collisions"] = {"ionNu": "0.06,0", "ionSpecies": "1,0", "neutralVth": "0.02", "neutralDrift": "0,0.01,0",
                         "seed": str(SEED)}
    ini = configs.write_ini(cfg)
    out = tmp_path / "out"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2", PYTHONPATH=str(ROOT))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", str(ROOT / "tests" / "ionize_worker.py"),
           "ranks", "--ini", ini, "--out", str(out)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    os.unlink(ini)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    ranks = [np.load(f"{out}_r{r}.npz") for r in range(2)]

    hits, before, after, born = [], 0, 0, 0
    for r, g in enumerate(ranks):
        pos, vel, ipos, ivel = g["x0_0"], g["v0_0"], g["x0_1"], g["v0_1"]
        n, ni = len(vel), len(ivel)
        assert n >= 8 ** 3 * 8
        ref = IR.ionize(vel, PAR, IR.key(SEED, 1, r, 0))
        assert IR.min_margin(ref) > 1e-9
        nb = ref.births
        assert g["births"].tolist() == [nb, 0] and nb > 50, (r, g["births"], nb)
        assert g["count"].tolist() == [n + nb, ni + nb]
        bound = IR.bound(ref, PAR, 3)
        x, v, ix, iv = g["x1_0"], g["v1_0"], g["x1_1"], g["v1_1"]
        np.testing.assert_array_equal(x[:n], pos)
        np.testing.assert_array_equal(np.any(v[:n] != vel, axis=1), ref.hit)
        np.testing.assert_array_equal(x[n:], pos[ref.parents])
        np.testing.assert_array_equal(ix, np.concatenate([ipos, pos[ref.parents]]))
        np.testing.assert_array_equal(iv[:ni], ivel)
        for got, want, what in ((v[:n][ref.parents], ref.vel[ref.parents], "parents"), (v[n:], ref.electrons, "electrons"),
                                (iv[ni:], ref.ions, "ions")):
            ratio = float(np.max(np.abs(got.astype(IR.LD) - want) / bound))
            print(f"rank {r}, {what}: largest error / bound = {ratio:.4f}")
            assert ratio <= 1.0, (r, what)
        hits.append(ref.hit)
        before, after, born = before + n + ni, after + int(g["count"].sum()), born + nb
    assert after == before + 2 * born
    m = min(len(hits[0]), len(hits[1]))
    assert np.any(hits[0][:m] != hits[1][:m])
