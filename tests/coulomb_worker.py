"""One rank of a two-rank run of the Coulomb collision test
(tests/test_gpu_coulomb_ranks.py; under torch.distributed.run, gloo moves the
data, every rank on cuda:0): runs op("coulomb") once after the init sequence
and saves its particles before and after, its counters, coefficients and masses.

    coulomb_worker.py --ini I --out O
"""
import argparse
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ini", required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    import torch.distributed as dist
    dist.init_process_group("gloo")
    from pinc_amd import Sim
    from pinc_amd.transport import GlooTransport
    pairs = ((0, 0), (0, 1), (1, 1))
    out = {}
    with Sim(args.ini, rank=rank, nranks=world, device=0, transport=GlooTransport(), maxwell=True, perturb=False,
             seed=5) as s:
        s.init()
        out["count0"] = np.array([s.coulomb_count(a, b) for a, b in pairs])
        for sp in range(2):
            out[f"x_{sp}"], out[f"v0_{sp}"] = s.particles(sp)
        s.op("coulomb")
        for sp in range(2):
            x, out[f"v1_{sp}"] = s.particles(sp)
            assert np.array_equal(x, out[f"x_{sp}"])
        out["count1"] = np.array([s.coulomb_count(a, b) for a, b in pairs])
        out["K"] = np.array([s.coulomb_coef(a, b) for a, b in pairs])
        out["mass"] = s.species()[1]
    np.savez(f"{args.out}_r{rank}.npz", **out)
    dist.barrier()
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
