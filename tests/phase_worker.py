"""One rank of the two-rank phase-space run (launched by
tests/test_gpu_phase_ranks.py through torch.distributed.run; gloo moves the
data, every rank on cuda:0).  Runs `--steps` steps and saves this rank's
particles (local frame), its offset and the (z, vz) histogram of every
species as this rank received it.
"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ini", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--spec", required=True, help="JSON: [axes, bins, lo, hi]")
    ap.add_argument("--steps", type=int, default=2)
    args = ap.parse_args()
    axes, bins, lo, hi = json.loads(args.spec)
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    import torch.distributed as dist
    dist.init_process_group("gloo")
    from pinc_amd import Sim
    from pinc_amd.transport import GlooTransport
    out = {}
    with Sim(args.ini, rank=rank, nranks=world, device=0, transport=GlooTransport(), maxwell=True, perturb=False,
             seed=5) as s:
        s.init()
        s.step(args.steps)
        out["offset"] = s.offset
        for sp in range(s.nspecies):
            h, o = s.phase_space(sp, axes, bins, lo, hi)      # collective: summed over the ranks
            out[f"hist{sp}"], out[f"outside{sp}"] = h, np.float64(o)
            out[f"pos{sp}"], out[f"vel{sp}"] = s.particles(sp)
    np.savez(f"{args.out}_r{rank}.npz", **out)
    dist.barrier()
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
