"""Processes of the ionisation tests (tests/test_gpu_ionize_sim.py,
tests/test_gpu_ionize_ranks.py).

    ionize_worker.py ranks --ini I --out O    one rank of a two-rank run (under
        torch.distributed.run; gloo moves the data, every rank on cuda:0): sets
        its own velocities, runs op("ionize") once and saves every species
        before and after it, and its births
    ionize_worker.py pending --ini I          mccIonize with a fused push pending

The last ends in msg(ERROR), which exits the process; it prints "REACHED-END"
if it did not.
"""
import argparse
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def ranks(args) -> int:
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    import torch.distributed as dist
    dist.init_process_group("gloo")
    from pinc_amd import Sim
    from pinc_amd.transport import GlooTransport
    out = {}
    with Sim(args.ini, rank=rank, nranks=world, device=0, transport=GlooTransport(), maxwell=True, perturb=False,
             seed=5) as s:
        s.init()                    # (the init sequence ionises once: the op below is call 1)
        rng = np.random.default_rng(700 + rank)
        for sp in range(s.nspecies):
            pos, _ = s.particles(sp)
            vel = 0.15 * rng.standard_normal(pos.shape)
            s.set_particles(sp, pos, vel)
            out[f"x0_{sp}"], out[f"v0_{sp}"] = pos, vel
        before = s.ionizations(0)
        s.op("ionize")
        for sp in range(s.nspecies):
            out[f"x1_{sp}"], out[f"v1_{sp}"] = s.particles(sp)
        out["births"] = np.array([s.ionizations(0) - before, s.ionizations(1)])
        out["count"] = np.array([s.count(sp) for sp in range(s.nspecies)])
    np.savez(f"{args.out}_r{rank}.npz", **out)
    dist.barrier()
    dist.destroy_process_group()
    return 0


def pending(args) -> int:
    from pinc_amd import Sim
    with Sim(args.ini, maxwell=True, perturb=False, seed=5) as s:
        s.init()                    # ends with the fused puAcc: its move is pending
        s.op("ionize")
    print("REACHED-END", flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("kind", choices=["ranks", "pending"])
    ap.add_argument("--ini", required=True)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    return {"ranks": ranks, "pending": pending}[args.kind](args)


if __name__ == "__main__":
    sys.exit(main())
