"""Processes of the collision tests (tests/test_gpu_collide_sim.py,
tests/test_gpu_collide_ranks.py).

    collide_worker.py ranks --ini I --out O    one rank of a two-rank run (under
        torch.distributed.run; gloo moves the data, every rank on cuda:0): sets
        its own particles, runs op("collide") twice and saves the velocities
        before and after each, and its counters
    collide_worker.py pending --ini I          mccCollide with a fused push pending
    collide_worker.py create --ini I           only creates the Sim (bad ini values)
    collide_worker.py maxvel --ini I           two steps with neutrals above population:maxVel

The last three end in msg(ERROR), which exits the process (io.c:214-215); they
print "REACHED-END" if it did not.
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
        s.init()
        rng = np.random.default_rng(900 + rank)
        for sp in range(s.nspecies):
            pos, _ = s.particles(sp)
            vel = 0.1 * rng.standard_normal(pos.shape)
            s.set_particles(sp, pos, vel)
            out[f"v0_{sp}"] = vel
        for step in (1, 2):
            s.op("collide")
            for sp in range(s.nspecies):
                out[f"v{step}_{sp}"] = s.particles(sp)[1]
        out["counts"] = np.array([s.collisions(sp) for sp in range(s.nspecies)])
    np.savez(f"{args.out}_r{rank}.npz", **out)
    dist.barrier()
    dist.destroy_process_group()
    return 0


def pending(args) -> int:
    from pinc_amd import Sim
    with Sim(args.ini, maxwell=True, perturb=False, seed=5) as s:
        s.init()                    # ends with the fused puAcc: its move is pending
        s.op("collide")
    print("REACHED-END", flush=True)
    return 0


def maxvel(args) -> int:
    from pinc_amd import Sim
    with Sim(args.ini, maxwell=True, perturb=False, seed=5) as s:
        s.init()
        s.step(2)                   # every ion takes a neutral drifting above population:maxVel
    print("REACHED-END", flush=True)
    return 0


def create(args) -> int:
    from pinc_amd import Sim
    with Sim(args.ini):
        pass
    print("REACHED-END", flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("kind", choices=["ranks", "pending", "create", "maxvel"])
    ap.add_argument("--ini", required=True)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    return {"ranks": ranks, "pending": pending, "create": create, "maxvel": maxvel}[args.kind](args)


if __name__ == "__main__":
    sys.exit(main())
