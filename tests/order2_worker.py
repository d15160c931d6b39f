"""Worker of tests/test_gpu_order2_sim.py.

--mode ranks     one rank of the two-rank order-2 deposit (launched through
                 torch.distributed.run; gloo moves the data, every rank on
                 cuda:0): takes the particles of --particles (global frame:
                 local + Sim.offset) that lie in this rank's slab, deposits them (op distr: the
                 deposit and the halo exchange) and saves its true-node rho.
--mode energies  a fresh process: --steps steps of the ini as it stands, the
                 energies of every step saved.
"""
import argparse
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["ranks", "energies"])
    ap.add_argument("--ini", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--particles")
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    from pinc_amd import Sim
    if args.mode == "energies":
        rows = []
        with Sim(args.ini) as s:
            s.init()
            for _ in range(args.steps):
                s.step()
                ke, pe, _ = s.energy()
                rows.append((ke, pe))
        np.save(args.out, np.array(rows))
        return 0
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    import torch.distributed as dist
    dist.init_process_group("gloo")
    from pinc_amd.transport import GlooTransport
    parts = np.load(args.particles)
    with Sim(args.ini, rank=rank, nranks=world, device=0, transport=GlooTransport()) as s:
        s.init()
        nd = s.ndims
        nloc = s.grid_shape(0)[nd] - 2
        # global frame = local frame + Sim.offset, per dimension
        off = s.offset.astype(np.float64)
        for sp in range(s.nspecies):
            loc = parts[f"pos{sp}"] - off
            zl = loc[:, nd - 1]
            loc = loc[(zl >= 0.5) & (zl < nloc + 0.5)]
            s.set_particles(sp, loc, np.zeros_like(loc))
        s.op("distr")
        rho = s.grid(0)
        np.save(f"{args.out}_r{rank}.npy", rho[1:-1, 1:-1, 1:-1, 0])
    dist.barrier()
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
