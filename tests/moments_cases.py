"""The particle populations shared by the GPU tests of the particle-to-grid
kernels (tests/test_gpu_moments_kernel.py, tests/test_gpu_deposit_kernel.py),
each with its reference (tests/moments_ref.py).  No GPU.
"""
import functools

import numpy as np

import moments_ref as MR
import push_ref as R

TW = 4


def extremes(geom, rng):
    """particles in cell 0 and in cell T of each dimension (the others mid
    domain), and in the lowest and the highest corner cell"""
    nd = len(geom)
    mid = np.array([t // 2 + 0.375 for t in geom])
    rows = []
    for d in range(nd):
        for x in (0.25, geom[d] + 0.75):
            p = mid.copy()
            p[d] = x
            rows.append(p)
    rows.append(np.full(nd, 0.625))
    rows.append(np.array([t + 0.125 for t in geom]))
    pos = np.array(rows)
    return pos, rng.uniform(-0.9, 0.9, size=pos.shape)


@functools.lru_cache(maxsize=None)
def case(name):
    """(geom, pos, vel, reference): made once, shared, never modified"""
    rng = np.random.default_rng({"uniform3d": 11, "sorted3d": 12, "edge3d": 13, "2d": 14, "1d": 15}[name])
    if name == "uniform3d":
        geom = (8, 8, 8)
        pos, vel = R.uniform_particles(geom, 5000, rng, R.V_MAX)
    elif name in ("sorted3d", "edge3d"):
        geom = (16, 8, 8)
        pos, vel = R.uniform_particles(geom, 20000, rng, R.V_MAX)
        pos, vel = R.cell_sorted(pos, vel, geom, TW)
        if name == "edge3d":
            pe, ve = R.edge_particles(geom)
            px, vx = extremes(geom, rng)
            pos, vel = np.concatenate([pos, pe, px]), np.concatenate([vel, ve, vx])
    elif name == "2d":
        geom = (16, 16)
        pos, vel = R.uniform_particles(geom, 6000, rng, R.V_MAX)
        pos, vel = R.cell_sorted(pos, vel, geom, 8)
        pe, ve = R.edge_particles(geom)
        px, vx = extremes(geom, rng)
        pos, vel = np.concatenate([pos, pe, px]), np.concatenate([vel, ve, vx])
    else:
        geom = (64,)
        pos, vel = R.uniform_particles(geom, 5000, rng, R.V_MAX)
        px, vx = extremes(geom, rng)
        pos, vel = np.concatenate([pos, px]), np.concatenate([vel, vx])
    for a in (pos, vel):
        a.setflags(write=False)
    return geom, pos, vel, MR.moments_reference(pos, vel, geom)
