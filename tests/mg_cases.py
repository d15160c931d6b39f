"""Shapes and inputs shared by tests/test_gpu_mg_transfer_kernels.py (the
kernels of k_mg.hip against tests/mg_ref.py) and tests/test_mg_ref_cpu.py
(which proves, without a GPU, that these shapes and inputs tell deliberate
mutants of the restatement apart).  Shapes are (Tx, Ty, Tz); arrays are
[z][y][x].
"""
import numpy as np

# coarse shapes of the restriction.  (30, 20, 12): 7200 coarse points are 8
# blocks, point_walk's XCD path with a ragged last eighth
RESTRICT_COARSE = [(2, 2, 2), (3, 5, 7), (16, 4, 2), (30, 20, 12),
                   (2, 2), (5, 3), (64, 8),
                   (2,), (7,), (4100,)]

# fine shapes of the prolongation.  (158, 128, 130): more than 2048 * 1024
# points, so the block cap holds and the eighths are ragged
BIG = (158, 128, 130)
PROLONG_FINE = [(4, 4, 4), (6, 10, 14), (32, 8, 4), (30, 20, 12), BIG,
                (4, 4), (6, 10), (32, 8), (30, 20), (158, 128),
                (4,), (6,), (32,), (30,), (158,)]

# residual and its sum of squares: (shape, arrays offset by 8 bytes)
RESIDUAL = [((15,), 0), ((4100,), 0), ((5, 3), 0), ((64, 16), 0), ((30, 20), 0),
            ((15, 6, 4), 0), ((16, 6, 4), 1), ((30, 20, 12), 0), (BIG, 0), (BIG, 1)]

RESID_RESTRICT_FINE = [(4, 4, 4), (6, 10, 14), (32, 8, 16)]

GS_SHAPES = [(4, 2, 2), (6, 10, 4), (32, 8, 16), (2, 2), (6, 10), (128, 2), (2,), (10,), (4096,)]

# mg_coarse: (levels, hw3d, gs3d); nPre = nPost = 4, nCoarse = 10
COARSE_SMOOTH = (4, 4, 10)
COARSE = [
    ([(16, 16, 16), (8, 8, 8), (4, 4, 4), (2, 2, 2)], 1, 1),
    ([(16, 16, 16), (8, 8, 8), (4, 4, 4), (2, 2, 2)], 0, 0),
    ([(16, 8, 4), (8, 4, 2)], 1, 1),
    ([(4, 4, 4)], 1, 1),
    ([(32, 16), (16, 8), (8, 4), (4, 2)], 0, 0),
    ([(64,), (32,), (16,), (8,), (4,), (2,)], 0, 0),
]

# sharded level 0: (T, P ranks, hz halo planes)
SLABS = [((8, 4, 16), 2, 2), ((12, 6, 8), 4, 3), ((8, 8, 8), 1, 3), ((16, 16, 32), 2, 24)]


# one seed per operator, so both files see the same inputs
SEED = {"restrict": 11, "prolong": 12, "residual": 13, "resid_restrict": 14, "gs": 15, "coarse": 16, "slab": 17}


def fields(shapes, seed):
    """seeded standard normals, one [z][y][x] array per (Tx, Ty, Tz) shape"""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(tuple(s)[::-1]) for s in shapes]


def coarse_reference(case):
    """A case of COARSE: its source, the restated cycle in fp64, d = max |fp64
    - long double| of the restatement alone, and the bound on the kernel's
    deviation from the fp64 cycle: 16 d (the workgroup's neutralisation sums
    run in another order than numpy's; one reordered sum of at most 4096 terms
    per neutralisation perturbs the result by no more than rounding already
    does), but not below 64 eps max |phi|."""
    import mg_ref as MR
    levels, hw3d, gs3d = case
    (rho,) = fields([levels[0]], SEED["coarse"])
    pre, post, nc = COARSE_SMOOTH
    ref = MR.coarse_cycle(rho, levels, pre, post, nc, hw3d, gs3d, np.float64)
    hi = MR.coarse_cycle(rho, levels, pre, post, nc, hw3d, gs3d, np.longdouble)
    d = float(np.max(np.abs(ref - hi)))
    tol = max(16 * d, 64 * np.finfo(np.float64).eps * float(np.max(np.abs(ref))))
    return rho, ref, d, tol


def coarse_of(shape):
    return tuple(t // 2 for t in shape)


def fine_of(shape):
    return tuple(2 * t for t in shape)
