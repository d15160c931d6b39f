"""Shapes and inputs shared by tests/test_gpu_grid_kernels.py and
tests/test_gpu_spectral_kernels.py (the kernels of k_grid.hip and
k_spectral.hip against tests/field_ref.py) and tests/test_field_ref_cpu.py
(which shows, without a GPU, that these shapes and inputs tell deliberate
mutants of the restatement apart).  Shapes are (Tx, Ty, Tz); arrays are
[z][y][x]; a geometry is (T, off, nloc), the slab dimension the last of T.
"""
import numpy as np

import field_ref as FR

F64 = np.float64
LD = np.longdouble
EPS = float(np.finfo(F64).eps)


def whole(*T):
    return (tuple(T), 0, T[-1])


# k_efield_planes puts slab plane p on blockIdx.y: nloc + 2 = 65535 is the
# last size it serves, from nloc + 2 = 65536 on k_efield (grid stride) runs
PLANES_LAST = whole(65533)
FALLBACK = [whole(65534), whole(3, 65534), whole(2, 3, 65534)]

SMALL_GEOMS = [
    whole(2), whole(7), ((64,), 16, 16), ((64,), 48, 16),
    whole(2, 2), whole(5, 3), ((30, 20), 5, 5), ((30, 20), 15, 5),
    whole(2, 2, 2), whole(3, 5, 7), ((30, 20, 12), 4, 4), ((30, 20, 12), 8, 4), ((16, 16, 3), 1, 1),
]
# nloc == 1 in every dimension count: both adds of the fold land in plane 1
NLOC1 = [((5,), 2, 1), ((5, 3), 1, 1), ((16, 16, 3), 1, 1)]

GEOMS = SMALL_GEOMS + [whole(4100), whole(30, 20), whole(30, 20, 12), PLANES_LAST] + FALLBACK
FOLD_GEOMS = SMALL_GEOMS + [g for g in NLOC1 if g not in SMALL_GEOMS] + [whole(30, 20, 12)]
H = [0.5, -0.5]
NVALUES = [1, 3]

# the last hits k_sum's 1024-block cap with a ragged tail
N_ELEMENTS = [1, 63, 255, 256, 257, 4099, 1024 * 256 * 8 + 77]

SPECTRAL = [(2,), (8,), (16,), (2, 2), (8, 5), (6, 16), (2, 2, 2), (8, 5, 7), (4, 6, 3), (16, 8, 4)]
# (T, P): nloc = Tz / P planes and Tyl = Ty / P rows of ky per rank
SLAB_SPECTRAL = [((8, 6, 9), 3), ((4, 4, 4), 4), ((8, 6, 4), 2), ((6, 5, 7), 1), ((16, 8, 4), 4)]
SYMBOLS = [0, 1]

SEED = {"efield": 21, "slab": 22, "fold": 23, "plane": 24, "elementwise": 25, "reduce": 26, "spectral": 27,
        "slab_spectral": 28}


def geom_id(g):
    T, off, nloc = g
    return "x".join(map(str, T)) + ("" if (off, nloc) == (0, T[-1]) else f"-off{off}-nloc{nloc}")


def shape_id(T):
    return "x".join(map(str, T))


def normals(shape, seed):
    """seeded standard normals of an array shape"""
    return np.random.default_rng(seed).standard_normal(tuple(shape))


def slab_shape(g, nv=None):
    T, off, nloc = g
    return (nloc + 2,) + tuple(T[:-1])[::-1] + (() if nv is None else (nv,))


def spectral_tolerance(ref64, refld):
    """The bound on a kernel's deviation from the long-double reference, from
    the references alone: d = max |fp64 numpy.fft - long double|, tolerance
    max(16 d, 64 eps max|ref|) (another FFT differs from numpy's by summation
    order: rounding of the same size), never above 1e-11 max|ref|."""
    d = float(np.max(np.abs(ref64 - refld)))
    top = float(np.max(np.abs(refld)))
    return d, min(max(16 * d, 64 * EPS * top), 1e-11 * top), top


_cache = {}


def spectral_reference(T, discrete, seed=None):
    """rho, the long-double solve, d, the tolerance and max|phi| of a case,
    computed once and read-only"""
    key = (tuple(T), discrete, seed)
    if key not in _cache:
        rho = normals(tuple(T)[::-1], SEED["spectral"] if seed is None else seed)
        hi = FR.poisson(rho, T, discrete, LD)
        d, tol, top = spectral_tolerance(FR.poisson_fft64(rho, T, discrete), hi)
        for a in (rho, hi):
            a.setflags(write=False)
        _cache[key] = (rho, hi, d, tol, top)
    return _cache[key]


def slab_block_reference(T, P, rank):
    """rho of SLAB_SPECTRAL's case (the whole domain), and for the rank: the
    long-double S, d of numpy's rfft2 against it, and the tolerance"""
    key = ("S", tuple(T), P, rank)
    if key not in _cache:
        rho = normals(tuple(T)[::-1], SEED["slab_spectral"])
        nloc = T[2] // P
        mine = rho[rank * nloc:(rank + 1) * nloc]
        hi = FR.slab_spectrum_blocks(mine, T, P, LD)
        d, tol, top = spectral_tolerance(FR.slab_spectrum_blocks(mine, T, P), hi)
        hi.setflags(write=False)
        _cache[key] = (hi, d, tol, top)
    return _cache[key]
