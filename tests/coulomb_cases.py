"""The cases of tests/test_gpu_coulomb_kernel.py, kept apart from it so that the
CPU suite (test_coulomb_ref_cpu.py::test_reference_margins) can hold every one
of them to its decision margins without a GPU.

A case is (T, species a, species b, launches): positions and velocities (n, 3)
of the two species of a population (b may be empty) on a grid of T true cells,
and the launches (a, b, Params, key) applied to it in turn.  The shapes are the
smallest at which each path of the kernel exists; `cap` is the library's
pinc_hip_coulomb_cell_cap().
"""
import functools

import numpy as np

import coulomb_ref as R

T = (4, 3, 2)
NC = T[0] * T[1] * T[2]
ELECTRON_ION = dict(fa=1836.0 / 1837.0, fb=1.0 / 1837.0)


def _cell_pos(rng, cell, n):
    c = np.array([cell % T[0], (cell // T[0]) % T[1], cell // (T[0] * T[1])])
    return 1.0 + c + rng.random((n, 3))


def populate(rng, occupancy, vth=0.2):
    """particles with occupancy[c] members in cell c, in shuffled index order"""
    pos = np.concatenate([_cell_pos(rng, c, n) for c, n in enumerate(occupancy)] + [np.zeros((0, 3))])
    p = rng.permutation(len(pos))
    return pos[p], vth * rng.standard_normal((len(pos), 3))


def _pad(occ):
    return list(occ) + [0] * (NC - len(occ))


def _empty():
    return np.zeros((0, 3)), np.zeros((0, 3))


def build(name, cap):
    """(species a, species b, launches) of a case"""
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name))
    rng = np.random.default_rng(seed)
    k = lambda step, a, b: R.key(seed, step, 0, a, b)
    like = lambda K, step=0, **kw: [(0, 0, R.Params(K=K, **kw), k(step, 0, 0))]
    if name == "occupancy":
        occ = [0, 1, 2, 3, 4, 5, 63, 64, 65, cap - 1, cap, cap + 1] + [6 + c for c in range(NC - 12)]
        return populate(rng, occ), _empty(), like(2e-5)
    if name == "one cell":
        return populate(rng, _pad([0] * 7 + [2 * cap + 45])), _empty(), like(1e-6)
    if name == "isotropic":
        return populate(rng, [5 + (c % 4) for c in range(NC)]), _empty(), like(1e3)
    if name == "K0":
        return populate(rng, [8] * NC), _empty(), like(0.0)
    if name == "h":
        return populate(rng, [7 + (c % 3) for c in range(NC)]), _empty(), like(2e-4, h=(1.0, 2.0, 0.5))
    if name == "faces":
        # on cell faces (integer coordinates) and outside the true cells, where the cell is clamped
        pos, vel = populate(rng, [4] * NC)
        pos[0::3, 0] = np.floor(pos[0::3, 0])
        pos[1::3, 1] = np.floor(pos[1::3, 1])
        pos[2::5, 2] = np.floor(pos[2::5, 2])
        pos[0:6, 0] = [0.25, 0.999, -0.5, T[0] + 1.0, T[0] + 1.75, T[0] + 3.0]
        pos[6:10, 2] = [0.0, 0.5, T[2] + 1.0, T[2] + 1.5]
        return (pos, vel), _empty(), like(1e-4)
    if name == "aligned":
        # cell 0: a pair that differs in vz alone (g_perp == 0), both signs of gz over the launches'
        # orders; cell 1: two equal velocities (g == 0: no collision); cell 2: a triple with them
        pos, vel = populate(rng, _pad([2, 2, 3, 6, 4]))
        c = R.cells(pos, T)
        i0, i1, i2 = (np.flatnonzero(c == q) for q in range(3))
        vel[i0[1], :2] = vel[i0[0], :2]
        vel[i1[1]] = vel[i1[0]]
        vel[i2[1]] = vel[i2[0]]
        vel[i2[2], :2] = vel[i2[0], :2]
        return (pos, vel), _empty(), like(1e-4) + like(1e-4, step=1) + like(1e-4, step=2)
    if name == "five":
        return populate(rng, [3 + (c % 5) for c in range(NC)]), _empty(), sum((like(3e-4, step=s) for s in range(5)), [])
    if name == "two keys":
        return populate(rng, [9] * NC), _empty(), like(2e-4) + like(2e-4, step=1)
    if name == "second species":
        # the like pair (1, 1): species 0 is there and must stay as it is
        return populate(rng, [3] * NC), populate(rng, [5 + (c % 4) for c in range(NC)]), \
            [(1, 1, R.Params(K=2e-4), k(0, 1, 1))]
    # ---- unlike pairs: occupancies (species a, species b) per cell
    ua = _pad([5, 7, 3, 4, 0, cap + 3, cap + 2, 1, 2, cap, 6, 64])
    ub = _pad([1, 3, 7, 0, 4, 10, cap + 5, 1, 2, cap + 1, 6, 65])
    if name in ("unlike", "unlike equal mass", "like then unlike"):
        sa, sb = populate(rng, ua), populate(rng, ub, vth=0.02)
        if name == "unlike":
            return sa, sb, [(0, 1, R.Params(K=1e-5, **ELECTRON_ION), k(0, 0, 1))]
        if name == "unlike equal mass":
            return sa, sb, [(0, 1, R.Params(K=1e-5), k(0, 0, 1))]
        return sa, sb, [(0, 0, R.Params(K=2e-5), k(0, 0, 0)), (0, 1, R.Params(K=1e-5, **ELECTRON_ION), k(0, 0, 1)),
                        (1, 1, R.Params(K=1e-9), k(0, 1, 1))]
    if name == "unlike equal lengths":
        return populate(rng, [5] * NC), populate(rng, [5] * NC), [(0, 1, R.Params(K=1e-4, fa=0.75, fb=0.25), k(0, 0, 1))]
    if name == "unlike isotropic":
        return populate(rng, [6] * NC), populate(rng, [4] * NC), [(0, 1, R.Params(K=1e3, **ELECTRON_ION), k(0, 0, 1))]
    if name == "unlike empty b":
        return populate(rng, [6] * NC), _empty(), [(0, 1, R.Params(K=1e-4), k(0, 0, 1))]
    raise KeyError(name)


NAMES = ["occupancy", "one cell", "isotropic", "K0", "h", "faces", "aligned", "five", "two keys", "second species",
         "unlike", "unlike equal mass", "like then unlike", "unlike equal lengths", "unlike isotropic", "unlike empty b"]


def freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(name, cap):
    """(species a, species b, launches, the reference's Result of every launch
    -- each from the state the one before left): made once, shared, never
    modified"""
    (pa, va), (pb, vb), launches = build(name, cap)
    freeze(pa, va, pb, vb)
    state = [va, vb]
    results = []
    for a, b, par, key in launches:
        res = reference((pa, pb), state, a, b, par, key)
        results.append(res)
        state = advance(state, a, b, res)
    return (pa, va), (pb, vb), launches, results


def reference(pos, vel, a, b, par, key, err0=None):
    """the restatement's launch (a, b) on the population (pos, vel: per species);
    err0: per species, coulomb_ref.coulomb's input errors"""
    if a == b:
        return R.coulomb(pos[a], vel[a], None, None, par, key, T, None if err0 is None else [err0[a], None])
    return R.coulomb(pos[a], vel[a], pos[b], vel[b], par, key, T, None if err0 is None else [err0[a], err0[b]])


def advance(vel, a, b, res):
    """the velocities after a launch, rounded to float64 (the chain of references)"""
    out = list(vel)
    out[a] = np.asarray(res.vel[0], dtype=np.float64)
    if b != a:
        out[b] = np.asarray(res.vel[1], dtype=np.float64)
    return out
