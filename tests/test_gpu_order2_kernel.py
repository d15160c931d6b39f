"""pinc_hip_deposit_tsc and pinc_hip_accelerate_tsc called directly (ctypes:
pinc_amd._lib's prototypes, the device species of tests/push_abi.py) against
the restatement tests/order2_ref.py.

Grids: 1-D T = 8, 2-D 8 x 6, 3-D 8 x 6 with nloc = 5, and 3-D 20 x 20 with
nloc = 12, whose padded volume 22 * 22 * 14 = 6776 exceeds the deposit's 4096
LDS nodes.  Particles: species 1 of 2 at an odd iStart, 4096 + 37 of them (a
full chunk and a partial one): the planted edge values of order2_ref.planted
(0.5, nextafter(T + 0.5, 0), T + 0.5 itself, integers, half-integers and both
neighbours of a half-integer, per dimension), the rest uniform in
[0.5, T + 0.5); in random order and sorted by nearest node.  Which path a
chunk takes follows from its nearest nodes' bounding box and is asserted: on
the three small grids every chunk fits the LDS box; on 20 x 20 x 12 the full
chunk does not (in either order: 4095 of 4133 particles span the grid) and
goes through global atomics, the partial chunk of the sorted order (one
z-plane of nodes) fits.

Deposit, per slab node, k the terms that are not zero:

    |rho - ref| <= (k + 8) eps sum|terms|,   exactly 0 where k = 0

The 8: at most 2 roundings per one-dimensional weight, three weights and two
multiplications per node weight (6 + 2), then k - 1 additions (and one
multiplication by the literal factor, a power of two or 3, 7: exact or one
more rounding, inside the k + 8 since k - 1 < k).

Acceleration, per component: |v' - ref| <= (27 + 8) eps sum|w E| + eps |v'|
(27 terms at the most, each w E one more rounding, the final v + dv the last
term), sum(kePartial) within 1e-12 relative of the long double sum (the
project's acceleration bound); positions untouched.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import order2_ref as O
import push_ref as R
from push_abi import DevSpecies, geom_of

pytestmark = pytest.mark.gpu

CHUNK = 4096      # particles per workgroup of k_deposit_tsc
LDS_NODES = 4096  # its LDS box
N = CHUNK + 37
START = 1001
GEOMS = {"1d": (8,), "2d": (8, 6), "3d": (8, 6, 5), "3d-big": (20, 20, 12)}
EPS = O.EPS


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available()
    from pinc_amd import _lib
    return _lib.HIP


def lib_pop(pop):
    """a push_abi.Pop as the pinc_pop_t of pinc_amd._lib's prototypes (the same layout)"""
    from pinc_amd import _lib
    return _lib.HipPop.from_buffer_copy(pop)


def lib_geom(T, literal=0, nd=None):
    from pinc_amd import _lib
    g = _lib.HipGeom.from_buffer_copy(geom_of(T))
    g.literal = literal
    if nd is not None:
        g.nd = nd
    return g


@functools.lru_cache(maxsize=None)
def positions(name, order):
    T = GEOMS[name]
    pos = O.particles(T, N, 100 + len(name))
    if order == "random":
        pos = pos[np.random.default_rng(7).permutation(N)]
    else:
        pos = O.node_sorted(pos, T)
    pos.setflags(write=False)
    return pos


@functools.lru_cache(maxsize=None)
def deposit_ref(name, order, literal):
    T = GEOMS[name]
    return O.slab(O.deposit(positions(name, order), T, literal), T)


def chunk_fits(pos, T):
    """per workgroup of species [START, START + N): its nearest nodes'
    bounding box, one node wider on each side, fits the LDS box"""
    j, _ = O.split(pos, T)
    first = START & ~1
    out = []
    for c0 in range(first, START + N, CHUNK):
        jj = j[max(c0 - START, 0):c0 - START + CHUNK]
        out.append(int(np.prod(jj.max(axis=0) - jj.min(axis=0) + 3)) <= LDS_NODES)
    return out


def species_1_of_2(pos, vel):
    sp = DevSpecies(pos, vel, start=START, pad=7)
    sp.pop.nSpecies = 2
    sp.pop.iStart = (C.c_long * 9)(0, sp.start, sp.cap)
    sp.pop.iStop = (C.c_long * 8)(sp.start, sp.start + sp.n)
    return sp


def check_rho(rho, ref, calls, what):
    err = np.abs(rho.astype(O.LD) - calls * ref.M)
    lim = (calls * ref.k + 8) * EPS * (calls * ref.A)
    worst = float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1), 0), initial=0.0))
    print(f"{what}: charge error / bound {worst:.3f}")
    assert np.all(rho[ref.k == 0] == 0), what
    assert np.all(err <= lim), (what, worst)


@pytest.mark.parametrize("order", ["random", "sorted"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_deposit(hip, name, order):
    import torch
    T = GEOMS[name]
    pos = positions(name, order)
    fits = chunk_fits(pos, T)
    assert len(fits) == 2
    if name == "3d-big":
        assert fits == ([False, False] if order == "random" else [False, True])
    else:
        assert fits == [True, True]
    sp = species_1_of_2(pos, np.zeros_like(pos))
    shape = R.slab_shape(T)
    for literal in (0, 1, 2):
        g = lib_geom(T, literal)
        ref = deposit_ref(name, order, literal)
        rho = torch.zeros(int(np.prod(shape)), dtype=torch.float64, device="cuda")
        for calls in (1, 2):   # the second call accumulates
            assert hip.pinc_hip_deposit_tsc(lib_pop(sp.pop), 1, g, rho.data_ptr(), None) == 0
            torch.cuda.synchronize()
            check_rho(rho.cpu().numpy().reshape(shape), ref, calls, f"{name} {order} literal {literal} call {calls}")
    assert sp.padding_untouched(sp.xs)


@pytest.mark.parametrize("order", ["random", "sorted"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_accelerate(hip, name, order):
    import torch
    T = GEOMS[name]
    nd = len(T)
    pos = positions(name, order)
    rng = np.random.default_rng(3)
    vel = rng.uniform(-0.6, 0.6, size=pos.shape)
    Es = rng.uniform(-R.E_MAX, R.E_MAX, size=R.slab_shape(T) + (nd,))   # every node, ghost planes included
    dv, mag = O.gather(pos, Es, T)
    v_ref = vel.astype(O.LD) + dv
    sp = species_1_of_2(pos, vel)
    dE = torch.from_numpy(Es).cuda()
    ke = torch.full((64,), -1.0, dtype=torch.float64, device="cuda")
    nb = C.c_int(-1)
    assert hip.pinc_hip_accelerate_tsc(lib_pop(sp.pop), 1, lib_geom(T), dE.data_ptr(), ke.data_ptr(), C.byref(nb), None) == 0
    torch.cuda.synchronize()
    assert nb.value == -(-N // 2048)
    v = sp.live(sp.vs)
    err = np.abs(v.astype(O.LD) - v_ref)
    lim = (27 + 8) * EPS * mag + EPS * np.abs(v)
    print(f"{name} {order}: velocity error / bound {float(np.max(err / lim)):.3f}")
    assert np.all(err <= lim)
    terms = vel.astype(O.LD) * v_ref
    ke_ref = terms.sum()
    ke_dev = ke.cpu().numpy()
    assert np.all(ke_dev[nb.value:] == -1.0)
    rel = abs(float((ke_dev[:nb.value].astype(O.LD).sum() - ke_ref) / ke_ref))
    print(f"{name} {order}: kinetic energy relative error {rel:.3e}")
    assert rel <= 1e-12
    np.testing.assert_array_equal(sp.live(sp.xs), pos)
    assert sp.padding_untouched(sp.xs) and sp.padding_untouched(sp.vs)


def test_bad_arguments_launch_nothing(hip):
    import torch
    T = GEOMS["2d"]
    pos = positions("2d", "random")
    vel = np.full_like(pos, 0.25)
    sp = species_1_of_2(pos, vel)
    rho = torch.zeros(int(np.prod(R.slab_shape(T))), dtype=torch.float64, device="cuda")
    Es = torch.ones(rho.numel() * 2, dtype=torch.float64, device="cuda")
    ke = torch.zeros(64, dtype=torch.float64, device="cuda")
    nb = C.c_int(0)
    for nd, s in ((0, 1), (4, 1), (2, -1), (2, 2), (2, 8)):
        g = lib_geom(T, nd=nd)
        assert hip.pinc_hip_deposit_tsc(lib_pop(sp.pop), s, g, rho.data_ptr(), None) != 0, (nd, s)
        assert hip.pinc_hip_accelerate_tsc(lib_pop(sp.pop), s, g, Es.data_ptr(), ke.data_ptr(), C.byref(nb), None) != 0, (nd, s)
        assert nb.value == 0
    torch.cuda.synchronize()
    assert float(rho.abs().sum()) == 0.0
    np.testing.assert_array_equal(sp.live(sp.vs), vel)
    assert hip.pinc_hip_error_string()
