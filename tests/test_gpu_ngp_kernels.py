"""pinc_hip_deposit_ngp and pinc_hip_accelerate_ngp (order 0: the nearest
node (int)(x + 0.5)) called through the C ABI, against tests/glue_ref.py.

Grids: 1-D T = 8, 2-D 8 x 6, 3-D 8 x 6 with nloc = 5, and a 3-D slab of
nloc = 5 planes of T[2] = 10 at offset 5; literal 0, 1 and 2.  Species 1 of 2
at an odd iStart, 2 * 2048 + 37 particles uniform in [0, T + 1) per dimension
with planted coordinates: integers, k + 0.5 exactly (node k + 1; rounding
half to even would give k), its lower neighbour, 0.0, and the lower neighbour
of T + 1.5 (node T + 1: storage 0 of a periodic dimension, ghost plane
nloc + 1 of the slab dimension).

Deposit: rho starts as integers, and every particle adds 1 times a literal
factor from {0, 1, 2, 3, 4, 6}: all sums are integers far below 2^53, exact
in fp64 in any order, so the comparison is bit for bit whatever order the
atomics take.  A 1-D species of 65536 * 256 + 3 particles crosses the launch
cap of 65536 blocks (the grid stride).

Acceleration: v' = v + E[node] bit for bit (one add), positions untouched,
nBlocks = ceil(n / 2048), and each kePartial[b] within

    (2048 + 4) eps sum |v (v + dv)|

of the long-double sum over block b's own 2048 particles: per particle at
most 4 roundings (the add, the product, two additions over the dimensions),
then fewer than 2048 additions whatever tree the block uses.  The bound is
far below what a block owning other particles would give
(tests/test_glue_ref_cpu.py).  kePartial behind nBlocks is untouched.
"""
import ctypes as C

import numpy as np
import pytest

import glue_ref as G
from gpu_buf import Buf, same_bits
from push_abi import Geom, Pop

pytestmark = pytest.mark.gpu

LD = G.LD


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available()
    from pinc_amd import _lib
    h = _lib.HIP
    vp = C.c_void_p
    h.pinc_hip_deposit_ngp.argtypes = [Pop, C.c_int, Geom, vp, vp]
    h.pinc_hip_accelerate_ngp.argtypes = [Pop, C.c_int, Geom, vp, vp, C.POINTER(C.c_int), vp]
    return h


def geom(name, literal=0):
    T, nloc, off, nranks = G.NGP_GEOMS[name]
    return Geom(len(T), (C.c_int * 3)(*(list(T) + [1] * (3 - len(T)))), nloc, off, nranks, literal)


@pytest.mark.parametrize("literal", [0, 1, 2])
@pytest.mark.parametrize("name", list(G.NGP_GEOMS))
def test_deposit(hip, name, literal):
    """bit for bit: integer sums"""
    Tl = G.ngp_local(name)
    pos = G.ngp_particles(name)
    sp = G.species_1_of_2(pos, np.zeros_like(pos))
    rho0 = G.ngp_rho0(Tl)
    rho = Buf(rho0)
    assert hip.pinc_hip_deposit_ngp(sp.pop, 1, geom(name, literal), rho.ptr, None) == 0
    want = G.ngp_deposit(pos, Tl, literal, rho0)
    got = rho.get()
    np.testing.assert_array_equal(got, want)
    assert same_bits(got, want)
    np.testing.assert_array_equal(sp.live(sp.xs), pos)
    assert sp.padding_untouched(sp.xs) and sp.padding_untouched(sp.vs)


def test_deposit_past_the_block_cap(hip):
    """65536 * 256 + 3 particles in 1-D: more than the cap of 65536 blocks of
    256 threads covers at one particle each"""
    import torch
    from push_abi import SENTINEL
    T, n, start = G.NGP_BIG_T, G.NGP_BIG_N, G.START
    pos = np.random.default_rng(43).random(n) * (T + 1)
    pos[-3:] = [T + 0.5, 0.5, np.nextafter(T + 1.5, 0.0)]        # the stride's last particles
    x = torch.full((start + n + 7,), SENTINEL, dtype=torch.float64, device="cuda")
    x[start:start + n] = torch.from_numpy(pos).cuda()
    pop = Pop((C.c_void_p * 3)(x.data_ptr(), None, None), (C.c_void_p * 3)(), 2, 1, (C.c_long * 9)(0, start, start + n + 7),
              (C.c_long * 8)(start, start + n))
    rho0 = G.ngp_rho0((T,))
    rho = Buf(rho0)
    g = Geom(1, (C.c_int * 3)(T, 1, 1), T, 0, 1, 0)
    assert hip.pinc_hip_deposit_ngp(pop, 1, g, rho.ptr, None) == 0
    got = rho.get()
    want = rho0 + np.bincount(G.nearest(pos), minlength=T + 2)
    assert int(want.sum() - rho0.sum()) == n
    np.testing.assert_array_equal(got, want)
    assert same_bits(got, want)
    assert bool((x[:start] == SENTINEL).all()) and bool((x[start + n:] == SENTINEL).all())


def test_deposit_of_no_particles(hip):
    Tl = G.ngp_local("3d")
    pos = G.ngp_particles("3d")
    sp = G.species_1_of_2(pos, np.zeros_like(pos))
    sp.pop.iStop[1] = sp.pop.iStart[1]
    rho = Buf(G.ngp_rho0(Tl))
    assert hip.pinc_hip_deposit_ngp(sp.pop, 1, geom("3d"), rho.ptr, None) == 0
    assert rho.unchanged()


@pytest.mark.parametrize("name", list(G.NGP_GEOMS))
def test_accelerate(hip, name):
    """v' bit for bit; kePartial[b] within (2048 + 4) eps sum|v (v + dv)| of
    block b's own long-double sum (measured on an MI355X: at most 0.0004 of
    the bound)"""
    Tl = G.ngp_local(name)
    pos = G.ngp_particles(name)
    vel = np.random.default_rng(3).uniform(-0.6, 0.6, size=pos.shape)
    Es = G.ngp_field(Tl)
    v1, ke_ref, mag = G.ngp_accelerate(pos, vel, Es, Tl)
    sp = G.species_1_of_2(pos, vel)
    E = Buf(Es)
    nblk = -(-G.N_PART // G.CHUNK)
    ke = Buf(np.full(nblk + 5, -1.0))
    nb = C.c_int(-1)
    assert hip.pinc_hip_accelerate_ngp(sp.pop, 1, geom(name), E.ptr, ke.ptr, C.byref(nb), None) == 0
    got = ke.get()
    assert nb.value == nblk == 3
    v = sp.live(sp.vs)
    np.testing.assert_array_equal(v, v1)
    assert same_bits(v, v1)
    np.testing.assert_array_equal(sp.live(sp.xs), pos)
    assert sp.padding_untouched(sp.xs) and sp.padding_untouched(sp.vs)
    assert E.unchanged()
    assert np.all(got[nblk:] == -1.0)
    err = np.abs(got[:nblk].astype(LD) - ke_ref)
    lim = (G.CHUNK + 4) * G.EPS * mag
    print(f"{name}: KE partial error / bound {float(np.max(err / lim)):.4f}")
    assert np.all(err <= lim)


def test_accelerate_of_no_particles(hip):
    Tl = G.ngp_local("2d")
    pos = G.ngp_particles("2d")
    vel = np.full_like(pos, 0.25)
    sp = G.species_1_of_2(pos, vel)
    sp.pop.iStop[1] = sp.pop.iStart[1]
    E, ke = Buf(G.ngp_field(Tl)), Buf(np.full(4, -1.0))
    nb = C.c_int(-1)
    assert hip.pinc_hip_accelerate_ngp(sp.pop, 1, geom("2d"), E.ptr, ke.ptr, C.byref(nb), None) == 0
    assert nb.value == 0
    assert ke.unchanged()
    np.testing.assert_array_equal(sp.live(sp.vs), vel)
