"""pinc_hip_moments called directly (ctypes, tests/push_abi.py) against the
numpy reference tests/moments_ref.py.

Bound, per node and moment (moments_ref.check):

    |M - M_ref| <= (k + 8) eps sum|terms|,   exactly 0 where k = 0

k roundings from the sum in any order, at most 8 from the fp64 weight, the
two velocity factors and the flush (the push test's charge bound, widened for
the extra products).

Cases, the smallest at which each path exists: a population in random order
on 8^3 (the chunk's cells overflow the LDS box: runs go to global memory;
species 1 of 2 at an odd iStart: unaligned first pair, partial last block,
the other species' slots hold SENTINEL); a cell-sorted one on 16x8x8 (the LDS
box, chunks that straddle tiles); particles in cells 0 and T of every
dimension (x/y wrap into storage, z lands on both ghost planes; before and
after the fold); geom.literal = 1 (ignored); the 2-D and 1-D instances;
velocity arrays other than pop.v; two calls into one slab; M[0] against
pinc_hip_deposit.
"""
import ctypes as C

import numpy as np
import pytest

import moments_ref as MR
import push_ref as R
from moments_cases import case
from push_abi import SENTINEL, DevSpecies, Geom, Pop, geom_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available()
    from pinc_amd import _lib
    h = _lib.HIP
    vp = C.c_void_p
    h.pinc_hip_moments.argtypes = [Pop, C.c_int, Geom, C.POINTER(vp), vp, vp]
    h.pinc_hip_deposit.argtypes = [Pop, C.c_int, Geom, vp, vp]
    h.pinc_hip_fold_self_values.argtypes = [vp, Geom, C.c_int, vp]
    return h


def slab_zeros(geom, nv):
    import torch
    return torch.zeros(int(np.prod(R.slab_shape(geom))) * nv, dtype=torch.float64, device="cuda")


def run(hip, sp, geom, *, s=0, vs=None, slab=None, literal=0):
    """one pinc_hip_moments of species s of sp.pop into slab (new, zero, if
    None); returns (host copy shaped slab_shape + (NM,), the device tensor)"""
    import torch
    nm = MR.n_moments(len(geom))
    if slab is None:
        slab = slab_zeros(geom, nm)
    g = geom_of(geom)
    g.literal = literal
    v = sp.ptrs(vs if vs is not None else sp.vs)
    assert hip.pinc_hip_moments(sp.pop, s, g, v, slab.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return slab.cpu().numpy().reshape(R.slab_shape(geom) + (nm,)), slab


def test_random_order_second_species_odd_start(hip):
    geom, pos, vel, ref = case("uniform3d")
    sp = DevSpecies(pos, vel, start=1001, pad=7)
    # species 1 of 2: species 0 is [0, 1001), live, every slot SENTINEL
    sp.pop.nSpecies = 2
    sp.pop.iStart = (C.c_long * 9)(0, sp.start, sp.cap)
    sp.pop.iStop = (C.c_long * 8)(sp.start, sp.start + sp.n)
    M, _ = run(hip, sp, geom, s=1)
    MR.check(M, ref, "random order, species 1")
    assert sp.padding_untouched(sp.xs) and sp.padding_untouched(sp.vs)


def test_cell_sorted(hip):
    geom, pos, vel, ref = case("sorted3d")
    M, _ = run(hip, DevSpecies(pos, vel), geom)
    MR.check(M, ref, "cell-sorted")


@pytest.mark.parametrize("name", ["edge3d", "2d", "1d"])
def test_edges_before_and_after_the_fold(hip, name):
    import torch
    geom, pos, vel, ref = case(name)
    nd = len(geom)
    # cells 0 and T of every dimension are there
    cells = pos.astype(np.int64)
    for d in range(nd):
        assert cells[:, d].min() == 0 and cells[:, d].max() == geom[d]
    assert ref.k[0].sum() > 0 and ref.k[geom[-1] + 1].sum() > 0   # both ghost planes
    M, slab = run(hip, DevSpecies(pos, vel, start=3), geom)
    MR.check(M, ref, f"{name} unfolded")
    assert hip.pinc_hip_fold_self_values(slab.data_ptr(), geom_of(geom), MR.n_moments(nd), None) == 0
    torch.cuda.synchronize()
    F = slab.cpu().numpy().reshape(M.shape)[1:geom[-1] + 1]
    MR.check(F, MR.folded(ref, geom[-1]), f"{name} folded")


def test_literal_is_ignored(hip):
    geom, pos, vel, ref = case("edge3d")
    sp = DevSpecies(pos, vel)
    M1, _ = run(hip, sp, geom, literal=1)
    MR.check(M1, ref, "literal = 1")
    M2, _ = run(hip, sp, geom, literal=2)
    MR.check(M2, ref, "literal = 2")


def test_reads_the_velocity_arrays_it_is_given(hip):
    geom, pos, vel, ref = case("edge3d")
    sp = DevSpecies(pos, np.full_like(vel, SENTINEL), start=5)
    other = DevSpecies(pos, vel, start=5)      # same ranges: indexed like pop.v
    M, _ = run(hip, sp, geom, vs=other.vs)
    MR.check(M, ref, "separate velocity arrays")
    assert np.all(sp.live(sp.vs) == SENTINEL)


def test_accumulates(hip):
    geom, pos, vel, ref = case("edge3d")
    g2, p2, v2, ref2 = case("sorted3d")
    assert g2 == geom
    _, slab = run(hip, DevSpecies(pos, vel), geom)
    M, _ = run(hip, DevSpecies(p2, v2, start=1), geom, slab=slab)
    MR.check(M, MR.add(ref, ref2), "two calls into one slab")


@pytest.mark.parametrize("name", ["uniform3d", "edge3d", "2d", "1d"])
def test_number_matches_the_deposit(hip, name):
    """M[0] and pinc_hip_deposit on the same particles: each within the bound
    of the reference, so within twice the bound of each other"""
    import torch
    geom, pos, vel, ref = case(name)
    sp = DevSpecies(pos, vel)
    M, _ = run(hip, sp, geom)
    rho = slab_zeros(geom, 1)
    assert hip.pinc_hip_deposit(sp.pop, 0, geom_of(geom), rho.data_ptr(), None) == 0
    torch.cuda.synchronize()
    rho = rho.cpu().numpy().reshape(R.slab_shape(geom))
    lim = ((ref.k + 8) * MR.EPS * ref.A[..., 0]).astype(np.float64)
    e_dep = np.abs(rho - ref.M[..., 0])
    e_mom = np.abs(M[..., 0] - ref.M[..., 0])
    both = np.abs(M[..., 0] - rho)
    print(f"{name}: deposit {float(np.max(e_dep / np.where(lim > 0, lim, 1))):.3f}, "
          f"moments {float(np.max(e_mom / np.where(lim > 0, lim, 1))):.3f} of the bound")
    assert np.all(e_dep <= lim) and np.all(e_mom <= lim) and np.all(both <= 2 * lim)
    assert np.all(rho[ref.k == 0] == 0) and np.all(M[ref.k == 0] == 0)


def test_rejects_bad_arguments(hip):
    geom, pos, vel, _ = case("1d")
    sp = DevSpecies(pos, vel)
    slab = slab_zeros(geom, 3)
    hip.pinc_hip_error_string.restype = C.c_char_p
    assert hip.pinc_hip_moments(sp.pop, 0, geom_of(geom), None, slab.data_ptr(), None) != 0
    assert b"moments" in hip.pinc_hip_error_string()
    assert hip.pinc_hip_moments(sp.pop, 9, geom_of(geom), sp.ptrs(sp.vs), slab.data_ptr(), None) != 0
