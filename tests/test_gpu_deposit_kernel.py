"""pinc_hip_deposit and pinc_hip_deposit_cells called directly (ctypes,
tests/push_abi.py) against the numpy reference tests/moments_ref.py: the
number moment, moments_reference(...).M[..., 0], is the charge of unit
particles.

Bound, per node (the moments tests' bound):

    |rho - rho_ref| <= (k + 8) eps sum|terms|,   exactly 0 where k = 0

Cases, the smallest at which each path exists.

pinc_hip_deposit (k_deposit_tiled):
  * the global path, a chunk whose cells' bounding box exceeds the 4096 LDS
    nodes (cells 0..T span T + 2 nodes per dimension): 16^3, 64 x 64 and one
    dimension of 4100, random order, species 1 of 2 at an odd iStart (the
    other species' slots hold SENTINEL);
  * the LDS path with partial blocks and an odd start: the cell-sorted 16 x 8
    x 8 population with the edge rows at start = 3, and the 2-D one;
  * one chunk plus one particle (n = 4097) on 8^3.  At an even iStart the
    second block has one live slot, the first of its pair; at an odd iStart
    the first pair of the first block has only its second slot live and the
    second block holds the last two particles.

pinc_hip_deposit_cells (k_deposit_cells), after pinc_hip_sort_tiles:
  * movers: a tenth of the sorted particles shifted by up to one cell, also
    across the periodic x and y faces (those land far outside the block's
    box: global atomics; the others inside its one-cell margin);
  * tile width 2 on 4^3: the one block of 216 keys spans 27 tiles of 8 cells,
    more than the 16 the kernel allows for its LDS box, so every add is
    global (any tile width with fewer than 16 cells per tile does this).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import moments_ref as MR
import push_ref as R
from moments_cases import case
from push_abi import DevSpecies, Geom, Pop, geom_of

pytestmark = pytest.mark.gpu

CHUNK = 4096     # particles per workgroup of k_deposit_tiled
LDS_NODES = 4096  # its LDS box


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available()
    from pinc_amd import _lib
    h = _lib.HIP
    vp = C.c_void_p
    h.pinc_hip_deposit.argtypes = [Pop, C.c_int, Geom, vp, vp]
    h.pinc_hip_sort_tiles.argtypes = [Pop, Pop, C.c_int, Geom, C.c_int, vp, C.c_long, C.POINTER(C.c_long), vp]
    h.pinc_hip_deposit_cells.argtypes = [Pop, C.c_int, Geom, C.c_int, vp, C.c_long, vp, vp]
    return h


def check_rho(rho, ref, what):
    """the bound above for a device charge rho (slab_shape); prints the worst
    error over the bound first"""
    assert rho.shape == ref.k.shape, (what, rho.shape, ref.k.shape)
    err = np.abs(rho.astype(MR.LD) - ref.M[..., 0])
    lim = (ref.k + 8) * MR.EPS * ref.A[..., 0]
    worst = float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1), 0), initial=0.0))
    print(f"{what}: charge error / bound {worst:.3f}")
    assert np.all(rho[ref.k == 0] == 0), what
    assert np.all(err <= lim), (what, worst)


def deposit(hip, sp, geom, s=0):
    import torch
    rho = torch.zeros(int(np.prod(R.slab_shape(geom))), dtype=torch.float64, device="cuda")
    assert hip.pinc_hip_deposit(sp.pop, s, geom_of(geom), rho.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return rho.cpu().numpy().reshape(R.slab_shape(geom))


@functools.lru_cache(maxsize=None)
def uniform_case(geom, n, seed):
    """(pos, vel, reference) of n uniformly random particles: made once,
    shared, never modified"""
    pos, vel = R.uniform_particles(geom, n, np.random.default_rng(seed), R.V_MAX)
    for a in (pos, vel):
        a.setflags(write=False)
    return pos, vel, MR.moments_reference(pos, vel, geom)


def box_nodes(pos):
    """nodes of the bounding box of the cells of pos (j .. j + 1 per dimension)"""
    cells = pos.astype(np.int64)
    return int(np.prod(cells.max(axis=0) - cells.min(axis=0) + 2))


@pytest.mark.parametrize("geom", [(16, 16, 16), (64, 64), (4100,)], ids=["16x16x16", "64x64", "4100"])
def test_global_path_second_species_odd_start(hip, geom):
    pos, vel, ref = uniform_case(geom, 5000, 21 + len(geom))
    start = 1001
    # the first workgroup's particles: slots [start - 1, start - 1 + CHUNK), the first one not live
    assert box_nodes(pos[:CHUNK - 1]) > LDS_NODES
    sp = DevSpecies(pos, vel, start=start, pad=7)
    # species 1 of 2: species 0 is [0, 1001), live, every slot SENTINEL
    sp.pop.nSpecies = 2
    sp.pop.iStart = (C.c_long * 9)(0, sp.start, sp.cap)
    sp.pop.iStop = (C.c_long * 8)(sp.start, sp.start + sp.n)
    check_rho(deposit(hip, sp, geom, s=1), ref, f"global path {geom}")
    assert sp.padding_untouched(sp.xs) and sp.padding_untouched(sp.vs)


@pytest.mark.parametrize("name", ["edge3d", "2d"])
def test_lds_path_partial_blocks_odd_start(hip, name):
    geom, pos, vel, ref = case(name)
    assert pos.shape[0] % CHUNK != 0
    sp = DevSpecies(pos, vel, start=3)
    check_rho(deposit(hip, sp, geom), ref, f"LDS path {name}")
    assert sp.padding_untouched(sp.xs)


@pytest.mark.parametrize("start", [0, 1, 2, 3])
def test_one_chunk_plus_one_particle(hip, start):
    geom = (8, 8, 8)
    pos, vel, ref = uniform_case(geom, CHUNK + 1, 31)
    assert box_nodes(pos) <= LDS_NODES
    sp = DevSpecies(pos, vel, start=start)
    check_rho(deposit(hip, sp, geom), ref, f"n = {CHUNK + 1}, iStart = {start}")
    assert sp.padding_untouched(sp.xs)


def sorted_on_device(hip, pos, geom, tw):
    """pinc_hip_sort_tiles of pos: (the sorted species, the work tensor, the
    address of the ranges' ends)"""
    import torch
    src = DevSpecies(pos, np.zeros_like(pos), pad=5, fill=0.0)
    out = DevSpecies(np.zeros_like(pos), np.zeros_like(pos), pad=5, fill=0.0)
    g = geom_of(geom)
    nk = C.c_long()
    assert hip.pinc_hip_sort_tiles(src.pop, out.pop, 0, g, tw, None, 0, C.byref(nk), None) != 0
    assert nk.value == R.tile_geo(geom, tw)[3]
    need = 2 * (nk.value + 1) + 2 * (nk.value // 4096 + 1) + 1
    work = torch.zeros(need, dtype=torch.int32, device="cuda")
    assert hip.pinc_hip_sort_tiles(src.pop, out.pop, 0, g, tw, work.data_ptr(), need, C.byref(nk), None) == 0
    torch.cuda.synchronize()
    return out, work, work.data_ptr() + 4 * (nk.value + 1)


def with_movers(pos, geom, rng):
    """a tenth of pos shifted by up to one cell per dimension; x and y wrap
    into [0.5, T + 0.5), the slab dimension is kept inside it"""
    nd = len(geom)
    pos = pos.copy()
    m = rng.random(pos.shape[0]) < 0.1
    pos[m] += rng.uniform(-1.0, 1.0, size=(int(m.sum()), nd))
    T = np.array(geom, dtype=np.float64)
    lo, up = 0.5, np.nextafter(T + 0.5, -np.inf)
    for d in range(nd - 1):
        pos[:, d] = np.where(pos[:, d] < lo, pos[:, d] + T[d], np.where(pos[:, d] > up[d], pos[:, d] - T[d], pos[:, d]))
    return np.clip(pos, lo, up), m


@pytest.mark.parametrize("geom,tw,n", [((16, 8, 8), 4, 20000), ((4, 4, 4), 2, 3000)], ids=["movers", "box-off"])
def test_deposit_cells_with_movers(hip, geom, tw, n):
    import torch
    pos0, _, _ = uniform_case(geom, n, 41 + tw)
    out, work, ends = sorted_on_device(hip, pos0, geom, tw)
    srt = out.live(out.xs)
    keys = R.cell_keys(srt.astype(np.int64), geom, tw)
    assert np.all(np.diff(keys) >= 0)
    if tw == 2:
        # the first workgroup's keys (256 at the most) span 16 or more tiles: no LDS box
        assert (min(256, R.tile_geo(geom, tw)[3]) - 1) // tw ** 3 >= 16
    pos, moved = with_movers(srt, geom, np.random.default_rng(51 + tw))
    cells0, cells = srt.astype(np.int64), pos.astype(np.int64)
    changed = np.any(cells != cells0, axis=1)
    far = np.any(np.abs(cells - cells0) > 1, axis=1)
    assert changed.sum() > n // 50 and far.sum() > 0 and not np.any(changed & ~moved)
    for d in range(3):
        out.xs[d][:n] = torch.from_numpy(np.ascontiguousarray(pos[:, d])).cuda()
    ref = MR.moments_reference(pos, np.zeros_like(pos), geom)
    rho = torch.zeros(int(np.prod(R.slab_shape(geom))), dtype=torch.float64, device="cuda")
    assert hip.pinc_hip_deposit_cells(out.pop, 0, geom_of(geom), tw, ends, n, rho.data_ptr(), None) == 0
    torch.cuda.synchronize()
    check_rho(rho.cpu().numpy().reshape(R.slab_shape(geom)), ref, f"deposit_cells {geom} tile width {tw}")
    del work   # (alive until here: the ranges' ends are in it)
