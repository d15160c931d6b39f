"""The fused push kernel (k_push, through pinc_hip_push) called directly
against the numpy reference of tests/push_ref.py.  All 16 instantiations
that pinc_hip_push dispatches to are run: 3-D x kick x sort x objects, 2-D
and 1-D x kick x sort.

Every case (plain_case, sorting_case, the counting push) checks: x' and the
flags exactly (the reference's float64 kick is the kernels' expression
order), chunkCount, *nBlocks, errFlag, emigTotal and moved exactly, the
padding and the inputs untouched, the same flags and chunkCount from a
second run with flagsSparse = 1 over a pre-centred flag array, and

  |v' - v'_ref|   <= 32 eps max|Es|            per component,
  |rho - rho_ref| <= (k + 4) eps rho_ref       per node (k contributions;
                                                exactly 0 where k = 0),
  |KE - KE_ref|   <= 1e-12 sum|terms|.

A plain push without objects is also compared bit for bit (x', v', flags,
chunkCount) with pinc_hip_accelerate + pinc_hip_move_classify, which have no
object test; a sorting push row by row with the plain push of its input.

With the slab dimension wrapped in place (wrapMask bit nd-1) a block that
straddles that boundary deposits at the periodic images of its cells, so
ghost plane 0 and true plane nloc (nloc + 1 and 1) hold one node's charge
between them until the halo fold; the charge is compared after that fold
(plane 0 into nloc, plane nloc + 1 into 1), applied to both sides.

Instantiations and paths per case are listed at each test.
"""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest

import push_ref as R
from push_abi import SENTINEL, DevSpecies, Geom, Pop, PushArgs, geom_of

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TW = 4
FLAG_FILL = 99


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available()
    from pinc_amd import _lib
    h = _lib.HIP
    vp = C.c_void_p
    h.pinc_hip_push.argtypes = [Pop, C.c_int, Geom, C.POINTER(PushArgs), C.POINTER(C.c_int), vp]
    h.pinc_hip_accelerate.argtypes = [Pop, C.c_int, Geom, vp, vp, C.POINTER(C.c_int), vp]
    h.pinc_hip_move_classify.argtypes = [Pop, C.c_int, C.c_int, vp, vp, vp, C.c_double, vp, C.c_int, vp]
    h.pinc_hip_sort_tiles.argtypes = [Pop, Pop, C.c_int, Geom, C.c_int, vp, C.c_long, C.POINTER(C.c_long), vp]
    h.pinc_hip_tile_keys.argtypes = [Geom, C.c_int]
    h.pinc_hip_tile_keys.restype = C.c_long
    h.pinc_hip_count_keys.argtypes = [Pop, C.c_int, C.c_long, Geom, C.c_int, vp, vp]
    h.pinc_hip_scan_keys.argtypes = [vp, C.c_long, vp, vp, vp]
    h.pinc_hip_push_chunk.restype = C.c_long
    return h


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _thr_c(geom):
    return (C.c_double * 9)(*R.thresholds(geom))


def run_push(hip, sp, geom, *, kick, Es=None, wrap, out=None, cursor=None, cnt_next=None, sparse=0, obj=None):
    """One pinc_hip_push of species sp (DevSpecies) into `out` (a DevSpecies
    with the same ranges; None: in place).  Returns the host copies."""
    import torch
    n, nd = sp.n, sp.nd
    out = out or sp
    chunk = hip.pinc_hip_push_chunk()
    nblk = (n + chunk - 1) // chunk
    nch = (n + R.PINC_CHUNK - 1) // R.PINC_CHUNK
    i32 = lambda m: torch.zeros(m, dtype=torch.int32, device="cuda")
    u64 = lambda m: torch.zeros(m, dtype=torch.int64, device="cuda")
    rho = torch.zeros(int(np.prod(R.slab_shape(geom))), dtype=torch.float64, device="cuda")
    fl = np.full(sp.cap, FLAG_FILL, dtype=np.uint8)
    if sparse:
        fl[sp.start:sp.start + n] = R.centre(nd)
    flags = _dev(fl)
    cnt, err, emig, moved = i32(nch + 2), i32(1), u64(1), u64(1)
    ke = torch.full((nblk + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    dg = u64(8)
    thr = _thr_c(geom)
    a = PushArgs()
    a.xout, a.vout = out.ptrs(out.xs), out.ptrs(out.vs)
    a.kick = int(kick)
    Et = _dev(Es.ravel()) if kick else None
    a.Es = Et.data_ptr() if kick else None
    a.rhoS = rho.data_ptr()
    a.thr = C.cast(thr, C.c_void_p)
    a.flags = flags.data_ptr()
    a.chunkCount = cnt.data_ptr()
    a.maxVel = 1.0
    a.errFlag = err.data_ptr()
    a.wrapMask = wrap
    a.kePartial = ke.data_ptr()
    a.tileWidth = TW
    a.cursor = cursor.data_ptr() if cursor is not None else None
    a.cntNext = cnt_next.data_ptr() if cnt_next is not None else None
    a.moved = moved.data_ptr()
    a.emigTotal = emig.data_ptr()
    a.flagsSparse = sparse
    a.diag = dg.data_ptr()
    keep = []
    if obj is not None:
        ins = _dev(obj["inside"].ravel())
        oc = i32(obj["n"] + 1)
        keep += [ins, oc]
        tz, ty, tx = obj["inside"].shape
        a.objInside, a.objSy, a.objSz, a.objNodes = ins.data_ptr(), tx, tx * ty, tx * ty * tz
        a.objCount = oc.data_ptr()
        a.objLo, a.objHi = (C.c_int * 3)(*obj["lo"]), (C.c_int * 3)(*obj["hi"])
    nb = C.c_int(-1)
    assert hip.pinc_hip_push(sp.pop, 0, geom_of(geom), C.byref(a), C.byref(nb), None) == 0
    torch.cuda.synchronize()
    kep = ke.cpu().numpy()
    assert np.all(kep[nblk:] == SENTINEL)
    f = flags.cpu().numpy()
    assert np.all(f[:sp.start] == FLAG_FILL) and np.all(f[sp.start + n:] == FLAG_FILL)
    c = cnt.cpu().numpy()
    assert np.all(c[nch:] == 0)
    return SimpleNamespace(
        x=out.live(out.xs), v=out.live(out.vs), flag=f[sp.start:sp.start + n], chunk=c[:nch], nb=nb.value,
        nblk=nblk, err=int(err[0]), emig=int(emig[0]), moved=int(moved[0]),
        ke=math.fsum(kep[:nblk]) if kick else 0.0, rho=rho.cpu().numpy().reshape(R.slab_shape(geom)),
        diag=dg.cpu().numpy(), obj_count=oc.cpu().numpy() if obj is not None else None)


def _fold(a, geom):
    nloc = geom[-1]
    a = a.copy()
    a[nloc] += a[0]
    a[1] += a[nloc + 1]
    a[0] = 0
    a[nloc + 1] = 0
    return a


def check_charge(rho, r, geom, wrap):
    ref, k = r.rho, r.contrib
    if (wrap >> (len(geom) - 1)) & 1:
        rho, ref, k = _fold(rho, geom), _fold(ref, geom), _fold(k, geom)
    err = np.abs(rho - ref)
    lim = (k + 4) * EPS * ref
    worst = float(np.max(np.where(k > 0, err / np.where(k > 0, lim, 1), 0)))
    print(f"charge error / bound {worst:.3f}")
    assert np.all(err <= lim), worst
    assert np.all(rho[k == 0] == 0)


def check_sums(g, r, kick):
    """velocity-independent scalars, charge excluded"""
    assert g.err == 0
    assert g.nb == g.nblk
    assert g.emig == r.emig_total
    assert g.moved == r.moved
    if kick:
        print(f"KE error / bound {abs(float(g.ke - r.ke)) / (1e-12 * float(r.ke_abs)):.3g}")
        assert abs(float(g.ke - r.ke)) <= 1e-12 * float(r.ke_abs)


def check_particles(g, r, vel, Es, kick):
    assert np.array_equal(g.x, r.x)
    assert np.array_equal(g.flag, r.flag)
    assert np.array_equal(g.chunk, r.chunk_emig)
    if kick:
        emax = np.abs(Es).max()
        print(f"velocity error {float(np.abs(g.v - r.v).max() / (EPS * (emax or 1.0))):.2f} eps max|Es|")
        assert np.all(np.abs(g.v - r.v) <= 32 * EPS * emax)
    else:
        assert np.array_equal(g.v, vel)


def separate_kernels(hip, pos, vel, geom, Es, kick, wrap, start):
    """pinc_hip_accelerate, then pinc_hip_move_classify(doMove = 1): (x', v', flags, chunkCount)"""
    import torch
    sp = DevSpecies(pos, vel, start)
    n = sp.n
    part = torch.zeros((n + 1) // 1024 + 8, dtype=torch.float64, device="cuda")
    nb = C.c_int()
    if kick:
        Et = _dev(Es.ravel())
        assert hip.pinc_hip_accelerate(sp.pop, 0, geom_of(geom), Et.data_ptr(), part.data_ptr(), C.byref(nb), None) == 0
    flags = torch.zeros(sp.cap, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros((n + 2047) // 2048 + 1, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert hip.pinc_hip_move_classify(sp.pop, 0, 1, _thr_c(geom), flags.data_ptr(), cnt.data_ptr(), 1.0, err.data_ptr(),
                                      wrap, None) == 0
    torch.cuda.synchronize()
    assert int(err[0]) == 0
    return sp.live(sp.xs), sp.live(sp.vs), flags.cpu().numpy()[start:start + n], cnt.cpu().numpy()[:(n + 2047) // 2048]


def plain_case(hip, geom, pos, vel, *, kick, wrap, start, inplace=False, obj=None, seed=1, Es=None):
    """a plain push against the reference and the separate kernels; returns (gpu, ref)"""
    nd = len(geom)
    if kick and Es is None:
        Es = R.random_E(geom, np.random.default_rng(seed), wrap)
    r = R.push_reference(pos, vel, Es, geom, R.thresholds(geom), wrap, kick, obj)
    sp = DevSpecies(pos, vel, start)
    out = None if inplace else DevSpecies.blank(sp.n, nd, start)
    g = run_push(hip, sp, geom, kick=kick, Es=Es, wrap=wrap, out=out, obj=obj)
    # the same push writing only the flags that are not the centre
    sp2 = DevSpecies(pos, vel, start)
    out2 = None if inplace else DevSpecies.blank(sp.n, nd, start)
    gs = run_push(hip, sp2, geom, kick=kick, Es=Es, wrap=wrap, out=out2, obj=obj, sparse=1)
    assert np.array_equal(gs.flag, g.flag) and np.array_equal(gs.chunk, g.chunk) and gs.emig == g.emig
    assert np.array_equal(gs.x, g.x) and np.array_equal(gs.v, g.v)
    check_particles(g, r, vel, Es, kick)
    check_sums(g, r, kick)
    check_charge(g.rho, r, geom, wrap)
    print(f"paths: {int(g.diag[1])} particles gathered E from memory, {int(g.diag[2])} deposit runs added to memory, "
          f"of {len(pos)}")
    for s in (sp, out or sp):
        assert s.padding_untouched(s.xs) and s.padding_untouched(s.vs)
    if not inplace:
        assert np.array_equal(sp.live(sp.xs), pos) and np.array_equal(sp.live(sp.vs), vel)
    if obj is None:
        x2, v2, f2, c2 = separate_kernels(hip, pos, vel, geom, Es, kick, wrap, start)
        assert np.array_equal(g.x, x2) and np.array_equal(g.v, v2) and np.array_equal(g.flag, f2)
        assert np.array_equal(g.chunk, c2)
    else:
        assert np.array_equal(g.obj_count[:obj["n"]], r.obj_count) and g.obj_count[obj["n"]] == 0
    return g, r


def full_wrap(geom):
    return (1 << len(geom)) - 1


SHAPES = [(8, 8, 8), (20, 12, 16), (16, 24), (64,)]
_gid = lambda g: "x".join(map(str, g))


@pytest.mark.parametrize("start", [0, 1])
@pytest.mark.parametrize("n", [1, 5, 1023, 1024, 1025, 4099])
@pytest.mark.parametrize("geom", SHAPES, ids=_gid)
@pytest.mark.parametrize("kick", [0, 1])
def test_plain_push_shapes(hip, kick, geom, n, start):
    """k_push<ND, V3D, kick, false, false> for ND = 3, 2, 1; start 0: the
    aligned path (full blocks through the lane exchange), start 1: the
    unaligned one; n = 1023 / 1024 / 1025 / 4099: a partial block alone, a
    full one, full + partial, four full + a partial one.  Order (c): the
    first half cell-ordered and slow (LDS boxes, images gated off away from
    the faces), the second uniform and fast (the boxes exceed the LDS: global
    atomics; every face is crossed)."""
    pos, vel = R.generate("c", geom, n, kick, seed=100 + n)
    plain_case(hip, geom, pos, vel, kick=kick, wrap=full_wrap(geom), start=start)


def test_plain_push_more_than_512_blocks(hip):
    """n = 1024 * 582 + 17: 583 blocks, so push_chunk_of permutes the first
    512 chunks over the XCDs and leaves the tail of 71 in order (3-D, kick,
    aligned, full + partial)."""
    geom = (20, 12, 16)
    n = 1024 * 582 + 17
    pos, vel = R.generate("c", geom, n, 1, seed=7)
    g, _ = plain_case(hip, geom, pos, vel, kick=1, wrap=7, start=0)
    assert g.nb == 583


def _gpu_sorted(hip, pos, vel, geom, start=0):
    """the particles after pinc_hip_sort_tiles (host copies)"""
    import torch
    sp = DevSpecies(pos, vel, start)
    out = DevSpecies.blank(sp.n, sp.nd, start)
    nk = C.c_long()
    g = geom_of(geom)
    assert hip.pinc_hip_sort_tiles(sp.pop, out.pop, 0, g, TW, None, 0, C.byref(nk), None) != 0
    need = 2 * (nk.value + 1) + 2 * (nk.value // 4096 + 1) + 1
    work = torch.zeros(need, dtype=torch.int32, device="cuda")
    assert hip.pinc_hip_sort_tiles(sp.pop, out.pop, 0, g, TW, work.data_ptr(), need, C.byref(nk), None) == 0
    torch.cuda.synchronize()
    assert nk.value == R.tile_geo(geom, TW)[3] == hip.pinc_hip_tile_keys(g, TW)
    return out.live(out.xs), out.live(out.vs)


@pytest.mark.parametrize("order", ["a", "b", "c"])
@pytest.mark.parametrize("geom", SHAPES, ids=_gid)
@pytest.mark.parametrize("kick", [0, 1])
def test_plain_push_particle_orders(hip, kick, geom, order):
    """(a) uniform over the domain, |v| up to 0.95: node boxes beyond the LDS
    (global-atomic deposit, E gathered from memory), every face crossed;
    (b) the same particles after pinc_hip_sort_tiles with |v| <= 0.05: LDS
    boxes, interior blocks with their images gated off; (c) half and half.
    In place (xout = pop.x, vout = pop.v), as the host's plain push."""
    n = 4099
    rng = np.random.default_rng(31)
    pos, vfast = R.uniform_particles(geom, n, rng, R.V_MAX - (R.E_MAX if kick else 0))
    vslow = rng.uniform(-0.05, 0.05, size=pos.shape)
    if order == "a":
        vel = vfast
    else:
        pos, vel = _gpu_sorted(hip, pos, vslow, geom)
        c = np.clip(pos.astype(np.int64), 0, np.array(geom) + 1)
        assert np.all(np.diff(R.cell_keys(c, geom, TW)) >= 0)      # the numpy key is the sort's
        if order == "c":
            pos[n // 2:], vel[n // 2:] = R.uniform_particles(geom, n - n // 2, rng, vfast.max())
    plain_case(hip, geom, pos, vel, kick=kick, wrap=full_wrap(geom), start=0, inplace=True)


@pytest.mark.parametrize("embedded", [0, 1], ids=["alone", "after-a-full-block"])
@pytest.mark.parametrize("geom", SHAPES, ids=_gid)
@pytest.mark.parametrize("kick", [0, 1])
@pytest.mark.parametrize("wrap", ["none", "all"])
def test_plain_push_edges(hip, wrap, kick, geom, embedded):
    """Hand-placed dyadic particles: x' on lo and on up, one ulp below each,
    x on a node (weights exactly 1 and 0), v = 0, two and three faces crossed
    at a corner; alone (one partial block) and at the end of a full block
    plus a partial one.  kick = 1 gathers a zero field, so the sums stay exact."""
    pos, vel = R.edge_particles(geom)
    if embedded:
        p0, v0 = R.generate("b", geom, 1024 + 100, 0, seed=9)
        pos, vel = np.concatenate([p0, pos]), np.concatenate([v0, vel])
    Es = np.zeros(R.slab_shape(geom) + (len(geom),))
    w = full_wrap(geom) if wrap == "all" else 0
    g, r = plain_case(hip, geom, pos, vel, kick=kick, wrap=w, start=0, Es=Es)
    ne = len(R.edge_particles(geom)[0])
    if wrap == "none":
        want = {3: [13, 14, 12, 13, 13, 13, 9, 18], 2: [4, 5, 3, 4, 4, 4, 0, 0], 1: [1, 2, 0, 1, 1, 1, 0, 0]}[len(geom)]
        assert g.flag[-ne:].tolist() == want
    else:
        assert np.all(g.flag == R.centre(len(geom)))


@pytest.mark.parametrize("geom,wrap", [((20, 12, 16), 7), ((20, 12, 16), 3), ((20, 12, 16), 0), ((16, 24), 3),
                                       ((16, 24), 1)], ids=["3d-7", "3d-3", "3d-0", "2d-3", "2d-1"])
@pytest.mark.parametrize("kick", [0, 1])
def test_plain_push_wrap_masks(hip, kick, geom, wrap):
    """wrapMask 7: every crossing wrapped in place, nothing flagged; 3 (2-D:
    1): crossings of the slab dimension emigrate with the slab digit alone
    (3-D flags 4 and 22), the stayers' deposit reaches ghost plane nloc + 1;
    0: the full 3^nd code.  Non-stayers are not deposited: the charge is the
    reference's, which deposits the centre flags only."""
    nd = len(geom)
    pos, vel = R.generate("a", geom, 4099, kick, seed=17)
    g, r = plain_case(hip, geom, pos, vel, kick=kick, wrap=wrap, start=0)
    codes = set(np.unique(g.flag).tolist())
    centre = R.centre(nd)
    if wrap == full_wrap(geom):
        assert codes == {centre} and g.emig == 0 and not g.chunk.any()
    elif wrap == 0:
        faces = {centre + s * 3 ** d for d in range(nd) for s in (-1, 1)}
        assert faces <= codes and len(codes) > 2 * nd + 1      # faces, and edges or corners
    else:
        slab = 3 ** (nd - 1)
        assert codes == {centre - slab, centre, centre + slab}
        assert g.emig == int(np.count_nonzero(g.flag != centre)) > 0
        assert r.rho[geom[-1] + 1].sum() > 0 and g.rho[geom[-1] + 1].sum() > 0
    assert abs(g.rho.sum() - np.count_nonzero(g.flag == centre)) < 1e-9 * len(pos)


def _objects(geom):
    tx, ty, tz = geom
    inside = np.zeros((tz + 2, ty + 2, tx + 2), dtype=np.uint8)
    inside[6:9, 4:7, 5:8] = 1          # a 3 x 3 x 3 block of nodes
    inside[12, 9, 15] = 2              # a single node
    return {"inside": inside, "lo": (5, 4, 6), "hi": (15, 9, 12), "n": 2}


@pytest.mark.parametrize("kick", [0, 1])
def test_plain_push_objects(hip, kick):
    """k_push<3, true, kick, false, true>: a stayer whose moved cell's lower
    node has an id is flagged PINC_NE_SINK, counted per id and in chunkCount
    and emigTotal, and not deposited; one in the bounding box at an id-0 node
    is unaffected."""
    geom = (20, 12, 16)
    obj = _objects(geom)
    pos, vel = R.generate("a", geom, 40_000, kick, seed=29)
    g, r = plain_case(hip, geom, pos, vel, kick=kick, wrap=7, start=0, obj=obj)
    assert np.all(r.obj_count > 0) and g.emig == int(r.obj_count.sum())
    assert np.array_equal(np.nonzero(g.flag == R.NE_SINK)[0], np.nonzero(r.flag == R.NE_SINK)[0])
    cell = g.x.astype(np.int64)
    inbb = np.all((cell >= obj["lo"]) & (cell <= obj["hi"]), axis=1)
    assert np.count_nonzero(inbb & (g.flag == 13)) > 0
    assert abs(g.rho.sum() - (len(pos) - g.emig)) < 1e-9 * len(pos)


def _count_keys(hip, pos, vel, geom):
    import torch
    nk = R.tile_geo(geom, TW)[3]
    cnt = torch.zeros(nk + 1, dtype=torch.int32, device="cuda")
    if len(pos):
        sp = DevSpecies(pos, vel, 0)
        assert hip.pinc_hip_count_keys(sp.pop, 0, 0, geom_of(geom), TW, cnt.data_ptr(), None) == 0
        torch.cuda.synchronize()
    return cnt


def _scan(hip, cnt, nk):
    import torch
    cur = torch.zeros(nk + 1, dtype=torch.int32, device="cuda")
    work = torch.zeros(2 * (nk // 4096 + 1) + 1, dtype=torch.int32, device="cuda")
    assert hip.pinc_hip_scan_keys(cnt.data_ptr(), nk, cur.data_ptr(), work.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return cur


@pytest.mark.parametrize("geom,wrap", [((20, 12, 16), 7), ((20, 12, 16), 3), ((16, 24), 3), ((64,), 1)],
                         ids=["3d-7", "3d-3", "2d-3", "1d-1"])
@pytest.mark.parametrize("kick", [0, 1])
def test_counting_push(hip, kick, geom, wrap):
    """A plain push with cntNext: the counts equal pinc_hip_count_keys over
    the stayers of its output (compacted on the host) and the numpy key's
    histogram.  Order (c): brick counters in LDS and, for the far movers,
    counts straight to memory."""
    import torch
    nd = len(geom)
    pos, vel = R.generate("c", geom, 4099, kick, seed=41)
    Es = R.random_E(geom, np.random.default_rng(2), wrap) if kick else None
    nk = R.tile_geo(geom, TW)[3]
    cn = torch.zeros(nk + 1, dtype=torch.int32, device="cuda")
    sp = DevSpecies(pos, vel, 0)
    g = run_push(hip, sp, geom, kick=kick, Es=Es, wrap=wrap, out=DevSpecies.blank(sp.n, nd, 0), cnt_next=cn)
    cs = torch.zeros_like(cn)
    s = run_push(hip, sp, geom, kick=kick, Es=Es, wrap=wrap, out=DevSpecies.blank(sp.n, nd, 0), cnt_next=cs, sparse=1)
    assert np.array_equal(s.flag, g.flag) and np.array_equal(s.chunk, g.chunk) and torch.equal(cs, cn)
    r = R.push_reference(pos, vel, Es, geom, R.thresholds(geom), wrap, kick)
    check_particles(g, r, vel, Es, kick)
    check_sums(g, r, kick)
    check_charge(g.rho, r, geom, wrap)
    stay = g.flag == R.centre(nd)
    want = np.bincount(R.brick_keys(g.x[stay], g.v[stay], geom, TW), minlength=nk + 1)
    assert np.array_equal(cn.cpu().numpy(), want)
    assert np.array_equal(_count_keys(hip, g.x[stay], g.v[stay], geom).cpu().numpy(), want)


def _rows(*cols):
    a = np.column_stack(cols)
    return a[np.lexsort(a.T[::-1])]


def sorting_case(hip, geom, pos, vel, *, kick, wrap, start=0, cursor=None, seed=3, obj=None):
    """A sorting push of (pos, vel) (cursor None: count_keys + scan_keys as
    push_all) against the plain push and the reference on the same input;
    run twice, with flagsSparse 0 and 1."""
    import torch
    nd, n = len(geom), len(pos)
    Es = R.random_E(geom, np.random.default_rng(seed), wrap) if kick else None
    nk = R.tile_geo(geom, TW)[3]
    keys = R.brick_keys(pos, vel, geom, TW)           # ranked by the input's x + v (before the kick)
    sp = DevSpecies(pos, vel, start)
    if cursor is None:
        cnt = torch.zeros(nk + 1, dtype=torch.int32, device="cuda")
        assert hip.pinc_hip_count_keys(sp.pop, 0, 0, geom_of(geom), TW, cnt.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(cnt.cpu().numpy(), np.bincount(keys, minlength=nk + 1))
        cursor = _scan(hip, cnt, nk)
    offsets = cursor.cpu().numpy().astype(np.int64)
    assert np.array_equal(offsets[1:], np.cumsum(np.bincount(keys, minlength=nk + 1))[:nk])
    slot_key = np.searchsorted(offsets, np.arange(n), side="right") - 1
    r = R.push_reference(pos, vel, Es, geom, R.thresholds(geom), wrap, kick, obj)
    # the plain push on this input is the reference's
    plain = run_push(hip, sp, geom, kick=kick, Es=Es, wrap=wrap, out=DevSpecies.blank(n, nd, start), obj=obj)
    check_particles(plain, r, vel, Es, kick)
    want = _rows(keys, plain.x, plain.v, plain.flag)
    for sparse in (0, 1):
        out = DevSpecies.blank(n, nd, start)
        g = run_push(hip, sp, geom, kick=kick, Es=Es, wrap=wrap, out=out, cursor=cursor.clone(), obj=obj,
                     sparse=sparse)
        print(f"diag[0] (items given a global slot one by one) = {int(g.diag[0])} of {n}")
        # the input is only read and nothing is written outside [0, n)
        assert np.array_equal(sp.live(sp.xs), pos) and np.array_equal(sp.live(sp.vs), vel)
        assert out.padding_untouched(out.xs) and out.padding_untouched(out.vs)
        assert not np.any(g.x == SENTINEL) and not np.any(g.flag == FLAG_FILL)
        # rows (key of the slot's range, x', v', flag) jointly: each range
        # [offsets[b], offsets[b + 1]) holds exactly the particles of brick
        # key b, with their own velocities and flags (the flags by slot: the
        # sparse run leaves the pre-set centre where it writes none).  That
        # every slot of [0, n) is written exactly once is inferred: the n
        # slots hold the plain push's n rows and no sentinel, so none was
        # written twice over another left out.
        np.testing.assert_array_equal(_rows(slot_key, g.x, g.v, g.flag), want)
        # chunkCount by destination chunk
        leave = np.nonzero(g.flag != R.centre(nd))[0]
        assert np.array_equal(g.chunk, np.bincount(leave // R.PINC_CHUNK, minlength=len(g.chunk)))
        assert g.emig == len(leave) == r.emig_total
        check_sums(g, r, kick)
        check_charge(g.rho, r, geom, wrap)
        if obj is not None:
            assert np.array_equal(g.obj_count[:obj["n"]], r.obj_count) and g.obj_count[obj["n"]] == 0
    return g


def _fresh(hip, geom, n, seed, start=0):
    rng = np.random.default_rng(seed)
    pos, _ = R.uniform_particles(geom, n, rng, 0.05)
    return _gpu_sorted(hip, pos, rng.uniform(-0.05, 0.05, size=pos.shape), geom, start)


@pytest.mark.parametrize("geom,n,start", [((20, 12, 16), 5, 0), ((20, 12, 16), 1025, 0), ((20, 12, 16), 40_000, 0),
                                          ((16, 24), 10_000, 0), ((20, 12, 16), 1025, 1), ((64,), 3000, 0)],
                         ids=["3d-5", "3d-1025", "3d-40000", "2d-10000", "3d-1025-start1", "1d-3000"])
@pytest.mark.parametrize("kick", [0, 1])
@pytest.mark.parametrize("wrap", ["all", "not-slab"])
def test_sorting_push_fresh(hip, wrap, kick, geom, n, start):
    """k_push<ND, V3D, kick, true, false> on a freshly sorted input with
    |v| <= 0.05 (brick and cell-rank counters in LDS), set up as push_all
    does: sort_tiles, count_keys, scan_keys, push(cursor)."""
    pos, vel = _fresh(hip, geom, n, seed=n, start=start)
    w = full_wrap(geom) if wrap == "all" else full_wrap(geom) >> 1
    sorting_case(hip, geom, pos, vel, kick=kick, wrap=w, start=start)


@pytest.mark.parametrize("kick", [0, 1])
def test_sorting_push_objects(hip, kick):
    """k_push<3, true, kick, true, true>: the sorting push with the object
    test; the collected particles' PINC_NE_SINK flags land at their slots and
    count in the destination chunks."""
    geom = (20, 12, 16)
    obj = _objects(geom)
    pos, vel = _fresh(hip, geom, 40_000, seed=19)
    g = sorting_case(hip, geom, pos, vel, kick=kick, wrap=7, obj=obj)
    assert np.all(g.obj_count[:2] > 0) and np.count_nonzero(g.flag == R.NE_SINK) == g.obj_count[:2].sum()


def _decayed(hip, geom, n, pushes, seed):
    """sorted, then `pushes` plain pushes at |v| ~ 0.5 wrapped in place"""
    rng = np.random.default_rng(seed)
    pos, _ = R.uniform_particles(geom, n, rng, 0.05)
    vel = rng.uniform(0.3, 0.6, size=pos.shape) * rng.choice([-1.0, 1.0], size=pos.shape)
    pos, vel = _gpu_sorted(hip, pos, vel, geom)
    sp = DevSpecies(pos, vel, 0)
    for _ in range(pushes):
        run_push(hip, sp, geom, kick=0, wrap=full_wrap(geom))
    return sp.live(sp.xs), sp.live(sp.vs)


@pytest.mark.parametrize("geom,n", [((20, 12, 16), 40_000), ((16, 24), 10_000)], ids=["3d-40000", "2d-10000"])
@pytest.mark.parametrize("kick", [0, 1])
def test_sorting_push_decayed(hip, kick, geom, n):
    """The same after the order has decayed by six plain pushes at
    |v| = 0.3 .. 0.6: particles that wrapped through a periodic face lie far
    from their block's bricks and take a global slot one by one (diag[0] > 0:
    the fallback runs)."""
    pos, vel = _decayed(hip, geom, n, 6, seed=n + 1)
    g = sorting_case(hip, geom, pos, vel, kick=kick, wrap=full_wrap(geom))
    assert g.diag[0] > 0


@pytest.mark.parametrize("kick", [0, 1])
def test_counting_push_then_sorting_push(hip, kick):
    """push_all's chain: a counting push, the swap, then a sorting push whose
    cursor is the scan of cntNext (no count_keys), wrapMask 7."""
    import torch
    geom, n = (20, 12, 16), 40_000
    pos, vel = _decayed(hip, geom, n, 2, seed=77)
    nk = R.tile_geo(geom, TW)[3]
    cn = torch.zeros(nk + 1, dtype=torch.int32, device="cuda")
    Es = R.random_E(geom, np.random.default_rng(5), 7) if kick else None
    sp = DevSpecies(pos, vel, 0)
    out = DevSpecies.blank(n, 3, 0)
    g = run_push(hip, sp, geom, kick=kick, Es=Es, wrap=7, out=out, cnt_next=cn)
    assert g.emig == 0
    sorting_case(hip, geom, g.x, g.v, kick=kick, wrap=7, cursor=_scan(hip, cn, nk))
