"""The four entry points of k_objects.hip called through the C ABI, against
the numpy restatement tests/glue_ref.py.

pinc_hip_obj_flag: species 1 of 2 at an odd iStart, 2 * 2048 + 37 particles
over the padded frame of a 16 x 10 x 12 grid whose mask holds a 3 x 3 x 3
block (id 1), a single node (id 2) and the corner ghost node (id 3); planted
particles sit exactly on a node's integer and one step below it, in (-1, 0)
(C truncation: cell 0), and outside the node table on either side; the first
chunk is all hits, the second has none.  Flags, per-chunk counts and
per-object counts are exact (integers: no bound).  The flags and counts then
go to pinc_hip_extract as pinc_obj.c hands them over, and the survivors'
order is the serial back-fill's (tests/migrate_ref.py).

pinc_hip_obj_gather, _add, _correct: n in {1, 255, 256, 257, 600} surface
nodes, distinct indices with about one in five -1, a matrix that is not
symmetric.  Bit for bit against the restatement (the expression order is
fixed: c += M[j][i] (phiC - phiS[j]) for j = 0..n-1 from 0.0, then one add
into rho).  The correction also lies within

    (n + 2) eps sum_j |M[j][i] (phiC - phiS[j])|

of the long-double sum: one subtraction and one product per term (eps
together), n - 1 additions (eps / 2 each, of partial sums below the magnitude
sum), and the final add into rho, eps / 2 of |rho'|, which the input builder
keeps below 1.26 times the magnitude sum (rho starts below a quarter of it):
(n + 1) / 2 + 0.63 < n + 2 times eps.

Every output sits pre-filled between guard elements of its own type; what
lies outside the documented write range comes back unchanged, and so do the
inputs.  tests/test_glue_ref_cpu.py shows that these inputs tell mutants
(floor, chunks from slot 0, M transposed) apart.
"""
import ctypes as C

import numpy as np
import pytest

import glue_ref as G
import migrate_ref as M
from gpu_buf import Buf, IntBuf, same_bits
from migrate_ref import ExtractWs
from push_abi import Pop

pytestmark = pytest.mark.gpu

LD = G.LD
BYTE_FILL = 0xEE
COUNT_FILL = -5
OBJ_PRE = (100, 200, 300)
GUARD = 64
INT_GUARD = -77


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available()
    from pinc_amd import _lib
    h = _lib.HIP
    vp, ci, cl, cd, lp = C.c_void_p, C.c_int, C.c_long, C.c_double, C.POINTER(C.c_long)
    h.pinc_hip_obj_flag.argtypes = [Pop, ci, vp, cl, cl, cl, vp, vp, vp, vp]
    h.pinc_hip_obj_gather.argtypes = [vp, vp, cl, vp, vp]
    h.pinc_hip_obj_correct.argtypes = [vp, vp, cl, cd, vp, vp, vp]
    h.pinc_hip_obj_add.argtypes = [vp, vp, cl, cd, vp]
    h.pinc_hip_extract.argtypes = [Pop, ci, vp, vp, ci, ci, ExtractWs, lp, lp, vp]
    return h


@pytest.fixture(scope="module")
def case():
    pos, _ = G.obj_particles()
    vel = -pos - 0.125
    mask, sy, sz, nn = G.obj_mask()
    flags, cc, cnt = G.obj_flag(pos, mask, sy, sz, nn)
    for a in (pos, vel, mask, flags, cc, cnt):
        a.setflags(write=False)
    return G.SimpleNamespace(pos=pos, vel=vel, mask=mask, sy=sy, sz=sz, nn=nn, flags=flags, cc=cc, cnt=cnt)


class FlagBufs:
    """the mask (between guards of id 7: a read outside the table would flag
    and count) and the three outputs of pinc_hip_obj_flag, pre-filled"""

    def __init__(self, case, cap):
        self.mask = IntBuf(case.mask.ravel(), guard=7)
        self.flags = IntBuf(np.full(cap, BYTE_FILL, dtype=np.uint8), guard=0xAA)
        self.chunk = IntBuf(np.full(len(case.cc) + 5, COUNT_FILL, dtype=np.int32))
        self.obj = IntBuf(np.array(OBJ_PRE, dtype=np.int32))

    def call(self, hip, pop, case):
        return hip.pinc_hip_obj_flag(pop, 1, self.mask.ptr, case.sy, case.sz, case.nn, self.flags.ptr, self.chunk.ptr,
                                     self.obj.ptr, None)

    def untouched(self):
        return self.flags.unchanged() and self.chunk.unchanged() and self.obj.unchanged() and self.mask.unchanged()


def test_obj_flag(hip, case):
    """flags 0 where the node's id is not 0 and 13 elsewhere over [iStart,
    iStop) only; chunkCount[b] exact per 2048 particles from iStart for b <
    3, untouched behind; objCount[id - 1] increased by the exact count"""
    sp = G.species_1_of_2(case.pos, case.vel)
    b = FlagBufs(case, sp.cap)
    assert b.call(hip, sp.pop, case) == 0
    want = np.full(sp.cap, BYTE_FILL, dtype=np.uint8)
    want[sp.start:sp.start + sp.n] = case.flags
    np.testing.assert_array_equal(b.flags.get(), want)
    nch = -(-sp.n // G.CHUNK)
    assert nch == len(case.cc) == 3
    np.testing.assert_array_equal(b.chunk.get(), np.concatenate([case.cc, np.full(5, COUNT_FILL, dtype=np.int32)]))
    np.testing.assert_array_equal(b.obj.get(), np.array(OBJ_PRE, dtype=np.int32) + case.cnt)
    assert b.mask.unchanged()
    np.testing.assert_array_equal(sp.live(sp.xs), case.pos)
    np.testing.assert_array_equal(sp.live(sp.vs), case.vel)
    assert sp.padding_untouched(sp.xs) and sp.padding_untouched(sp.vs)


def test_obj_flag_is_3d_only(hip, case):
    sp = G.species_1_of_2(case.pos, case.vel)
    sp.pop.nd = 2
    b = FlagBufs(case, sp.cap)
    assert b.call(hip, sp.pop, case) != 0
    assert b"3-D" in hip.pinc_hip_error_string()
    assert b.untouched()


def test_obj_flag_of_no_particles(hip, case):
    sp = G.species_1_of_2(case.pos, case.vel)
    sp.pop.iStop[1] = sp.pop.iStart[1]
    b = FlagBufs(case, sp.cap)
    assert b.call(hip, sp.pop, case) == 0
    assert b.untouched()


def _ints(size):
    import torch
    t = torch.zeros(size + GUARD, dtype=torch.int32, device="cuda")
    t[size:] = INT_GUARD
    return t


def test_obj_flag_then_extract(hip, case):
    """pinc_obj.c's collection: obj_flag's flags and chunk counts handed to
    pinc_hip_extract with centre 13.  The removed particles arrive in the
    buffer in the serial loop's extraction order, the survivors in its
    back-fill order; every flag is the centre again.  Exact."""
    import torch
    from push_abi import SENTINEL
    sp = G.species_1_of_2(case.pos, case.vel)
    n = sp.n
    b = FlagBufs(case, sp.cap)
    b.flags = IntBuf(np.full(sp.cap, G.CENTRE3, dtype=np.uint8), guard=0xAA)   # the host keeps idle flags at the centre
    assert b.call(hip, sp.pop, case) == 0
    slots, order = M.serial_backfill(case.flags, G.CENTRE3)
    E = len(order)
    nch = len(case.cc)
    size = {"chunkOffset": nch + 1, "scanWork": 2 * -(-nch // 4096) + 1, "tail": E + 1, "holes": E + 1, "order": E,
            "blockHist": 28 * -(-E // 1024) + 28, "scratch": 92}
    ints = {k: _ints(v) for k, v in size.items()}
    buf = torch.full((6 * E + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    buf_ne = torch.full((E + GUARD,), BYTE_FILL, dtype=torch.uint8, device="cuda")
    ws = ExtractWs(*[ints[k].data_ptr() for k in ("chunkOffset", "scanWork", "tail", "holes", "order", "blockHist",
                                                  "scratch")], buf.data_ptr(), buf_ne.data_ptr(), E)
    n_rem, ne_count = C.c_long(-1), (C.c_long * M.NE_CODES)()
    assert hip.pinc_hip_extract(sp.pop, 1, b.flags.ptr, b.chunk.ptr, G.CENTRE3, 27, ws, C.byref(n_rem), ne_count,
                                None) == 0
    torch.cuda.synchronize()
    assert n_rem.value == E == int(case.cc.sum())
    assert list(ne_count) == [E] + [0] * (M.NE_CODES - 1)          # flag 0: the first direction's bucket
    hb = buf.cpu().numpy()
    assert np.all(hb[6 * E:] == SENTINEL) and np.all(buf_ne.cpu().numpy()[E:] == BYTE_FILL)
    hb = hb[:6 * E].reshape(6, E)
    np.testing.assert_array_equal(hb[:3].T, case.pos[order])
    np.testing.assert_array_equal(hb[3:].T, case.vel[order])
    np.testing.assert_array_equal(sp.live(sp.xs)[:n - E], case.pos[slots])
    np.testing.assert_array_equal(sp.live(sp.vs)[:n - E], case.vel[slots])
    assert sp.padding_untouched(sp.xs) and sp.padding_untouched(sp.vs)
    assert np.all(b.flags.get() == G.CENTRE3)
    for k, t in ints.items():
        assert bool((t[size[k]:] == INT_GUARD).all()), k
    np.testing.assert_array_equal(b.chunk.get()[:nch], case.cc)


# --------------------------------------------------------- surface nodes ---
@pytest.mark.parametrize("n", G.SURFACE_N)
def test_gather_add_correct(hip, n):
    """gather: grid[idx] and +0.0 where idx < 0, bit for bit.  add: the
    listed nodes plus v, every other node's bits unchanged.  correct: bit for
    bit against the j = 0..n-1 accumulation, and within (n + 2) eps sum_j
    |M[j][i] (phiC - phiS[j])| of the long-double sum (the module docstring
    has the count); rows with idx < 0 add nothing.  Measured on an MI355X:
    0.160 of the bound at n = 1, at most 0.006 from n = 255 on."""
    c = G.surface_case(n)
    idx = IntBuf(c.idx, guard=-1)
    live = c.idx >= 0
    grid, out = Buf(c.grid), Buf(np.full(n, np.nan))
    assert hip.pinc_hip_obj_gather(grid.ptr, idx.ptr, n, out.ptr, None) == 0
    assert same_bits(out.get(), G.obj_gather(c.grid, c.idx))
    assert grid.unchanged()
    assert hip.pinc_hip_obj_add(grid.ptr, idx.ptr, n, c.v, None) == 0
    assert same_bits(grid.get(), G.obj_add(c.grid, c.idx, c.v))
    Mb, phiS, rho = Buf(c.M), Buf(c.phiS), Buf(c.rho)
    assert hip.pinc_hip_obj_correct(Mb.ptr, phiS.ptr, n, c.phiC, idx.ptr, rho.ptr, None) == 0
    got = rho.get()
    assert same_bits(got, G.obj_correct(c.M, c.phiS, c.phiC, c.idx, c.rho))
    ref, S = G.obj_correct_ld(c.M, c.phiS, c.phiC)
    at = c.idx[live]
    err = np.abs(got[at].astype(LD) - (c.rho[at].astype(LD) + ref[live]))
    lim = (n + 2) * G.EPS * S[live]
    print(f"n = {n}: correction error / bound {float(np.max(err / lim)):.3f}")
    assert np.all(err <= lim)
    assert Mb.unchanged() and phiS.unchanged() and idx.unchanged()


def test_surface_entries_with_nothing_to_do(hip):
    c = G.surface_case(255)
    idx = IntBuf(c.idx, guard=-1)
    grid, out, Mb, phiS = Buf(c.grid), Buf(np.full(255, np.nan)), Buf(c.M), Buf(c.phiS)
    for n in (0, -3):
        assert hip.pinc_hip_obj_gather(grid.ptr, idx.ptr, n, out.ptr, None) == 0
        assert hip.pinc_hip_obj_add(grid.ptr, idx.ptr, n, c.v, None) == 0
        assert hip.pinc_hip_obj_correct(Mb.ptr, phiS.ptr, n, c.phiC, idx.ptr, grid.ptr, None) == 0
    assert grid.unchanged() and out.unchanged()
