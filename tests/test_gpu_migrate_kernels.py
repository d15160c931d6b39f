"""The migration kernels of libpinc_hip.so through the C ABI, against the
serial loop they replace (tests/migrate_ref.py).

pinc_hip_extract (k_scan_*, k_extract_a/b, k_rank_*, k_hist_scan,
k_fill_holes) gets flags and chunk counts written by the test, so the
extraction is tested apart from the classification (which has its own
reference, tests/push_ref.py).  Every comparison is exact: nothing on this
path rounds but the one add of the import shift, which numpy performs alike.

A particle is identifiable in every component: original index i of species
s has x[d] = i + 0.125 (d + 1) + 1e7 s and v[d] = -x[d], exact in float64.
The species under test is species 1 of two, at a start that is no multiple
of 64, with species 0 live before it and sentinel padding behind it.  Every
work array has exactly the size include/pinc_hip.h documents, followed by 64
guard elements.
"""
import ctypes as C
import time

import numpy as np
import pytest

import migrate_ref as M
from migrate_ref import ExtractWs
from push_abi import SENTINEL, Pop

pytestmark = pytest.mark.gpu

N0 = 50                # live particles of species 0
START1 = N0 + 13       # iStart of species 1: 63
PAD1 = 11              # sentinel slots behind species 1
GUARD = 64
INT_GUARD = -77
BYTE_GUARD = 0xEE
SHIFT_T = (20, 12, 16)
SIZES = (1, 2, 63, 64, 65, 2047, 2048, 2049, 4096, 6000)
CASES = [(nd, n, name) for nd in (1, 2, 3) for n in SIZES for name in M.pattern_names(n)]


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available()
    from pinc_amd import _lib
    h = _lib.HIP
    vp, lp = C.c_void_p, C.POINTER(C.c_long)
    h.pinc_hip_extract.argtypes = [Pop, C.c_int, vp, vp, C.c_int, C.c_int, ExtractWs, lp, lp, vp]
    h.pinc_hip_pack.argtypes = [vp, C.c_long, vp, C.c_long, C.c_long, C.c_int, vp, vp]
    h.pinc_hip_import.argtypes = [Pop, C.c_int, C.c_long, vp, C.c_long, vp, C.c_long, C.c_long,
                                  C.POINTER(C.c_int), C.c_int, vp]
    h.pinc_hip_import_rec.argtypes = [Pop, C.c_int, C.c_long, vp, C.c_long, C.POINTER(C.c_int), vp]
    h.pinc_hip_mem_info.argtypes = [C.POINTER(C.c_ulong), C.POINTER(C.c_ulong)]
    return h


def ident(i, d, s):
    """coordinate d of the particle with original index i of species s"""
    return np.asarray(i, dtype=np.float64) + 0.125 * (d + 1) + 1e7 * s


def _guarded(size, dtype, fill, guard):
    """`size` elements of `fill` and GUARD elements of `guard` behind them, on the device"""
    import torch
    t = torch.full((size + GUARD,), fill, dtype=dtype, device="cuda")
    t[size:] = guard
    return t


class TwoSpecies:
    """Species 0 (N0 live, 13 free slots) and species 1 (n live at START1,
    `pad` sentinel slots behind) of an nd-dimensional population; x[d], v[d]
    null for d >= nd."""

    def __init__(self, nd, n, pad=PAD1):
        import torch
        self.nd, self.n, self.total = nd, n, START1 + n + pad
        self.hx = np.full((nd, self.total), SENTINEL)
        for d in range(nd):
            self.hx[d, :N0] = ident(np.arange(N0), d, 0)
            self.hx[d, START1:START1 + n] = ident(np.arange(n), d, 1)
        self.hv = -self.hx
        self.xs = [torch.from_numpy(self.hx[d].copy()).cuda() for d in range(nd)]
        self.vs = [torch.from_numpy(self.hv[d].copy()).cuda() for d in range(nd)]
        ptrs = lambda ts: (C.c_void_p * 3)(*([t.data_ptr() for t in ts] + [None] * (3 - nd)))
        self.pop = Pop(ptrs(self.xs), ptrs(self.vs), 2, nd, (C.c_long * 9)(0, START1, self.total),
                       (C.c_long * 8)(N0, START1 + n))

    def state(self):
        """host copies (nd, total) of the positions and the velocities"""
        return (np.stack([t.cpu().numpy() for t in self.xs]), np.stack([t.cpu().numpy() for t in self.vs]))


class Work:
    """pinc_extract_ws_t and the chunk counts for n particles, E emigrants
    and a buffer of cap entries, each array at its documented minimum."""
    INTS = ("chunkCount", "chunkOffset", "scanWork", "tail", "holes", "order", "blockHist", "scratch")

    def __init__(self, n, E, cap, counts):
        import torch
        nch = -(-n // M.CHUNK)
        assert len(counts) == nch and int(np.sum(counts)) == E
        self.size = {"chunkCount": nch, "chunkOffset": nch + 1, "scanWork": 2 * -(-nch // 4096) + 1,
                     "tail": E + 1, "holes": E + 1, "order": E, "blockHist": 28 * -(-E // 1024) + 28,
                     "scratch": 92, "buf": 6 * cap, "bufNe": cap}
        self.guard = {k: INT_GUARD for k in self.INTS}
        self.guard.update(buf=SENTINEL, bufNe=BYTE_GUARD)
        # (the work arrays proper start as zeros: a valid index wherever one is read)
        self.t = {k: _guarded(self.size[k], torch.int32, 0, INT_GUARD) for k in self.INTS}
        self.t["chunkCount"][:nch] = torch.from_numpy(np.asarray(counts, dtype=np.int32)).cuda()
        self.t["buf"] = _guarded(6 * cap, torch.float64, SENTINEL, SENTINEL)
        self.t["bufNe"] = _guarded(cap, torch.uint8, BYTE_GUARD, BYTE_GUARD)
        self.cap, self.counts = cap, np.asarray(counts, dtype=np.int32)
        self.ws = ExtractWs(*[self.t[k].data_ptr() for k in ("chunkOffset", "scanWork", "tail", "holes", "order",
                                                             "blockHist", "scratch", "buf", "bufNe")], cap)

    def broken_guards(self):
        return [k for k, t in self.t.items() if not bool((t[self.size[k]:] == self.guard[k]).all())]

    def buf(self):
        return self.t["buf"].cpu().numpy()[:6 * self.cap].reshape(6, self.cap)

    def buf_ne(self):
        return self.t["bufNe"].cpu().numpy()[:self.cap]


def _flags_of(pop2, flags, centre):
    import torch
    h = np.full(pop2.total, centre, dtype=np.uint8)
    h[START1:START1 + len(flags)] = flags
    return h, torch.from_numpy(h.copy()).cuda()


def _extract(hip, pop2, dflags, work, centre):
    import torch
    n_emig = C.c_long(-1)
    ne_count = (C.c_long * M.NE_CODES)()
    rc = hip.pinc_hip_extract(pop2.pop, 1, dflags.data_ptr(), work.t["chunkCount"].data_ptr(), centre,
                              3 ** pop2.nd, work.ws, C.byref(n_emig), ne_count, None)
    torch.cuda.synchronize()
    return rc, n_emig.value, np.array(list(ne_count), dtype=np.int64)


def _check_extracted(pop2, flags, centre, dflags, work, result):
    """everything test_extract_matches_serial_loop asserts of a successful call"""
    nd, n = pop2.nd, len(flags)
    rc, n_emig, ne_count = result
    slots, order = M.serial_backfill(flags, centre)
    idx, ne, count = M.bucket(order, flags)
    E = len(order)
    assert rc == 0
    assert n_emig == E
    np.testing.assert_array_equal(ne_count, count)
    # the buffer: direction-major, extraction order inside, the object sink last
    np.testing.assert_array_equal(work.buf_ne()[:E], ne)
    assert np.all(work.buf_ne()[E:] == BYTE_GUARD)
    want = np.full((6, work.cap), SENTINEL)
    for d in range(nd):
        want[d, :E] = ident(idx, d, 1)
        want[3 + d, :E] = -ident(idx, d, 1)
    np.testing.assert_array_equal(work.buf(), want)
    # the survivors, slot by slot; species 0 and the padding
    x, v = pop2.state()
    wx = pop2.hx.copy()
    stale = slice(START1 + n - E, START1 + n)        # slots the serial loop gives up: not specified
    for d in range(nd):
        wx[d, START1:START1 + n - E] = ident(slots, d, 1)
        x[d, stale] = wx[d, stale]
        v[d, stale] = -wx[d, stale]
    np.testing.assert_array_equal(x, wx)
    np.testing.assert_array_equal(v, -wx)
    # the flags are all the centre again; nothing else was written
    assert np.all(dflags.cpu().numpy() == centre)
    assert work.broken_guards() == []
    np.testing.assert_array_equal(work.t["chunkCount"].cpu().numpy()[:len(work.counts)], work.counts)
    return idx, ne, count


def _run_case(hip, nd, flags, cap=None):
    centre = M.centre(nd)
    pop2 = TwoSpecies(nd, len(flags))
    _, dflags = _flags_of(pop2, flags, centre)
    E = int(np.count_nonzero(flags != centre))
    work = Work(len(flags), E, E if cap is None else cap, M.chunk_counts(flags, centre))
    result = _extract(hip, pop2, dflags, work, centre)
    idx, ne, count = _check_extracted(pop2, flags, centre, dflags, work, result)
    return work, E, count


def _pattern(nd, n, name):
    rng = np.random.default_rng([nd, n, M.PATTERN_NAMES.index(name)])
    return M.pattern(name, n, M.centre(nd), M.codes(nd), rng)


@pytest.mark.parametrize("nd,n,name", CASES, ids=[f"{nd}d-{n}-{name}" for nd, n, name in CASES])
def test_extract_matches_serial_loop(hip, nd, n, name):
    """Return code, counts, the whole buffer in order, every survivor slot,
    the flags, and everything that must stay untouched, for every named
    pattern (migrate_ref.patterns) at particle counts around the wave (64),
    the chunk (2048) and, with E > 1024, several k_rank_* blocks."""
    flags = _pattern(nd, n, name)
    _, E, _ = _run_case(hip, nd, flags)
    if n == 6000 and name in ("random_0.5", "random_0.99", "all"):
        assert E > 1024                               # several k_rank_* blocks, cross-block blockHist offsets


def test_extract_capacity(hip):
    """One emigrant more than the buffer holds: PINC_ERR_CAPACITY with the
    count to grow to, and nothing touched; at exactly E the call succeeds."""
    nd, n = 3, 2049
    centre = M.centre(nd)
    flags = _pattern(nd, n, "random_0.5")
    E = int(np.count_nonzero(flags != centre))
    pop2 = TwoSpecies(nd, n)
    hflags, dflags = _flags_of(pop2, flags, centre)
    counts = M.chunk_counts(flags, centre)
    small = Work(n, E, E - 1, counts)
    rc, n_emig, _ = _extract(hip, pop2, dflags, small, centre)
    assert rc == M.ERR_CAPACITY and n_emig == E
    x, v = pop2.state()
    np.testing.assert_array_equal(x, pop2.hx)
    np.testing.assert_array_equal(v, pop2.hv)
    np.testing.assert_array_equal(dflags.cpu().numpy(), hflags)
    assert np.all(small.buf() == SENTINEL) and np.all(small.buf_ne() == BYTE_GUARD)
    assert small.broken_guards() == []
    np.testing.assert_array_equal(small.t["chunkCount"].cpu().numpy()[:len(counts)], counts)
    exact = Work(n, E, E, counts)
    _check_extracted(pop2, flags, centre, dflags, exact, _extract(hip, pop2, dflags, exact, centre))


def test_extract_many_chunks(hip):
    """4098 chunks: the multi-block scan of the chunk counts (k_scan_sums,
    k_scan_single, k_scan_apply) with a second scan block of two chunks.
    About 5000 scattered emigrants, 2048 consecutive ones across the border
    of the two scan blocks (chunks 4095 and 4096) and the last 300 slots,
    against the sparse serial loop."""
    import torch
    nd, centre = 3, 13
    n = 4097 * M.CHUNK + 5
    total = START1 + n + PAD1
    free, whole = C.c_ulong(), C.c_ulong()
    assert hip.pinc_hip_mem_info(C.byref(free), C.byref(whole)) == 0
    if free.value < 0.75e9:
        pytest.skip(f"needs about 0.5 GB of device memory, {free.value / 1e9:.2f} GB are free")
    t0 = time.perf_counter()
    # the population, built on the device
    slot = torch.arange(total, dtype=torch.float64, device="cuda")
    live = (slot < N0) | ((slot >= START1) & (slot < START1 + n))
    base = torch.where(slot >= START1, slot - START1 + 1e7, slot)
    del slot
    xs, vs = [], []
    for d in range(nd):
        xs.append(torch.where(live, base + 0.125 * (d + 1), SENTINEL))
        vs.append(torch.where(live, -xs[d], SENTINEL))
    del base, live
    ptrs = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
    pop = Pop(ptrs(xs), ptrs(vs), 2, nd, (C.c_long * 9)(0, START1, total), (C.c_long * 8)(N0, START1 + n))
    # the flags
    rng = np.random.default_rng(4098)
    where = np.unique(np.concatenate([rng.choice(n, size=5000, replace=False),
                                      4095 * M.CHUNK + 1024 + np.arange(M.CHUNK), np.arange(n - 300, n)]))
    flags = np.full(n, centre, dtype=np.uint8)
    flags[where] = rng.choice(M.codes(nd), size=len(where))
    dflags = torch.full((total,), centre, dtype=torch.uint8, device="cuda")
    dflags[torch.from_numpy(where + START1).cuda()] = torch.from_numpy(flags[where]).cuda()
    counts = M.chunk_counts(flags, centre)
    assert len(counts) == 4098 and counts[4095] == M.CHUNK // 2 + np.count_nonzero(
        flags[4095 * M.CHUNK:4095 * M.CHUNK + 1024] != centre)
    # the reference
    slots, order = M.serial_backfill_sparse(flags, centre)
    idx, ne, count = M.bucket(order, flags)
    E = len(order)
    m = n - E
    assert E == len(where)
    work = Work(n, E, E, counts)
    n_emig, ne_count = C.c_long(-1), (C.c_long * M.NE_CODES)()
    rc = hip.pinc_hip_extract(pop, 1, dflags.data_ptr(), work.t["chunkCount"].data_ptr(), centre, 27, work.ws,
                              C.byref(n_emig), ne_count, None)
    torch.cuda.synchronize()
    assert rc == 0 and n_emig.value == E
    np.testing.assert_array_equal(np.array(list(ne_count)), count)
    np.testing.assert_array_equal(work.buf_ne(), ne)
    buf = work.buf()
    for d in range(nd):
        np.testing.assert_array_equal(buf[d], ident(idx, d, 1))
        np.testing.assert_array_equal(buf[3 + d], -ident(idx, d, 1))
    # survivors: every slot that received a back-fill, a strided sample of the others, both ends
    holes = where[where < m]
    assert len(holes) and np.all(slots[holes] >= m)
    look = np.unique(np.concatenate([holes, np.arange(0, m, 4099), [0, m - 1]]))
    dlook = torch.from_numpy(look + START1).cuda()
    for d in range(nd):
        np.testing.assert_array_equal(xs[d][dlook].cpu().numpy(), ident(slots[look], d, 1))
        np.testing.assert_array_equal(vs[d][dlook].cpu().numpy(), -ident(slots[look], d, 1))
        head = np.where(np.arange(START1) < N0, ident(np.arange(START1), d, 0), SENTINEL)
        np.testing.assert_array_equal(xs[d][:START1].cpu().numpy(), head)
        np.testing.assert_array_equal(vs[d][:START1].cpu().numpy(), np.where(np.arange(START1) < N0, -head, SENTINEL))
        assert bool((xs[d][START1 + n:] == SENTINEL).all()) and bool((vs[d][START1 + n:] == SENTINEL).all())
    assert bool((dflags == centre).all())
    assert work.broken_guards() == []
    np.testing.assert_array_equal(work.t["chunkCount"].cpu().numpy()[:len(counts)], counts)
    print(f"many chunks: n = {n}, E = {E}, {len(holes)} holes, wall {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------ pack and import ---
LIVE = 17        # live particles of the receiving species
RANGES = ("whole", "first", "inner", "last", "empty")


@pytest.fixture(scope="module")
def extracted(hip):
    """per nd: the buffer a random_0.5 extraction at n = 2049 leaves (checked
    as in test_extract_matches_serial_loop) and the number of entries before
    the object sink's"""
    cache = {}

    def get(nd):
        if nd not in cache:
            work, E, count = _run_case(hip, nd, _pattern(nd, 2049, "random_0.5"))
            assert count[M.NE_SINK] > 0 and E - count[M.NE_SINK] > 307
            cache[nd] = (work, work.buf(), work.buf_ne(), int(E - count[M.NE_SINK]))
        return cache[nd]
    return get


@pytest.mark.parametrize("kind", RANGES)
@pytest.mark.parametrize("nd", [1, 2, 3])
def test_pack_and_import(hip, extracted, nd, kind):
    """pinc_hip_pack, pinc_hip_import (every shiftMask) and
    pinc_hip_import_rec on sub-ranges of an extraction's buffer, into a
    receiving species that is otherwise sentinel-filled: exact records,
    exact shifted particles, nothing else written."""
    import torch
    work, hbuf, hne, E = extracted(nd)
    first, count = {"whole": (0, E), "first": (0, 1), "inner": (7, 300), "last": (E - 1, 1), "empty": (5, 0)}[kind]
    shift_t = (C.c_int * 3)(*(SHIFT_T[:nd] + (0,) * (3 - nd)))
    buf, buf_ne = work.t["buf"].data_ptr(), work.t["bufNe"].data_ptr()
    # pack
    out = _guarded(count * M.REC, torch.float64, SENTINEL, SENTINEL)
    assert hip.pinc_hip_pack(buf, work.cap, buf_ne, first, count, nd, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    rec = M.pack_ref(hbuf, hne, first, count, nd)
    np.testing.assert_array_equal(out.cpu().numpy(), np.concatenate([rec.ravel(), np.full(GUARD, SENTINEL)]))

    def received(call):
        """the receiving population after `call`, and the (count, nd) rows it appended"""
        recv = TwoSpecies(nd, LIVE, pad=count + 9)
        assert call(recv.pop) == 0
        torch.cuda.synchronize()
        x, v = recv.state()
        dst = slice(START1 + LIVE, START1 + LIVE + count)
        gx, gv = x[:, dst].T.copy(), v[:, dst].T.copy()
        x[:, dst], v[:, dst] = recv.hx[:, dst], recv.hv[:, dst]
        np.testing.assert_array_equal(x, recv.hx)          # nothing before dst or behind dst + count
        np.testing.assert_array_equal(v, recv.hv)
        return gx, gv

    # import, for every mask
    for mask in range(1 << nd):
        gx, gv = received(lambda pop: hip.pinc_hip_import(pop, 1, LIVE, buf, work.cap, buf_ne, first, count,
                                                          shift_t, mask, None))
        wx, wv = M.import_ref(hbuf, hne, first, count, nd, SHIFT_T, mask)
        np.testing.assert_array_equal(gx, wx)
        np.testing.assert_array_equal(gv, wv)
    # import of the packed records: the full mask, bit for bit
    rx, rv = received(lambda pop: hip.pinc_hip_import_rec(pop, 1, LIVE, out.data_ptr(), count, shift_t, None))
    wx, wv = M.import_rec_ref(rec, nd, SHIFT_T)
    np.testing.assert_array_equal(rx, wx)
    np.testing.assert_array_equal(rv, wv)
    np.testing.assert_array_equal(rx, gx)
    np.testing.assert_array_equal(rv, gv)
    assert work.broken_guards() == []
