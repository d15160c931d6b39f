"""pinc_hip_ionize called directly (ctypes, tests/push_abi.py and
tests/ionize_abi.py) against the long-double restatement of its rule,
tests/ionize_ref.py.

Checks of every case (_verify):
  * res[0] is exactly the reference's number of births, res[1] stays 0;
  * the parents whose bits changed are exactly the reference's ionisers;
  * the children sit at the reference's slots in its order: birth k (ascending
    parent index) at iStop[s] + k and iStop[target] + k, their positions
    bit-identical to the parent's;
  * every other value of every array is bit-identical to what it was: the
    positions of existing particles, the particles that did not ionise, every
    slot outside [iStart, iStop + births) of both species (SENTINEL) and every
    other species;
  * each written velocity component is within 64 eps (sum|n_d| + g) / h_d of
    the reference (the collide test's bound with the terms this rule has).
    sqrt(G - W) loses digits as G nears W: G carries a few eps (sum|n_d| + g) g
    of rounding (the neutral's log and sincospi), so g1 and g2 carry that over
    2 sqrt(G - W), and the bound holds while (G - W) / G of the ionisers is
    not tiny.  The cases keep it above 1e-2 and every decision margin above
    1e-9 (tests/test_ionize_ref_cpu.py::test_reference_margins, CPU suite), so
    no decision may differ from the reference's.

Cases, with the chunk read from the library: n = 0, 1, 3, chunk - 1, chunk,
chunk + 1, 2 chunk + 1 (three workgroups, births in more than one), by rate alone and
with a cross section, at even and odd iStart; everyone (nu = 40, wth = 0), no
one (wth above every relative speed), a threshold that splits the population;
3-D, 2-D, 1-D; h != 1; the projectile as species 1 of 3 at an odd iStart with a
target whose iStop is odd; two launches into one res, two keys; free slots
exactly the births, and one fewer in either species; bad arguments.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ionize_ref as IR
from ionize_abi import bind, params_t
from push_abi import SENTINEL, Pop

pytestmark = pytest.mark.gpu

WARM = dict(vth=0.03, drift=(0.01, -0.02, 0.005))
RATE = IR.Params(nu=1.0, wth=0.1, **WARM)
RATE_SIG = IR.Params(nu=0.5, sig=2.0, wth=0.1, **WARM)
CASES = {
    # name: (nd, n or ("chunk", m, k) for m chunks + k, seed of the particles, parameters, key)
    # (the seeds: the first of seed, seed + 100, ... at which the reference's margins hold)
    "n1": (3, 1, 201, IR.Params(nu=40.0, vth=0.02), IR.key(1, 0, 0, 0)),
    "n3": (3, 3, 202, IR.Params(nu=1.0, wth=0.05, vth=0.02), IR.key(1, 1, 0, 0)),
    "chunk-1": (3, ("chunk", 1, -1), 303, RATE, IR.key(2, 0, 0, 0)),
    "chunk": (3, ("chunk", 1, 0), 304, RATE, IR.key(2, 1, 0, 0)),
    "chunk+1": (3, ("chunk", 1, 1), 305, RATE, IR.key(2, 2, 0, 0)),
    "2chunk+1": (3, ("chunk", 2, 1), 306, RATE, IR.key(2, 3, 0, 0)),
    "n1 sig": (3, 1, 211, IR.Params(nu=40.0, sig=1.0, vth=0.02), IR.key(3, 0, 0, 0)),
    "n3 sig": (3, 3, 212, IR.Params(nu=1.0, sig=1.0, wth=0.05, vth=0.02), IR.key(3, 1, 0, 0)),
    "chunk-1 sig": (3, ("chunk", 1, -1), 213, RATE_SIG, IR.key(4, 0, 0, 0)),
    "chunk sig": (3, ("chunk", 1, 0), 214, RATE_SIG, IR.key(4, 1, 0, 0)),
    "chunk+1 sig": (3, ("chunk", 1, 1), 315, RATE_SIG, IR.key(4, 2, 0, 0)),
    "2chunk+1 sig": (3, ("chunk", 2, 1), 416, RATE_SIG, IR.key(4, 3, 0, 0)),
    "everyone": (3, 5000, 221, IR.Params(nu=40.0, wth=0.0, **WARM), IR.key(5, 0, 0, 0)),
    "no one": (3, 5000, 222, IR.Params(nu=40.0, sig=1.0, wth=10.0, **WARM), IR.key(5, 1, 0, 0)),
    "no one rate": (3, 5000, 223, IR.Params(nu=40.0, wth=10.0, **WARM), IR.key(5, 2, 0, 0)),
    "split": (3, 5000, 924, IR.Params(nu=0.05, wth=0.35, **WARM), IR.key(6, 0, 0, 0)),
    "split sig": (3, 5000, 1225, IR.Params(sig=0.3, wth=0.35, **WARM), IR.key(6, 1, 0, 0)),
    "2d": (2, 5000, 826, IR.Params(nu=0.05, wth=0.25, **WARM), IR.key(7, 0, 0, 0)),
    "2d sig": (2, 4999, 627, IR.Params(nu=0.02, sig=0.2, wth=0.25, **WARM), IR.key(7, 1, 0, 0)),
    "1d": (1, 5000, 428, IR.Params(nu=0.05, wth=0.15, **WARM), IR.key(7, 2, 0, 0)),
    "1d sig": (1, 4999, 429, IR.Params(nu=0.02, sig=0.2, wth=0.15, **WARM), IR.key(7, 3, 0, 0)),
    "h": (3, 5000, 330, IR.Params(nu=0.05, wth=0.3, h=(1.0, 2.5, 0.5), **WARM), IR.key(8, 0, 0, 0)),
    "h sig": (3, 5000, 631, IR.Params(sig=0.3, wth=0.3, h=(1.0, 2.5, 0.5), **WARM), IR.key(8, 1, 0, 0)),
    "second": (3, 5000, 924, IR.Params(nu=0.05, wth=0.35, **WARM), IR.key(6, 2, 0, 0)),   # "split" under another key
}


def chunk() -> int:
    """particles per workgroup of pinc_hip_ionize, from the library"""
    from pinc_amd import _lib
    f = _lib.HIP.pinc_hip_ionize_chunk
    f.restype = C.c_long
    return int(f())


@functools.lru_cache(maxsize=None)
def case(name):
    """(pos, vel, parameters, key, reference): made once, shared, never modified"""
    nd, n, seed, par, key = CASES[name]
    if isinstance(n, tuple):
        n = n[1] * chunk() + n[2]
    rng = np.random.default_rng(seed)
    pos = 1.0 + 6.0 * rng.random((n, nd))
    vel = 0.2 * rng.standard_normal((n, nd))
    for a in (pos, vel):
        a.setflags(write=False)
    return pos, vel, par, key, IR.ionize(vel, par, key)


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available()
    from pinc_amd import _lib
    h = bind(_lib.HIP)
    assert h.pinc_hip_ionize_chunk() >= 64
    return h


class DevPop:
    """Species in shared SoA device arrays (torch memory): species q owns the
    slots [iStart[q], iStart[q + 1]) and its first slots hold the particles
    data[q] = (pos, vel); every other slot is SENTINEL."""

    def __init__(self, nd, first, slots, data):
        import torch
        self.nd, self.ns = nd, len(slots)
        self.iStart = [first]
        for c in slots:
            self.iStart.append(self.iStart[-1] + c)
        self.iStop = [self.iStart[q] + len(data[q][0]) for q in range(self.ns)]
        total = self.iStart[-1] + 5
        self.host = np.full((2, nd, total), SENTINEL)
        for q, (pos, vel) in enumerate(data):
            assert len(pos) <= slots[q]
            self.host[0, :, self.iStart[q]:self.iStop[q]] = np.asarray(pos).T
            self.host[1, :, self.iStart[q]:self.iStop[q]] = np.asarray(vel).T
        self.dev = torch.from_numpy(self.host).cuda()
        ptr = lambda a: (C.c_void_p * 3)(*([self.dev[a, d].data_ptr() for d in range(nd)] + [None] * (3 - nd)))
        self.pop = Pop(ptr(0), ptr(1), self.ns, nd, (C.c_long * 9)(*self.iStart), (C.c_long * 8)(*self.iStop))

    def read(self):
        return self.dev.cpu().numpy()


def _others(n, nd, seed):
    rng = np.random.default_rng(seed)
    return 2.0 + rng.random((n, nd)), 0.01 * rng.standard_normal((n, nd))


def launch(hip, dp, s, par, key, res=None, work_ints=None):
    import torch
    if res is None:
        res = torch.zeros(2, dtype=torch.int64, device="cuda")
    need = hip.pinc_hip_ionize_work(dp.iStop[s] - dp.iStart[s])
    work = torch.full((need + 3,), -1, dtype=torch.int32, device="cuda")
    rc = hip.pinc_hip_ionize(dp.pop, s, params_t(par, key), work.data_ptr(), need if work_ints is None else work_ints,
                             res.data_ptr(), None)
    torch.cuda.synchronize()
    assert work[need:].cpu().tolist() == [-1, -1, -1]     # the scratch asked for is the scratch used
    return rc, res


def _verify(dp, got, s, par, pos, vel, ref, what):
    """the arrays `got` after one launch over dp (as built: dp.host) against the reference"""
    nd, t, nb = dp.nd, par.target, ref.births
    a, n = dp.iStart[s], len(vel)
    allowed = np.zeros(dp.host.shape, dtype=bool)
    allowed[1, :, a + ref.parents] = True
    for q in (s, t):
        allowed[:, :, dp.iStop[q]:dp.iStop[q] + nb] = True
    same = got.view(np.uint64) == dp.host.view(np.uint64)
    assert np.all(same | allowed), f"{what}: {int(np.sum(~same & ~allowed))} values outside the births were written"
    changed = np.any(~same[1, :, a:a + n], axis=0)
    np.testing.assert_array_equal(changed, ref.hit, err_msg=f"{what}: the parents that were written")
    if nb == 0:
        return 0.0
    bound = IR.bound(ref, par, nd)
    ratio = 0.0
    for q, want in ((s, ref.electrons), (t, ref.ions)):
        kids = got[:, :, dp.iStop[q]:dp.iStop[q] + nb]
        assert np.array_equal(kids[0].T.view(np.uint64), np.ascontiguousarray(pos[ref.parents]).view(np.uint64)), \
            f"{what}: positions of the children of species {q}"
        ratio = max(ratio, float(np.max(np.abs(kids[1].T.astype(IR.LD) - want) / bound)))
    newv = got[1, :, a:a + n].T[ref.parents]
    ratio = max(ratio, float(np.max(np.abs(newv.astype(IR.LD) - ref.vel[ref.parents]) / bound)))
    print(f"{what}: {nb} births of {n}, largest error / bound = {ratio:.4f}")
    assert ratio <= 1.0, f"{what}: error {ratio:.3f} of the bound"
    return ratio


def run_case(hip, name, first=0, free=(3, 3), three=False):
    """one launch of a case: the projectile as species 0 of 2 with the target
    behind it, or (three) as species 1 of 3 at an odd iStart with the target,
    species 2, ending at an odd iStop; free[k] slots more than the births"""
    pos, vel, par, key, ref = case(name)
    nd, n, nb = pos.shape[1], len(pos), ref.births
    if three:
        lead = _others(11, nd, 1)
        nt = 6
        slots = [13 - first, n + nb + free[0], nt + nb + free[1]]
        if (first + sum(slots[:2]) + nt) % 2 == 0:
            nt += 1
            slots[2] += 1
        dp = DevPop(nd, first, slots, [lead, (pos, vel), _others(nt, nd, 2)])
        s, par = 1, IR.Params(**{**par.__dict__, "target": 2})
        assert dp.iStart[1] % 2 == 1 and dp.iStop[2] % 2 == 1
    else:
        dp = DevPop(nd, first, [n + nb + free[0], 5 + nb + free[1]], [(pos, vel), _others(5, nd, 2)])
        s = 0
    rc, res = launch(hip, dp, s, par, key)
    assert rc == 0, hip.pinc_hip_error_string()
    assert res.cpu().tolist() == [nb, 0], (name, res.cpu().tolist(), nb)
    _verify(dp, dp.read(), s, par, pos, vel, ref, name)
    return ref


def test_empty_species(hip):
    pos, vel, par, key, _ = case("n3")
    dp = DevPop(3, 0, [8, 8], [(pos[:0], vel[:0]), _others(5, 3, 2)])
    rc, res = launch(hip, dp, 0, par, key)
    assert rc == 0 and res.cpu().tolist() == [0, 0]
    assert np.array_equal(dp.read().view(np.uint64), dp.host.view(np.uint64))


@pytest.mark.parametrize("sig", ["", " sig"])
@pytest.mark.parametrize("name,first", [("n1", 0), ("n1", 1), ("n3", 0), ("n3", 1), ("chunk-1", 0), ("chunk-1", 1),
                                        ("chunk", 0), ("chunk", 1), ("chunk+1", 0), ("chunk+1", 3), ("2chunk+1", 0),
                                        ("2chunk+1", 1)])
def test_sizes_around_a_chunk(hip, name, first, sig):
    """by rate alone (candidates listed in LDS) and with a cross section; even
    and odd iStart; 2 chunk + 1 runs three workgroups with births in more than
    one, whose order the scan of the block counts gives"""
    ref = run_case(hip, name + sig, first)
    assert ref.births > 0
    if name == "2chunk+1":
        # (the third workgroup holds one or two particles: the first two must have births)
        block = (ref.parents + first % 2) // chunk()
        assert np.any(block == 0) and np.any(block == 1)


@pytest.mark.parametrize("name", ["split", "split sig", "2d", "2d sig", "1d", "1d sig", "h", "h sig"])
def test_thresholds_dimensions_and_spacings(hip, name):
    pos, vel, par, key, ref = case(name)
    G = ref.extra["G"]
    assert 0.05 < np.mean(G > ref.extra["W"]) < 0.95       # the threshold splits the population
    assert 0 < ref.births < np.sum(G > ref.extra["W"])     # and the draw the fast ones
    run_case(hip, name, first=2)


def test_everyone_and_no_one(hip):
    assert run_case(hip, "everyone").births == 5000
    assert run_case(hip, "no one", first=1).births == 0
    assert run_case(hip, "no one rate", first=1).births == 0


@pytest.mark.parametrize("name", ["split", "split sig", "2chunk+1", "2d sig", "1d"])
def test_species_1_of_3_at_an_odd_start(hip, name):
    run_case(hip, name, first=0, three=True)


def test_two_launches_accumulate_and_two_keys_differ(hip):
    pos, vel, par, key, ref = case("split")
    _, _, _, key2, ref2 = case("second")
    assert key2 != key
    make = lambda: DevPop(3, 0, [len(pos) + 500, 505], [(pos, vel), _others(5, 3, 2)])
    dp = make()
    rc, res = launch(hip, dp, 0, par, key)
    assert rc == 0 and res.cpu().tolist() == [ref.births, 0]
    _verify(dp, dp.read(), 0, par, pos, vel, ref, "first launch")
    dp2 = make()
    rc, res = launch(hip, dp2, 0, par, key2, res=res)
    assert rc == 0 and res.cpu().tolist() == [ref.births + ref2.births, 0]
    _verify(dp2, dp2.read(), 0, par, pos, vel, ref2, "the same particles under another key")
    both = np.sum(ref.hit & ref2.hit)
    assert np.any(ref.hit != ref2.hit) and both < min(ref.births, ref2.births)


@pytest.mark.parametrize("name", ["split", "split sig", "2chunk+1"])
def test_free_slots_exactly_the_births(hip, name):
    run_case(hip, name, free=(0, 0))


@pytest.mark.parametrize("name", ["split", "split sig", "2chunk+1"])
@pytest.mark.parametrize("short", [0, 1])
def test_one_slot_too_few_writes_nothing(hip, name, short):
    import torch
    pos, vel, par, key, ref = case(name)
    free = [ref.births + 2, ref.births + 2]
    free[short] = ref.births - 1
    dp = DevPop(3, 1, [len(pos) + free[0], 5 + free[1]], [(pos, vel), _others(5, 3, 2)])
    res = torch.tensor([17, 0], dtype=torch.int64, device="cuda")
    rc, res = launch(hip, dp, 0, par, key, res=res)
    assert rc == 0, hip.pinc_hip_error_string()
    assert res.cpu().tolist() == [17, 1]
    assert np.array_equal(dp.read().view(np.uint64), dp.host.view(np.uint64))


def test_bad_arguments_are_refused(hip):
    import torch
    pos, vel, par, key, _ = case("n3")
    dp = DevPop(3, 0, [10, 10], [(pos, vel), _others(5, 3, 2)])
    res = torch.zeros(2, dtype=torch.int64, device="cuda")
    work = torch.zeros(64, dtype=torch.int32, device="cuda")
    call = lambda p, s=0, pop=None, w=work.data_ptr(), wi=64, r=res.data_ptr(): hip.pinc_hip_ionize(
        pop or dp.pop, s, params_t(p, key), w, wi, r, None)
    nan, inf = float("nan"), float("inf")
    P = lambda **kw: IR.Params(**{**par.__dict__, **kw})
    bad = [P(nu=-0.1), P(nu=nan), P(sig=-1.0), P(sig=inf), P(wth=-0.1), P(wth=nan), P(vth=-1.0), P(vth=inf),
           P(drift=(0.0, nan, 0.0)), P(h=(1.0, 0.0, 1.0)), P(h=(1.0, 1.0, -2.0)), P(target=0), P(target=2), P(target=-1)]
    for p in bad:
        assert call(p) != 0, p
        assert b"ionize" in hip.pinc_hip_error_string()
    assert call(par, s=2) != 0 and call(par, s=-1) != 0
    assert call(par, w=None) != 0 and call(par, r=None) != 0
    assert call(par, wi=hip.pinc_hip_ionize_work(3) - 1) != 0
    for nd in (0, 4):
        pop = Pop.from_buffer_copy(dp.pop)
        pop.nd = nd
        assert call(par, pop=pop) != 0
    pop = Pop.from_buffer_copy(dp.pop)
    pop.v[1] = None
    assert call(par, pop=pop) != 0
    torch.cuda.synchronize()
    assert res.cpu().tolist() == [0, 0] and np.array_equal(dp.read().view(np.uint64), dp.host.view(np.uint64))
    assert call(par) == 0          # (the arguments were otherwise good)
    torch.cuda.synchronize()


def test_key_is_the_references(hip):
    for c in [(0, 0, 0, 0), (9, 4, 1, 1), ((1 << 64) - 1, 1 << 40, 7, 3)]:
        assert hip.pinc_hip_ionize_key(*c) == IR.key(*c)
