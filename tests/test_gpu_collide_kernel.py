"""pinc_hip_collide called directly (ctypes, tests/push_abi.py) against the
long-double restatement of its rule, tests/collide_ref.py.

Checks of every case (collide_ref.check and _check below):
  * both counters are exactly the reference's; every particle the reference
    does not collide is bit-identical to the input, and so are all positions
    and every slot outside the species.  In 2-D and 3-D the particles whose
    bits changed are exactly the reference's colliders (in 1-D an elastic
    collision with e = +1 and w > n gives w' = w: a collider may keep its bits);
  * a collider's components are within
        |v' - v'_ref| h_d <= 64 eps (sum|w_d| + sum|n_d| + g)
    of the reference's outcome for its process (a few terms, each a product of
    log, sqrt and sin/cos results of <= 2 ulp, and the angle's rounding), so a
    collider that took the other process would show;
  * a decision may differ from the reference only where the reference's own
    margin is below 1e-12; the cap on such cases is zero, and the seeds are
    chosen so that the smallest margin of every case is above 1e-9
    (tests/test_collide_ref_cpu.py::test_reference_margins, in the CPU suite).

Cases: the smallest at which each path exists (the chunk is read from the
library): n = 0, 1, 3, chunk - 1, chunk, chunk + 1; each process alone and
both, by rate and by cross section (with a warm, drifting background);
everyone and no one colliding; species 1 of 2 at an odd iStart; 2-D and 1-D;
the sizes, the odd starts (with even and odd counts) and the two-species case
also with cross sections, whose instance alone reads 16-B pairs;
h != 1; velocity arrays other than pop.v; two launches into one pair of
counters; two keys.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import collide_ref as CR
from collide_abi import CollideT, params_t
from push_abi import SENTINEL, DevSpecies, Pop

pytestmark = pytest.mark.gpu



def chunk() -> int:
    """particles per workgroup of pinc_hip_collide, from the library"""
    from pinc_amd import _lib
    f = _lib.HIP.pinc_hip_collide_chunk
    f.restype = C.c_long
    return int(f())


BOTH = CR.Params(nu=(0.04, 0.06), b=28.0 / 29.0, vth=0.03, drift=(0.01, -0.02, 0.005))
# the same with cross sections: the instance that reads 16-B pairs (single
# loads at an odd head and at a partial last pair)
BOTH_SIG = CR.Params(nu=(0.04, 0.06), sig=(0.2, 0.3), b=28.0 / 29.0, vth=0.03, drift=(0.01, -0.02, 0.005))
SIGMA = CR.Params(sig=(0.4, 0.7), b=0.8, vth=0.04, drift=(0.05, 0.02, -0.03))
CASES = {
    # name: (nd, n or ("chunk", k) for the library's chunk + k, seed of the velocities, parameters, key)
    "n1": (3, 1, 101, CR.Params(nu=(30.0, 10.0), b=0.5, vth=0.02), CR.key(1, 0, 0, 0)),
    "n3": (3, 3, 102, CR.Params(nu=(1.0, 1.0), b=0.5, vth=0.02), CR.key(1, 1, 0, 0)),
    "chunk-1": (3, ("chunk", -1), 103, BOTH, CR.key(2, 0, 0, 0)),
    "chunk": (3, ("chunk", 0), 104, BOTH, CR.key(2, 1, 0, 0)),
    "chunk+1": (3, ("chunk", 1), 105, BOTH, CR.key(2, 2, 0, 0)),
    "n1 sig": (3, 1, 121, CR.Params(nu=(30.0, 10.0), sig=(0.5, 0.5), b=0.5, vth=0.02), CR.key(8, 0, 0, 0)),
    "n3 sig": (3, 3, 122, CR.Params(nu=(1.0, 1.0), sig=(0.5, 0.5), b=0.5, vth=0.02), CR.key(8, 1, 0, 0)),
    "chunk-1 sig": (3, ("chunk", -1), 123, BOTH_SIG, CR.key(8, 2, 0, 0)),
    "chunk sig": (3, ("chunk", 0), 124, BOTH_SIG, CR.key(8, 3, 0, 0)),
    "chunk+1 sig": (3, ("chunk", 1), 125, BOTH_SIG, CR.key(8, 4, 0, 0)),
    "sigma odd": (3, 4999, 126, SIGMA, CR.key(8, 5, 0, 0)),
    "2d odd": (2, 4999, 127, CR.Params(nu=(0.05, 0.05), sig=(0.1, 0.1), b=0.9, vth=0.03, drift=(0.02, 0.01, 0.0)),
               CR.key(8, 6, 0, 0)),
    "1d odd": (1, 4999, 128, CR.Params(nu=(0.08, 0.04), sig=(0.2, 0.0), b=0.7, vth=0.03, drift=(0.02, 0.0, 0.0)),
               CR.key(8, 7, 0, 0)),
    "elastic": (3, 5000, 106, CR.Params(nu=(0.1, 0.0), b=0.3, vth=0.05), CR.key(3, 0, 0, 0)),
    "cex": (3, 5000, 107, CR.Params(nu=(0.0, 0.1), vth=0.05, drift=(0.1, 0.0, 0.0)), CR.key(3, 1, 0, 0)),
    "both": (3, 5000, 108, BOTH, CR.key(3, 2, 0, 0)),
    "sigma": (3, 5000, 109, SIGMA, CR.key(4, 0, 0, 0)),
    "mixed": (3, 5000, 110, CR.Params(nu=(0.02, 0.0), sig=(0.0, 0.5), b=0.6, vth=0.04), CR.key(4, 1, 0, 0)),
    "everyone": (3, 5000, 111, CR.Params(nu=(25.0, 15.0), b=0.5, vth=0.05), CR.key(5, 0, 0, 0)),
    "no one": (3, 5000, 112, CR.Params(vth=0.05), CR.key(5, 1, 0, 0)),
    "2d": (2, 5000, 113, CR.Params(nu=(0.05, 0.05), sig=(0.1, 0.1), b=0.9, vth=0.03, drift=(0.02, 0.01, 0.0)),
           CR.key(6, 0, 0, 0)),
    "1d": (1, 5000, 114, CR.Params(nu=(0.08, 0.04), sig=(0.2, 0.0), b=0.7, vth=0.03, drift=(0.02, 0.0, 0.0)),
           CR.key(6, 1, 0, 0)),
    "h": (3, 5000, 115, CR.Params(nu=(0.06, 0.05), sig=(0.1, 0.1), b=0.5, vth=0.03, h=(1.0, 2.5, 1.0)),
          CR.key(7, 0, 0, 0)),
    "second": (3, 5000, 108, BOTH, CR.key(3, 3, 0, 0)),       # "both" again under the next step's key
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(pos, vel, parameters, key, reference): made once, shared, never modified"""
    nd, n, seed, par, key = CASES[name]
    if isinstance(n, tuple):
        n = chunk() + n[1]
    rng = np.random.default_rng(seed)
    pos = 1.0 + 6.0 * rng.random((n, nd))
    vel = 0.2 * rng.standard_normal((n, nd))
    for a in (pos, vel):
        a.setflags(write=False)
    return pos, vel, par, key, CR.collide(vel, par, key)


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available()
    from pinc_amd import _lib
    h = _lib.HIP
    vp = C.c_void_p
    h.pinc_hip_collide.argtypes = [Pop, C.c_int, C.POINTER(vp), CollideT, vp, vp]
    h.pinc_hip_collide_chunk.restype = C.c_long
    h.pinc_hip_error_string.restype = C.c_char_p
    assert h.pinc_hip_collide_chunk() >= 64
    return h


def launch(hip, sp, par, key, *, s=0, vs=None, counts=None):
    """one pinc_hip_collide of species s of sp; returns (velocities of the
    live range after it, [elastic, cex] counters, the counter tensor)"""
    import torch
    if counts is None:
        counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    vs = sp.vs if vs is None else vs
    rc = hip.pinc_hip_collide(sp.pop, s, sp.ptrs(vs), params_t(par, key), counts.data_ptr(), None)
    assert rc == 0, hip.pinc_hip_error_string()
    torch.cuda.synchronize()
    return sp.live(vs), counts.cpu().numpy().tolist(), counts


def _check(got, cnt, vel, res, par, what, exact_set=True):
    assert cnt == list(res.counts), (what, cnt, res.counts)
    ratio = CR.check(got, vel, res, par, what)
    if exact_set and len(vel):
        changed = np.any(got.view(np.uint64) != np.ascontiguousarray(vel).view(np.uint64), axis=1)
        np.testing.assert_array_equal(changed, res.proc >= 0, err_msg=what)
    return ratio


def run_case(hip, name, start=0):
    pos, vel, par, key, res = case(name)
    sp = DevSpecies(pos, vel, start=start)
    got, cnt, _ = launch(hip, sp, par, key)
    ratio = _check(got, cnt, vel, res, par, name, exact_set=vel.shape[1] > 1)
    np.testing.assert_array_equal(sp.live(sp.xs), pos)
    assert sp.padding_untouched(sp.xs) and sp.padding_untouched(sp.vs)
    return ratio, res


def test_empty_species(hip):
    import torch
    pos, vel, par, key, _ = case("n3")
    sp = DevSpecies(pos, vel)
    sp.pop.iStop = (C.c_long * 8)(sp.start)
    got, cnt, _ = launch(hip, sp, par, key)
    assert cnt == [0, 0]
    assert np.array_equal(sp.live(sp.vs), vel)
    torch.cuda.synchronize()


@pytest.mark.parametrize("sig", ["", " sig"])
@pytest.mark.parametrize("name,start", [("n1", 0), ("n1", 1), ("n3", 0), ("n3", 1), ("chunk-1", 0), ("chunk-1", 1),
                                        ("chunk", 0), ("chunk", 1), ("chunk+1", 0), ("chunk+1", 3)])
def test_sizes_around_a_chunk(hip, name, start, sig):
    """rates alone (the two-pass instance) and with cross sections (the
    instance that reads pairs): even and odd iStart, even and odd ends"""
    run_case(hip, name + sig, start)


@pytest.mark.parametrize("name", ["sigma", "mixed", "sigma odd", "2d", "2d odd", "1d", "1d odd", "h"])
@pytest.mark.parametrize("start", [1, 3])
def test_pair_loads_at_odd_starts(hip, name, start):
    """the cross-section instance's head and tail: an odd iStart (the first
    particle is the upper half of a pair) with an even and with an odd count"""
    run_case(hip, name, start)


@pytest.mark.parametrize("name", ["elastic", "cex", "both", "sigma", "mixed", "2d", "1d", "h"])
def test_processes_modes_and_dimensions(hip, name):
    ratio, res = run_case(hip, name, start=2)
    nel, ncx = res.counts
    want = {"elastic": (True, False), "cex": (False, True)}.get(name, (True, True))
    assert (nel > 0, ncx > 0) == want, (nel, ncx)


def test_everyone_and_no_one(hip):
    _, res = run_case(hip, "everyone")
    assert sum(res.counts) == 5000
    pos, vel, par, key, res = case("no one")
    sp = DevSpecies(pos, vel, start=1)
    got, cnt, _ = launch(hip, sp, par, key)
    assert cnt == [0, 0] and sum(res.counts) == 0
    assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(vel).view(np.uint64))


@pytest.mark.parametrize("name", ["both", "sigma", "sigma odd"])
def test_second_species_at_an_odd_start(hip, name):
    pos, vel, par, key, res = case(name)
    sp = DevSpecies(pos, vel, start=1001, pad=7)
    # species 1 of 2: species 0 is [0, 1001), live, every slot SENTINEL
    sp.pop.nSpecies = 2
    sp.pop.iStart = (C.c_long * 9)(0, sp.start, sp.cap)
    sp.pop.iStop = (C.c_long * 8)(sp.start, sp.start + sp.n)
    got, cnt, _ = launch(hip, sp, par, key, s=1)
    _check(got, cnt, vel, res, par, f"species 1 at an odd start, {name}")
    assert sp.padding_untouched(sp.xs) and sp.padding_untouched(sp.vs)
    np.testing.assert_array_equal(sp.live(sp.xs), pos)


def test_writes_the_velocity_arrays_it_is_given(hip):
    pos, vel, par, key, res = case("both")
    sp = DevSpecies(pos, np.full_like(vel, SENTINEL), start=5)
    other = DevSpecies(pos, vel, start=5)      # same ranges: indexed like pop.v
    got, cnt, _ = launch(hip, sp, par, key, vs=other.vs)
    _check(got, cnt, vel, res, par, "separate velocity arrays")
    assert np.all(sp.live(sp.vs) == SENTINEL) and other.padding_untouched(other.vs)


def test_two_launches_accumulate_and_two_keys_differ(hip):
    pos, vel, par, key, res = case("both")
    _, _, _, key2, res2 = case("second")
    assert key2 != key
    sp = DevSpecies(pos, vel)
    got, cnt, counts = launch(hip, sp, par, key)
    _check(got, cnt, vel, res, par, "first launch")
    # the same velocities under another key: other colliders
    sp2 = DevSpecies(pos, vel)
    got2, cnt2, _ = launch(hip, sp2, par, key2, counts=counts)
    assert cnt2 == [res.counts[0] + res2.counts[0], res.counts[1] + res2.counts[1]]
    ch1 = np.any(got != vel, axis=1)
    ch2 = np.any(got2 != vel, axis=1)
    np.testing.assert_array_equal(ch2, res2.proc >= 0)
    assert np.any(ch1 != ch2) and 0 < np.sum(ch1 & ch2) < min(ch1.sum(), ch2.sum())


def test_bad_arguments_are_refused(hip):
    import torch
    pos, vel, par, key, _ = case("n3")
    sp = DevSpecies(pos, vel)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    bad = [CR.Params(nu=(-0.1, 0.0)), CR.Params(sig=(0.0, float("nan"))), CR.Params(nu=(0.1, 0.0), b=1.5),
           CR.Params(nu=(0.1, 0.0), h=(1.0, 0.0, 1.0)), CR.Params(nu=(0.1, 0.0), vth=-1.0)]
    for p in bad:
        assert hip.pinc_hip_collide(sp.pop, 0, sp.ptrs(sp.vs), params_t(p, key), counts.data_ptr(), None) != 0
        assert b"collide" in hip.pinc_hip_error_string()
    assert hip.pinc_hip_collide(sp.pop, 3, sp.ptrs(sp.vs), params_t(par, key), counts.data_ptr(), None) != 0
    assert hip.pinc_hip_collide(sp.pop, 0, sp.ptrs(sp.vs), params_t(par, key), None, None) != 0
    torch.cuda.synchronize()
    assert counts.cpu().numpy().tolist() == [0, 0] and np.array_equal(sp.live(sp.vs), vel)
