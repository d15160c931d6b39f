"""pinc_hip_rho_combine, pinc_hip_field_chain_all (with pinc_hip_field_chain)
and pinc_hip_vel_assert called through the C ABI, against tests/glue_ref.py.

The two chains are bit for bit: each is a fixed sequence of IEEE
multiplications and additions (no fused multiply-add in the library),

    rho:  r = acc[0]; r = (r q[s-1]) (1.0 / q[s]) + acc[s]; rho = r q[ns-1]
    Es_s: v = E pre; Es_0 = v qm[0]; v = (v qm[s-1]) mq[s-1]; Es_s = v qm[s]

with charges and masses that are no powers of two, so that another order of
the multiplications gives other bits (tests/test_glue_ref_cpu.py).  ns in
{1, 2, 3, 8}, n in {1, 1023}, and at ns = 3 n = 8192 * 256 + 5 (every thread
strides) and n = 8192 * 1024 + 5 (past the launch cap of 8192 blocks).
Outputs are pre-filled with NaN between guards; inputs come back unchanged.

The velocity assert sets bit 0 of a word, or leaves the word alone: signed
and strict, as the reference's pVelAssertMax (population.c:342-365: `vel >
max`, no magnitude).  Exact.
"""
import ctypes as C

import numpy as np
import pytest

import glue_ref as G
from gpu_buf import Buf, IntBuf, same_bits
from push_abi import SENTINEL, Pop

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available()
    from pinc_amd import _lib
    h = _lib.HIP
    vp, ci, cl, cd = C.c_void_p, C.c_int, C.c_long, C.c_double
    h.pinc_hip_rho_combine.argtypes = [vp, C.POINTER(vp), C.POINTER(cd), ci, cl, vp]
    h.pinc_hip_field_chain_all.argtypes = [vp, vp, cl, vp, vp, cd, ci, vp]
    h.pinc_hip_field_chain.argtypes = [vp, vp, cl, vp, vp, cd, ci, vp]
    h.pinc_hip_vel_assert.argtypes = [Pop, ci, cd, vp, vp]
    return h


def assert_bits(got, want):
    assert got.shape == want.shape
    if not same_bits(got, want):
        np.testing.assert_array_equal(got, want)  # says where
        raise AssertionError("equal values, other bits (a zero's sign)")


# ------------------------------------------------------------ rho_combine ---
def combine(hip, accs, q, ns, n, rho):
    ptrs = (C.c_void_p * max(ns, 1))(*[a.ptr for a in accs[:max(ns, 1)]])
    return hip.pinc_hip_rho_combine(rho.ptr, ptrs, (C.c_double * len(q))(*q), ns, n, None)


@pytest.mark.parametrize("case", G.CHAIN_CASES, ids=G.chain_id)
def test_rho_combine(hip, case):
    """bit for bit; the accumulators unchanged"""
    ns, n = case
    c = G.chain_inputs(ns, n)
    accs = [Buf(c.acc[s]) for s in range(ns)]
    rho = Buf(np.full(n, np.nan))
    assert combine(hip, accs, c.q, ns, n, rho) == 0
    assert_bits(rho.get(), G.rho_combine(c.acc, c.q))
    assert all(a.unchanged() for a in accs)


def test_rho_combine_arguments(hip):
    """ns = 0 and ns = 9 are refused; n = 0 returns 0; nothing is written"""
    c = G.chain_inputs(8, 64)
    accs = [Buf(c.acc[s]) for s in range(8)]
    rho = Buf(np.full(64, np.nan))
    assert combine(hip, accs, c.q, 0, 64, rho) != 0
    assert b"rho_combine" in hip.pinc_hip_error_string()
    assert combine(hip, accs, c.q, 9, 64, rho) != 0
    assert rho.unchanged()
    for ns in (1, 3, 8):
        assert combine(hip, accs, c.q, ns, 0, rho) == 0
    assert rho.unchanged() and all(a.unchanged() for a in accs)


# ------------------------------------------------------- field_chain_all ---
@pytest.mark.parametrize("pre", G.CHAIN_PRE)
@pytest.mark.parametrize("case", G.CHAIN_CASES, ids=G.chain_id)
def test_field_chain_all(hip, case, pre):
    """every species' Es bit for bit against the numpy chain, and against
    what pinc_hip_field_chain(..., s) writes on the same inputs"""
    ns, n = case
    c = G.chain_inputs(ns, n)
    E, qm, mq = Buf(c.E), Buf(c.qm), Buf(c.mq)
    Es = Buf(np.full((ns, n), np.nan))
    assert hip.pinc_hip_field_chain_all(E.ptr, Es.ptr, n, qm.ptr, mq.ptr, pre, ns, None) == 0
    got = Es.get()
    assert_bits(got, G.field_chain_all(c.E, c.qm, c.mq, pre))
    for s in range(ns):
        one = Buf(np.full(n, np.nan))
        assert hip.pinc_hip_field_chain(E.ptr, one.ptr, n, qm.ptr, mq.ptr, pre, s, None) == 0
        assert_bits(one.get(), got[s])
    assert E.unchanged() and qm.unchanged() and mq.unchanged()


def test_field_chain_all_arguments(hip):
    c = G.chain_inputs(8, 64)
    E, qm, mq = Buf(c.E), Buf(c.qm), Buf(c.mq)
    Es = Buf(np.full((8, 64), np.nan))
    assert hip.pinc_hip_field_chain_all(E.ptr, Es.ptr, 64, qm.ptr, mq.ptr, 1.0, 0, None) != 0
    assert b"field_chain_all" in hip.pinc_hip_error_string()
    assert hip.pinc_hip_field_chain_all(E.ptr, Es.ptr, 64, qm.ptr, mq.ptr, 1.0, 9, None) != 0
    for args in ((None, Es.ptr, qm.ptr, mq.ptr), (E.ptr, None, qm.ptr, mq.ptr), (E.ptr, Es.ptr, None, mq.ptr),
                 (E.ptr, Es.ptr, qm.ptr, None)):
        e, es, a, b = args
        assert hip.pinc_hip_field_chain_all(e, es, 64, a, b, 1.0, 3, None) != 0
    assert hip.pinc_hip_field_chain_all(E.ptr, Es.ptr, 0, qm.ptr, mq.ptr, 1.0, 3, None) == 0
    assert Es.unchanged() and E.unchanged()


# ------------------------------------------------------- velocity assert ---
def flag_word(hip, pop, word):
    err = IntBuf(np.array([word], dtype=np.int32))
    assert hip.pinc_hip_vel_assert(pop, 1, G.MAX_VEL, err.ptr, None) == 0
    return int(err.get()[0])


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_vel_assert(hip, nd):
    """A component at maxVel exactly, or at -10 maxVel, leaves the word alone
    (0 stays 0, 6 stays 6); one at nextafter above maxVel sets bit 0 (6
    becomes 7): at the first slot, at the last, in each dimension in turn.
    The same offender in slot iStart - 1 or iStop does not flag."""
    for name, vel, bad in G.vel_cases(nd):
        sp = G.species_1_of_2(np.zeros_like(vel), vel)
        for word in (0, 6):
            assert flag_word(hip, sp.pop, word) == G.vel_assert(vel, G.MAX_VEL, word) == word + int(bad), name
        np.testing.assert_array_equal(sp.live(sp.vs), vel)
        assert sp.padding_untouched(sp.vs)
    _, vel, _ = G.vel_cases(nd)[0]
    above = float(np.nextafter(G.MAX_VEL, 2.0))
    for slot in (G.START - 1, G.START + len(vel)):
        for d in range(nd):
            sp = G.species_1_of_2(np.zeros_like(vel), vel)
            sp.vs[d][slot] = above
            assert flag_word(hip, sp.pop, 6) == 6, (slot, d)
            sp.vs[d][G.START if slot < G.START else slot - 1] = above      # and just inside it does
            assert flag_word(hip, sp.pop, 6) == 7, (slot, d)


@pytest.mark.parametrize("n", [G.VEL_N_STRIDE, G.VEL_N_CAP], ids=["stride", "cap"])
def test_vel_assert_last_slot_of_a_large_species(hip, n):
    """1-D species of 16384 * 256 + 3 particles (the grid stride) and of
    16384 * 2048 + 3 (past the launch cap of 16384 blocks of 8 x 256): the
    single offender in the last slot"""
    import torch
    start = G.START
    v = torch.full((start + n + 7,), SENTINEL, dtype=torch.float64, device="cuda")
    v[start:start + n] = G.MAX_VEL
    v[start - 1] = 2.0
    v[start + n] = 2.0
    pop = Pop((C.c_void_p * 3)(), (C.c_void_p * 3)(v.data_ptr(), None, None), 2, 1,
              (C.c_long * 9)(0, start, start + n + 7), (C.c_long * 8)(start, start + n))
    assert flag_word(hip, pop, 6) == 6
    v[start + n - 1] = float(np.nextafter(G.MAX_VEL, 2.0))
    assert flag_word(hip, pop, 6) == 7
    assert flag_word(hip, pop, 0) == 1


def test_vel_assert_of_no_particles(hip):
    _, vel, _ = G.vel_cases(2)[4]
    sp = G.species_1_of_2(np.zeros_like(vel), np.full_like(vel, 5.0))
    sp.pop.iStop[1] = sp.pop.iStart[1]
    assert flag_word(hip, sp.pop, 6) == 6
