"""tests/ionize_ref.py itself (no GPU): the key, the energy identity of the
rule's step 6, the directions and the energy share of the two electrons, the
birth order, and the decision margins of the GPU cases."""
import ctypes as C

import numpy as np
import pytest

import collide_ref as CR
import ionize_ref as IR

LD = IR.LD


def _vel(n, nd, seed, scale=0.3):
    return scale * np.random.default_rng(seed).standard_normal((n, nd))


def test_key_differs_from_the_collide_key_and_equals_the_library(built):
    from pinc_amd import _lib
    f = _lib.HIP.pinc_hip_ionize_key
    f.restype = C.c_ulonglong
    f.argtypes = [C.c_ulonglong, C.c_ulonglong, C.c_int, C.c_int]
    cases = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (12345, 678, 3, 7),
             ((1 << 64) - 1, (1 << 40) + 5, 1023, 2)]
    keys = [IR.key(*c) for c in cases]
    for c, k in zip(cases, keys):
        assert f(*c) == k, c
        assert k != CR.key(*c)
        assert k == int(CR.mix64(np.uint64(CR.key(*c) ^ 0x696F6E697365)))
    assert len(set(keys) | {CR.key(*c) for c in cases}) == 2 * len(cases)


@pytest.mark.parametrize("nd", [1, 2, 3])
@pytest.mark.parametrize("sig", [0.0, 0.8])
def test_energy_identity(nd, sig):
    """in the neutral's frame |w' - n|^2 + |w_new - n|^2 = G - W, the ion is the
    neutral, and nobody below the threshold ionises"""
    par = IR.Params(nu=0.7, sig=sig, wth=0.3, vth=0.06, drift=(0.02, -0.01, 0.03), h=(1.0, 1.25, 0.5))
    vel = _vel(5000, nd, 30 + nd)
    res = IR.ionize(vel, par, IR.key(3, 0, 0, 0))
    assert 100 < res.births < 4000
    h = np.array(par.h[:nd], dtype=LD)
    p = res.parents
    n, G, W = res.extra["n"][p], res.extra["G"][p], res.extra["W"]
    assert np.all(G > W)
    a = np.sum((res.vel[p] * h - n) ** 2, axis=1)
    b = np.sum((res.electrons * h - n) ** 2, axis=1)
    assert float(np.max(np.abs(a + b - (G - W)) / G)) <= 1e-15
    assert float(np.max(np.abs(res.ions * h - n))) <= 1e-17
    # the particles that did not ionise keep their velocity, and the births are in index order
    assert np.array_equal(res.vel[~res.hit], vel[~res.hit].astype(LD))
    assert np.all(np.diff(p) > 0) and len(res.electrons) == len(res.ions) == res.births


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_isotropy_and_an_even_energy_share(nd):
    """over 1e5 births: both unit vectors have zero mean and <e_d^2> = 1 / nd,
    and the share f has mean 1/2 (uniform: variance 1/12), all within 5 sigma"""
    N = 100000
    par = IR.Params(nu=40.0, wth=0.0, vth=0.05)
    res = IR.ionize(_vel(N, nd, 40 + nd), par, IR.key(4, 1, 0, 0))
    assert res.births == N
    f = res.extra["f"].astype(np.float64)
    assert abs(f.mean() - 0.5) <= 5 / np.sqrt(12 * N)
    for e in (res.extra["e1"], res.extra["e2"]):
        e = e.astype(np.float64)
        assert np.max(np.abs(np.sum(e * e, axis=1) - 1)) <= 1e-15
        for d in range(nd):
            assert abs(e[:, d].mean()) <= 5 * np.sqrt(1.0 / nd / N), (nd, d)
            # Var(e_d^2): 4/45 in 3-D (e_d uniform on [-1, 1]), 1/8 in 2-D, 0 in 1-D
            var2 = {3: 4.0 / 45.0, 2: 1.0 / 8.0, 1: 0.0}[nd]
            assert abs(np.mean(e[:, d] ** 2) - 1.0 / nd) <= 5 * np.sqrt(var2 / N) + 1e-15
    # the two directions are independent draws
    c = np.sum(res.extra["e1"] * res.extra["e2"], axis=1).astype(np.float64)
    assert abs(c.mean()) <= 5 * np.sqrt(1.0 / nd / N)


def test_ionised_count_is_binomial_above_the_threshold():
    N = 100000
    par = IR.Params(nu=0.05, wth=0.4)
    res = IR.ionize(_vel(N, 3, 50), par, IR.key(5, 0, 0, 0))
    fast = int(np.sum(res.extra["G"] > res.extra["W"]))
    P = -np.expm1(-0.05)
    assert 0.2 * N < fast < 0.8 * N
    assert abs(res.births - fast * P) <= 5 * np.sqrt(fast * P * (1 - P))


def test_reference_margins(built):
    """no decision of any case of tests/test_gpu_ionize_kernel.py is within 1e-9
    of either threshold (|G - W| / max(G, W), |u0 - P|): the kernel's fp64
    decisions cannot differ from the long-double reference's there, and the
    share of particles a GPU test may leave undecided is zero.  And every
    ioniser keeps (G - W) / G >= 1e-2, where sqrt(G - W) is conditioned well
    enough for the GPU tests' bound (the reasoning is in that file)."""
    import test_gpu_ionize_kernel as K
    refs = {name: K.case(name)[4] for name in K.CASES}
    worst = min(IR.min_margin(r) for r in refs.values())
    share = min(IR.min_rem_share(r) for r in refs.values())
    print(f"smallest decision margin over all cases: {worst:.3e}; smallest (G - W) / G of an ioniser: {share:.3e}")
    assert worst > 1e-9
    assert share >= 1e-2
