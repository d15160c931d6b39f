"""tests/collide_ref.py itself (no GPU): the key equals the library's, the
two processes conserve what they must, the collided count follows the
binomial law, and lazy draws change nothing."""
import ctypes as C

import numpy as np
import pytest

import collide_ref as CR

LD = CR.LD


def _vel(n, nd, seed, scale=0.3):
    return scale * np.random.default_rng(seed).standard_normal((n, nd))


def test_key_equals_the_library(built):
    from pinc_amd import _lib
    f = _lib.HIP.pinc_hip_collide_key
    f.restype = C.c_ulonglong
    f.argtypes = [C.c_ulonglong, C.c_ulonglong, C.c_int, C.c_int]
    cases = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (12345, 678, 3, 7),
             ((1 << 64) - 1, (1 << 40) + 5, 1023, 2)]
    keys = [CR.key(*c) for c in cases]
    for c, k in zip(cases, keys):
        assert f(*c) == k, c
    assert len(set(keys)) == len(keys)


def test_uni_is_the_kernels_float64():
    # (x >> 11) + 0.5 rounds in float64 above 2^52: the restatement keeps that
    u = CR.uni(7, np.arange(100000, dtype=np.uint64))
    assert u.dtype == np.float64 and u.min() > 0.0 and u.max() <= 1.0
    assert abs(u.mean() - 0.5) < 5 / np.sqrt(12 * len(u))


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_elastic_keeps_relative_speed_and_pair_momentum(nd):
    ms, mn = 1.0, 28.0
    par = CR.Params(nu=(50.0, 0.0), b=mn / (ms + mn), vth=0.07, drift=(0.02, -0.01, 0.03), h=(1.0, 1.25, 0.5))
    vel = _vel(4000, nd, 30 + nd)
    res = CR.collide(vel, par, CR.key(3, 0, 0, 0))
    assert np.all(res.proc == 0)
    h = np.array(par.h[:nd], dtype=LD)
    w, n, g = res.extra["w"], res.extra["n"], res.extra["g"]
    w2 = res.vel * h
    # the neutral's velocity after the collision, from the pair momentum
    n2 = n + (LD(ms) / LD(mn)) * (w - w2)
    g2 = np.sqrt(np.sum((w2 - n2) ** 2, axis=1))
    assert float(np.max(np.abs(g2 - g) / g)) <= 1e-14
    # |g| kept with the momentum m_s w + m_n n: stated through the centre of mass
    cm = (LD(ms) * w + LD(mn) * n) / LD(ms + mn)
    rel = np.sqrt(np.sum((w2 - cm) ** 2, axis=1)) / (LD(mn) / LD(ms + mn) * g)
    assert float(np.max(np.abs(rel - 1))) <= 1e-14
    p0, p1 = LD(ms) * w + LD(mn) * n, LD(ms) * w2 + LD(mn) * n2
    assert float(np.max(np.abs(p1 - p0)) / np.max(np.abs(p0))) <= 1e-14


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_charge_exchange_takes_the_neutral(nd):
    par = CR.Params(nu=(0.0, 50.0), vth=0.05, drift=(0.1, 0.0, -0.1), h=(1.0, 2.0, 0.5))
    vel = _vel(3000, nd, 40 + nd)
    res = CR.collide(vel, par, CR.key(4, 2, 0, 1))
    assert np.all(res.proc == 1)
    h = np.array(par.h[:nd], dtype=LD)
    assert np.array_equal(res.vel, res.extra["n"] / h)
    # the neutrals are the Maxwellian asked for
    n = res.extra["n"].astype(np.float64)
    for d in range(nd):
        assert abs(n[:, d].mean() - par.drift[d]) < 5 * par.vth / np.sqrt(len(n))
        assert abs(n[:, d].std() / par.vth - 1) < 5 / np.sqrt(2 * len(n))


@pytest.mark.parametrize("nu", [(0.01, 0.0), (0.02, 0.03), (0.0, 1.0)])
def test_collided_count_is_binomial(nu):
    N = 100000
    par = CR.Params(nu=nu)
    res = CR.collide(_vel(N, 3, 50), par, CR.key(5, 0, 0, 0))
    P = -np.expm1(-(nu[0] + nu[1]))
    sigma = np.sqrt(N * P * (1 - P))
    nel, ncx = res.counts
    assert abs(nel + ncx - N * P) <= 5 * sigma, (nel, ncx, N * P, sigma)
    # the split between the processes, given the colliders
    q = nu[0] / (nu[0] + nu[1])
    assert abs(nel - (nel + ncx) * q) <= 5 * np.sqrt((nel + ncx) * q * (1 - q)) + 1e-9


def test_cross_section_mode_collides_the_fast_more_often():
    par = CR.Params(sig=(0.0, 0.5))
    vel = np.concatenate([np.full((20000, 3), 0.01), np.full((20000, 3), 0.5)])
    res = CR.collide(vel, par, CR.key(6, 0, 0, 0))
    slow, fast = np.sum(res.proc[:20000] >= 0), np.sum(res.proc[20000:] >= 0)
    for cnt, speed in ((slow, 0.01), (fast, 0.5)):
        P = -np.expm1(-0.5 * speed * np.sqrt(3))
        assert abs(cnt - 20000 * P) <= 5 * np.sqrt(20000 * P * (1 - P))


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_lazy_and_eager_draws_agree(nd):
    par = CR.Params(nu=(0.03, 0.02), b=0.9, vth=0.05, drift=(0.01, 0.02, 0.03), h=(1.0, 1.5, 1.0))
    vel = _vel(20000, nd, 60 + nd)
    k = CR.key(8, 3, 1, 1)
    a, b = CR.collide(vel, par, k, lazy=False), CR.collide(vel, par, k, lazy=True)
    assert np.array_equal(a.proc, b.proc) and np.array_equal(a.vel, b.vel)
    assert 0 < np.sum(a.proc >= 0) < len(vel) // 5
    assert np.array_equal(a.vel[a.proc < 0], vel[a.proc < 0].astype(LD))
    assert np.array_equal(a.m0, b.m0)


def test_reference_margins(built):
    """no decision of any case of tests/test_gpu_collide_kernel.py is within
    1e-9 of its threshold, relative to P and to r: the kernel's fp64 decisions
    cannot differ from the long-double reference's there"""
    import test_gpu_collide_kernel as K
    worst = min(CR.min_margin(K.case(name)[4]) for name in K.CASES)
    print(f"smallest decision margin over all cases: {worst:.3e}")
    assert worst > 1e-9
