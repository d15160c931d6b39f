"""The restatement of the Coulomb collision rule (tests/coulomb_ref.py) held to
its own invariants, to the keys of the other collision processes, to the
decision margins the GPU tests rely on, to the physics of the rule, and the
coefficient K_ab to its closed form (no GPU)."""
import ctypes as C

import numpy as np
import pytest

import collide_ref as COL
import coulomb_cases as CC
import coulomb_ref as CR
import ionize_ref as ION

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)


def cap(built) -> int:
    from pinc_amd import _lib
    f = _lib.HIP.pinc_hip_coulomb_cell_cap
    f.restype = C.c_long
    return int(f())


def test_one_collision_conserves_momentum_and_energy():
    """per collision, in long double, to its rounding: small-angle and
    isotropic, g_perp == 0 with either sign of gz, 1836 : 1 and equal masses"""
    rng = np.random.default_rng(11)
    key = CR.subkey(CR.key(5, 0, 0, 0, 1), 3)
    n = {"small": 0, "iso": 0, "gp0": 0}
    for j in range(400):
        wp, wq = (rng.standard_normal(3).astype(LD) * LD(0.2) for _ in range(2))
        if j % 10 == 0:
            wq[:2] = wp[:2]                      # g_perp == 0, gz of either sign
        fa = 1836.0 / 1837.0 if j % 2 else 0.5
        mp, mq = LD(1 - fa), LD(fa)              # m_p : m_q = fq : fp
        kv = 10.0 ** rng.uniform(-6, 0)
        np_, nq_, info = CR.collide_one(wp, wq, kv, mq / (mp + mq), mp / (mp + mq), key, j)
        n["small" if info["small"] else "iso"] += 1
        n["gp0"] += int(info["gp"] == 0)
        scale = float(np.sum(np.abs(wp)) + np.sum(np.abs(wq)))
        assert np.all(np.abs((mp * np_ + mq * nq_) - (mp * wp + mq * wq)) <= 16 * EPS_LD * scale)
        e0 = mp * np.sum(wp * wp) + mq * np.sum(wq * wq)
        e1 = mp * np.sum(np_ * np_) + mq * np.sum(nq_ * nq_)
        assert abs(e1 - e0) <= 64 * EPS_LD * float(np.sum(wp * wp) + np.sum(wq * wq))
        g1 = np_ - nq_
        assert abs(np.sqrt(np.sum(g1 * g1)) - info["g"]) <= 32 * EPS_LD * float(info["g"])
    assert min(n.values()) > 10, n
    same = np.array([0.1, 0.2, 0.3], dtype=LD)
    assert CR.collide_one(same, same.copy(), 1.0, 0.5, 0.5, key, 0)[0] is None     # g == 0


def test_schedule_every_a_member_once_and_the_triple_halves():
    rng = np.random.default_rng(12)
    k = CR.key(1, 2, 0, 0, 1)
    ca, cb = rng.integers(0, 6, 200), rng.integers(0, 6, 37)
    for cell_a, cell_b in ((ca, cb), (cb, ca)):
        sched, gap = CR.schedule(cell_a, cell_b, k, 6)
        assert gap >= 1
        for c in range(6):
            na, nb = int(np.sum(cell_a == c)), int(np.sum(cell_b == c))
            mine = [s for s in sched if s.cell == c]
            sA = 0 if na >= nb else 1
            assert all(s.sp == sA and s.sq == 1 - sA and s.n_low == min(na, nb) and s.f == 1.0 for s in mine)
            members_a = np.flatnonzero((cell_a if sA == 0 else cell_b) == c)
            assert sorted(s.jp for s in mine) == members_a.tolist()          # every A-member exactly once
            per_b = np.unique([s.jq for s in mine], return_counts=True)[1]
            Q, Rm = divmod(max(na, nb), min(na, nb))
            assert sorted(per_b.tolist()) == sorted([Q + 1] * Rm + [Q] * (min(na, nb) - Rm))
            # a B-member's partners are consecutive
            jq = [s.jq for s in mine]
            assert len([1 for x, y in zip(jq, jq[1:]) if x != y]) == len(set(jq)) - 1
    # like: N = 7 gives the triple with f = 1/2 on (L0,L1), (L1,L2), (L2,L0), then two plain pairs
    sched, _ = CR.schedule(np.zeros(7, int), None, k, 1)
    L, _ = CR.ordered(np.arange(7), CR.subkey(k, 1))
    assert [(s.jp, s.jq, s.f) for s in sched] == [(L[0], L[1], 0.5), (L[1], L[2], 0.5), (L[2], L[0], 0.5),
                                                  (L[3], L[4], 1.0), (L[5], L[6], 1.0)]
    assert all(s.n_low == 7 for s in sched)
    assert CR.schedule(np.zeros(1, int), None, k, 1)[0] == []
    # the order does not depend on how the members were gathered
    p = rng.permutation(7)
    assert CR.ordered(np.arange(7)[p], CR.subkey(k, 1))[0].tolist() == L.tolist()


def test_keys_are_separate(built):
    from pinc_amd import _lib
    f = _lib.HIP.pinc_hip_coulomb_key
    f.argtypes = [C.c_ulonglong, C.c_ulonglong, C.c_int, C.c_int, C.c_int]
    f.restype = C.c_ulonglong
    seen = set()
    for seed in (0, 1, 99):
        for step in (0, 1, 2):
            for rank in (0, 1):
                for s in range(3):
                    ks = {COL.key(seed, step, rank, s), ION.key(seed, step, rank, s)}
                    for b in range(s, 3):
                        kc = CR.key(seed, step, rank, s, b)
                        assert f(seed, step, rank, s, b) == kc
                        ks |= {kc} | {CR.subkey(kc, t) for t in (1, 2, 3, 4)}
                    assert len(ks) == 2 + 5 * (3 - s)
                    assert not (ks & seen)
                    seen |= ks


@pytest.mark.parametrize("name", CC.NAMES)
def test_reference_margins(built, name):
    """every decision of every GPU case is at least 1e-9 from its threshold
    (var from 1; g and g_perp from 0 unless exactly 0, which a difference of
    equal numbers is in any precision) and no two hash keys of a cell are
    equal: the GPU tests allow no differing decision"""
    _, _, launches, results = CC.case(name, cap(built))
    assert len(results) == len(launches)
    for n, r in enumerate(results):
        for v in ("var", "gp", "g"):
            assert r.margins[v] > 1e-9, (name, n, v, r.margins[v])
        assert r.margins["hash_gap"] >= 1, (name, n)


def test_float64_twin_is_the_restatement():
    rng = np.random.default_rng(13)
    N, K = 64, 3e-6
    vel = 0.1 * rng.standard_normal((N, 3))
    pos = np.full((N, 3), 1.5)
    keys = [CR.key(3, s, 0, 0, 0) for s in range(3)]
    twin = CR.relax_f64(vel, K, keys, 3)
    v = vel
    for s in range(3):
        r = CR.coulomb(pos, v, None, None, CR.Params(K=K), keys[s], (1, 1, 1))
        assert r.count == N // 2
        v = np.asarray(r.vel[0], dtype=np.float64)
        np.testing.assert_allclose(twin[s + 1], v, rtol=0, atol=1e-13)


def relaxation_rate_closed_form(K, N, Tx, Tz):
    """d(T_z - T_perp)/step that the rule implies for small angles.  A pair
    with relative velocity g turns it by Theta with <Theta^2> = 4 var = 4 K N /
    g^3 about a uniform azimuth: <d g_z^2> = (Theta^2 / 2)(g^2 - 3 g_z^2), and
    the pair's sum of w_z^2 moves by half of that.  With N / 2 pairs among N
    particles, d T_z = (K N / 2) <(g^2 - 3 g_z^2) / g^3> over the pairs'
    relative velocities, Gaussian with variances 2 T_x, 2 T_x, 2 T_z.  In
    spherical coordinates the radial integral is elementary, leaving
        <(g^2 - 3 g_z^2) / g^3> = (2 pi)^(-1/2) / (a sqrt(c)) int_-1^1 (1 - 3 m^2) / q(m) dm,
        q(m) = (1 - m^2) / a + m^2 / c,  a = 2 T_x, c = 2 T_z,
    and d T_perp = -d T_z / 2 (energy is conserved)."""
    a, c = 2 * Tx, 2 * Tz
    m, wts = np.polynomial.legendre.leggauss(200)
    integral = np.sum(wts * (1 - 3 * m * m) / ((1 - m * m) / a + m * m / c))
    dTz = (K * N / 2) * integral / (np.sqrt(2 * np.pi) * a * np.sqrt(c))
    return 1.5 * dTz


def test_temperature_anisotropy_relaxes_at_the_rule_s_rate():
    """A like-particle Maxwellian with T_z = 2 T_x in one cell (N = 32768,
    var of the order 1e-3), 30 launches of the float64 twin per seed, 10 seeds:
    the mean of (D_30 - D_0) / 30, D = T_z - (T_x + T_y) / 2, against the
    closed form above at the initial temperatures.  The margin is three times
    the seed-to-seed standard deviation of that rate.

    Measured: closed form -1.1385e-5 per step, mean of the seeds -1.1287e-5
    (0.9 % slower: by the interval's middle the anisotropy has decayed by
    1.7 % of itself), standard deviation 8.2e-7, margin 2.4e-6."""
    N, K, steps, Tx, Tz = 32768, 5e-10, 30, 0.01, 0.02
    want = relaxation_rate_closed_form(K, N, Tx, Tz)
    rates = []
    for seed in range(10):
        rng = np.random.default_rng(1000 + seed)
        vel = rng.standard_normal((N, 3)) * np.sqrt([Tx, Tx, Tz])
        vel -= vel.mean(0)
        vel *= np.sqrt([Tx, Tx, Tz]) / vel.std(0)
        w = CR.relax_f64(vel, K, [CR.key(seed, s, 0, 0, 0) for s in range(steps)], steps)
        T = np.mean(w * w, axis=1)                    # (steps + 1, 3)
        D = T[:, 2] - 0.5 * (T[:, 0] + T[:, 1])
        np.testing.assert_allclose(T.sum(1), T[0].sum(), rtol=1e-12)      # energy
        np.testing.assert_allclose(w.mean(1), 0, atol=1e-15)              # momentum
        rates.append((D[-1] - D[0]) / steps)
    mean, sd = np.mean(rates), np.std(rates, ddof=1)
    print(f"closed form {want:.4e}, mean {mean:.4e}, sd {sd:.3e}, margin {3 * sd:.3e}")
    assert want < 0
    assert abs(mean - want) <= 3 * sd, (mean, want, sd)


def test_coefficient_from_si_inputs_is_the_closed_form():
    """K_ab = (q_a q_b)^2 lnL / (8 pi eps0^2 mu^2) x (W / cell volume) x dt, for g
    in stepSize[0] / dt, against the normalised form the host computes,
    (qh_a qh_b / muh)^2 lnL / (8 pi W H): uNormalize's charge and mass of a
    computational particle are q W / Q and m W / M with Q = W_0 |q_0| and
    M = (dt Q)^2 / (eps0 X^3)."""
    eps0, e, me = 8.8541878128e-12, 1.602176634e-19, 9.1093837015e-31
    q, m = np.array([-e, e]), np.array([me, 1836.15 * me])
    step = np.array([2e-3, 3e-3, 2.5e-3])
    dt, density, L, ppc, lnL = 4e-10, 5e12, (8, 8, 8), 8, 11.5
    V = np.prod(L) * step[0] ** 3                      # units.c's volume (stepSize[0] cubed per cell)
    W = density * V / (ppc * np.prod(L))
    X, Q = step[0], W * e
    M = (dt * Q) ** 2 / (eps0 * X ** 3)
    qh, mh = q * W / Q, m * W / M
    H = np.prod(step) / X ** 3
    for a, b in ((0, 0), (0, 1), (1, 1)):
        mu = m[a] * m[b] / (m[a] + m[b])
        si = (q[a] * q[b]) ** 2 * lnL / (8 * np.pi * eps0 ** 2 * mu ** 2) * (W / np.prod(step)) * dt * (dt / X) ** 3
        muh = mh[a] * mh[b] / (mh[a] + mh[b])
        code = (qh[a] * qh[b] / muh) ** 2 * lnL / (8 * np.pi * W * H)
        assert abs(code - si) <= 1e-12 * si, (a, b, code, si)
