"""Coulomb collisions through the whole stack: the ini's collisions:coulombLog,
Sim.op("coulomb"), Sim.coulomb_count, Sim.coulomb_coef, the step's call after
puMigrate, and the ini's refusals.  8^3 cells, 8 particles per cell of
electrons and of ions (1 : 1836), equal weights.

  * op("coulomb") leaves exactly the bits of direct pinc_hip_coulomb calls for
    (0, 0), (0, 1), (1, 1) on a copy of the population, with the host's key
    (the init sequence has collided once: call 1) and Sim.coulomb_coef;
    Sim.coulomb_count grows by the direct calls' counters; the coefficient is
    the closed form of the ini's SI inputs;
  * a full step collides after the migration: each pair's count of the step is
    what the rule pairs in the cells of the positions the step left (the step
    does not move a particle after its collisions); the particle counts stay;
    the init sequence collides too (after its migration, before its half
    kick): against the same ini without coulombLog, whose init has the same
    positions, fields and kicks, the total momentum differs by at most
    (8 P + 2) eps sum m |v| with P = 8 collisions per particle (the kernel
    test's bound per cell, and one rounding of the kick's sum per run).  The
    momentum of the later steps is not asserted: there the fields change it,
    and the run without coulombLog has other positions after its first move,
    so nothing separates the collisions' share (the kernel tests hold every
    launch's momentum per cell);
  * coulombLog all zero: 3 steps on the cold lattice are bit-identical to the
    ini without the key (positions, velocities, rho, phi, energies), and the op
    warns (a ValueError in Python);
  * elastic and ionisation rates: their counts over 3 steps are the same with
    and without coulombLog (separate key streams and call counters);
  * an asymmetric matrix, a wrong count, a negative entry, a 2-D grid and
    unequal weights on an unlike pair end with msg(ERROR): in subprocesses.
"""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import coulomb_ref as CR
from coulomb_abi import declare, params_t
from pinc_amd import configs
from push_abi import Pop, geom_of

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SEED = 41
T = (8, 8, 8)
LOG = {"coulombLog": "10,12,12,15", "seed": str(SEED)}


def _cfg(collisions=None, **pop):
    cfg = configs.config("c3", true_size=T, ppc=8, nalloc_pc=16)
    cfg["population"].update(pop)
    if collisions is not None:
        cfg["collisions"] = collisions
    return cfg


def _sim(cfg, maxwell=True):
    from pinc_amd import Sim
    ini = configs.write_ini(cfg)
    try:
        return Sim(ini, maxwell=maxwell, perturb=False, seed=5)
    finally:
        os.unlink(ini)


def _fractions(s, a, b):
    """mu / m_a and mu / m_b as the host forms them"""
    _, m = s.species()
    mu = m[a] * m[b] / (m[a] + m[b])
    return mu / m[a], mu / m[b]


def test_op_coulomb_is_the_direct_kernel_call(built):
    import torch
    from pinc_amd import _lib
    hip = declare(_lib.HIP)
    with _sim(_cfg(LOG, fused="0")) as s:
        s.init()
        state = [s.particles(sp) for sp in range(2)]
        n = [len(x) for x, _ in state]
        before = {(a, b): s.coulomb_count(a, b) for a, b in ((0, 0), (0, 1), (1, 1))}
        assert all(v > 0 for v in before.values())          # the init sequence collided
        assert s.coulomb_count(1, 0) == before[(0, 1)]
        s.op("coulomb")
        after = [s.particles(sp) for sp in range(2)]
        # the same launches on a copy
        first = [0, n[0] + 3]
        cap = first[1] + n[1]
        t = []
        for r in range(6):
            host = np.zeros(cap)
            for sp in range(2):
                host[first[sp]:first[sp] + n[sp]] = state[sp][r // 3][:, r % 3]
            t.append(torch.from_numpy(host).cuda())
        vp3 = C.c_void_p * 3
        pop = Pop(vp3(*[x.data_ptr() for x in t[:3]]), vp3(*[x.data_ptr() for x in t[3:]]), 2, 3,
                  (C.c_long * 9)(first[0], first[1], cap), (C.c_long * 8)(first[0] + n[0], first[1] + n[1]))
        for a, b in ((0, 0), (0, 1), (1, 1)):
            K = s.coulomb_coef(a, b)
            assert K > 0 and s.coulomb_coef(b, a) == K
            fa, fb = _fractions(s, a, b)
            par = CR.Params(K=K, fa=fa, fb=fb)
            need = hip.pinc_hip_coulomb_work(n[a], 0 if a == b else n[b], T[0] * T[1] * T[2])
            work = torch.zeros(need, dtype=torch.int32, device="cuda")
            counts = torch.zeros(1, dtype=torch.int64, device="cuda")
            rc = hip.pinc_hip_coulomb(pop, a, b, geom_of(T), params_t(par, CR.key(SEED, 1, 0, a, b)), work.data_ptr(),
                                      need, counts.data_ptr(), None)
            assert rc == 0, hip.pinc_hip_error_string()
            torch.cuda.synchronize()
            assert s.coulomb_count(a, b) - before[(a, b)] == int(counts.cpu()[0]) > 0
        for sp in range(2):
            np.testing.assert_array_equal(after[sp][0], state[sp][0])
            got = np.stack([x.cpu().numpy()[first[sp]:first[sp] + n[sp]] for x in t[3:]], 1)
            assert np.any(got != state[sp][1])
            np.testing.assert_array_equal(after[sp][1].view(np.uint64), got.view(np.uint64))
        with pytest.raises(ValueError):
            s.coulomb_count(0, 2)
        with pytest.raises(ValueError):
            s.coulomb_coef(-1, 0)


def test_coefficient_is_the_closed_form_of_the_ini(built):
    """K_ab = (q_a q_b)^2 lnL / (8 pi eps0^2 mu^2) (W / cell volume) dt (dt / X)^3
    from the ini's SI values (semiSI: charges in e, masses in m_e, the time step
    in 1 / omega_pe of species 0)"""
    cfg = _cfg(LOG)
    eps0, e, me = configs.VACUUM_PERMITTIVITY, configs.ELEMENTARY_CHARGE, configs.ELECTRON_MASS
    X = float(cfg["grid"]["stepSize"])
    dens = [float(x) for x in cfg["population"]["density"].split(",")]
    dt = float(cfg["time"]["timeStep"]) / np.sqrt(e * e * dens[0] / (eps0 * me))
    q, m = np.array([-e, e]), np.array([me, 1836 * me])
    W = dens[0] * X ** 3 / 8
    logs = {(0, 0): 10.0, (0, 1): 12.0, (1, 1): 15.0}
    with _sim(cfg) as s:
        for (a, b), lnL in logs.items():
            mu = m[a] * m[b] / (m[a] + m[b])
            want = (q[a] * q[b]) ** 2 * lnL / (8 * np.pi * eps0 ** 2 * mu ** 2) * (W / X ** 3) * dt * (dt / X) ** 3
            assert abs(s.coulomb_coef(a, b) - want) <= 1e-10 * want, (a, b, s.coulomb_coef(a, b), want)


def _pairs_of(cells_a, cells_b, nc):
    """the collisions the rule pairs in these cells (no two equal velocities)"""
    na = np.bincount(cells_a, minlength=nc)
    if cells_b is None:
        return int(np.sum(na // 2 + 2 * ((na & 1) & (na >= 3))))
    nb = np.bincount(cells_b, minlength=nc)
    return int(np.sum(np.where((na > 0) & (nb > 0), np.maximum(na, nb), 0)))


def test_a_step_collides_after_the_migration(built):
    with _sim(_cfg()) as plain:
        plain.init()
        without = [plain.particles(sp) for sp in range(2)]
    with _sim(_cfg(LOG)) as s:
        s.init()
        _, m = s.species()
        mom, scale = np.zeros(3), 0.0
        for sp in range(2):
            (x1, v1), (x0, v0) = s.particles(sp), without[sp]
            np.testing.assert_array_equal(x1, x0)
            assert np.any(v1 != v0)
            mom += m[sp] * (np.sum(v1.astype(np.longdouble), 0) - np.sum(v0.astype(np.longdouble), 0)).astype(float)
            scale += m[sp] * float(np.sum(np.abs(v0)))
        print("momentum change by the collisions / (eps sum m|v|):", mom / (CR.EPS * scale))
        assert np.all(np.abs(mom) <= (8 * 8 + 2) * CR.EPS * scale)
        count = {p: s.coulomb_count(*p) for p in ((0, 0), (0, 1), (1, 1))}
        n = [s.count(0), s.count(1)]
        for step in range(2):
            s.step(1)
            assert [s.count(0), s.count(1)] == n
            cells = [CR.cells(s.particles(sp)[0], T) for sp in range(2)]
            for (a, b), old in count.items():
                new = s.coulomb_count(a, b)
                assert new - old == _pairs_of(cells[a], None if a == b else cells[b], 512), (step, a, b)
                count[(a, b)] = new
        ke, pe, kes = s.energy()
        assert np.isfinite(ke) and np.isfinite(pe)


def _three_steps(cfg):
    with _sim(cfg, maxwell=False) as s:
        s.init()
        s.step(3)
        parts = [s.particles(sp) for sp in range(2)]
        ke, pe, kes = s.energy()
        refused = False
        try:
            s.op("coulomb")
        except ValueError:
            refused = True
        return parts, s.grid(0), s.grid(1), (ke, pe) + tuple(kes), s.coulomb_count(0, 1), refused


def test_all_zero_and_absent_change_nothing(built):
    a = _three_steps(_cfg(fused="0"))
    b = _three_steps(_cfg({"coulombLog": "0,0,0,0"}, fused="0"))
    for (xa, va), (xb, vb) in zip(a[0], b[0]):
        np.testing.assert_array_equal(xa.view(np.uint64), xb.view(np.uint64))
        np.testing.assert_array_equal(va.view(np.uint64), vb.view(np.uint64))
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2], b[2])
    assert a[3] == b[3], (a[3], b[3])
    assert a[4] == b[4] == 0
    assert a[5] and b[5]          # neither has an active pair: the op warns


def test_other_collisions_draw_the_same_with_and_without(built):
    other = {"elasticNu": "0.05,0.02", "neutralMass": repr(28.0 * 1836.0), "neutralVth": "0.01", "ionNu": "0.02,0",
             "ionSpecies": "1,0", "seed": str(SEED)}
    out = []
    for extra in ({}, {"coulombLog": "10,12,12,15"}):
        with _sim(_cfg(dict(other, **extra))) as s:
            s.init()
            s.step(3)
            out.append(([s.collisions(sp) for sp in range(2)], [s.ionizations(sp) for sp in range(2)],
                        s.coulomb_count(0, 0)))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1], out
    assert out[0][0][0][0] > 0 and out[0][1][0] > 0
    assert out[0][2] == 0 and out[1][2] > 0


def _worker(cfg):
    ini = configs.write_ini(cfg)
    try:
        return subprocess.run([sys.executable, str(ROOT / "tests" / "collide_worker.py"), "create", "--ini", ini],
                              capture_output=True, text=True, timeout=240, env=dict(os.environ, PYTHONPATH=str(ROOT)))
    finally:
        os.unlink(ini)


def _flat():
    cfg = configs.config("langmuir2d")
    cfg["collisions"] = {"coulombLog": "10,10,10,10"}
    return cfg


@pytest.mark.parametrize("cfg,word", [(lambda: _cfg({"coulombLog": "10,12,11,15"}), "symmetric"),
                                      (lambda: _cfg({"coulombLog": "10,12,15"}), "nSpecies x nSpecies"),
                                      (lambda: _cfg({"coulombLog": "10,-1,-1,15"}), ">= 0"),
                                      (_flat, "nDims"),
                                      (lambda: _cfg({"coulombLog": "10,12,12,15"}, density="1e11,2e11"), "equal weights"),
                                      (lambda: _cfg({"coulombLog": "10,0,0,15", "macroWeight": "1,1"}), "macroWeight")])
def test_bad_ini_values_are_refused(built, cfg, word):
    r = _worker(cfg())
    assert r.returncode != 0 and "REACHED-END" not in r.stdout, (r.stdout[-800:], r.stderr[-800:])
    assert "ERROR" in r.stderr and word in r.stderr, r.stderr[-800:]


def test_unequal_weights_are_fine_for_like_pairs(built):
    with _sim(_cfg({"coulombLog": "10,0,0,15"}, density="1e11,2e11")) as s:
        assert s.coulomb_coef(0, 0) > 0 and s.coulomb_coef(1, 1) > 0 and s.coulomb_coef(0, 1) == 0
