"""Collisions through the whole stack: the ini's [collisions] section,
Sim.op("collide"), Sim.collisions, the step's call after puMove, and the
operator's refusals.

  * set_particles, op("collide"), particles against tests/collide_ref.py with
    rank 0's key of step 0, then of step 1, at the kernel test's tolerance
    (|v' - v'_ref| h_d <= 64 eps (sum|w_d| + sum|n_d| + g); non-colliders bit
    for bit; counters exact);
  * a Sim without [collisions] and one with every rate zero are bit-identical
    in particles, rho and energies after 3 steps (8^3 cells, 4096 particles
    per species), and the zero-rate one has no operator at all (mccAlloc
    returned NULL: op("collide") is refused, nothing can be launched).  The
    run is the cold lattice (no Maxwellian, no perturbation), unfused, with
    the spectral solver: two runs of this program are bit-reproducible only
    where every deposit sum is exact, because the deposit adds with float
    atomics whose order changes from run to run.  Measured, two plain runs
    of one ini without any [collisions], twice each: warm plasma at 8^3
    with 4096 particles per species, unfused: 10 of 12288 coordinates one
    ulp apart after 3 steps; with 1024 per species (one wave per deposit)
    rho differs already after init, fused or not, spectral or multigrid;
    with 512 per species from step 1; the cold lattice (positions multiples
    of 1/2: every weight and sum exact): identical, every grid and particle,
    all 3 steps (tests/test_gpu_moments_sim.py has the same finding at 16^3);
  * charge exchange of the ions at cexNu = 0.05 for 20 steps on 16^3 with
    32768 ions, in the default layout and in the tiled one with a sort every
    8 pushes: the cumulative count within 5 sigma of Binomial(20 N, 1 -
    exp(-0.05)), the electrons' counters zero, the particle count unchanged;
  * op("collide") with a fused push pending, bad ini values, and a neutral
    above population:maxVel end with msg(ERROR): in subprocesses
    (tests/collide_worker.py).
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import collide_ref as CR
from pinc_amd import configs

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
WORKER = str(ROOT / "tests" / "collide_worker.py")
MN = 28.0 * 1836.0
MASS = (1.0, 1836.0)
SEED = 77


def _small(collisions=None, ppc=8, **pop):
    cfg = configs.config("c3", true_size=(8, 8, 8), ppc=ppc, nalloc_pc=ppc + 4)
    cfg["population"].update(pop)
    if collisions is not None:
        cfg["collisions"] = collisions
    return cfg


def _sim(cfg, **kw):
    from pinc_amd import Sim
    ini = configs.write_ini(cfg)
    try:
        return Sim(ini, maxwell=True, perturb=False, seed=5, **kw)
    finally:
        os.unlink(ini)


COLL = {"elasticNu": "0.05,0.02", "cexNu": "0,0.04", "elasticSigma": "0.1,0", "cexSigma": "0,0.2",
        "neutralMass": repr(MN), "neutralVth": "0.01", "neutralDrift": "0.01,0,-0.01", "seed": str(SEED)}
PARAMS = [CR.Params(nu=(0.05, 0.0), sig=(0.1, 0.0), b=MN / (MASS[0] + MN), vth=0.01, drift=(0.01, 0.0, -0.01)),
          CR.Params(nu=(0.02, 0.04), sig=(0.0, 0.2), b=MN / (MASS[1] + MN), vth=0.01, drift=(0.01, 0.0, -0.01))]


def test_op_collide_against_the_reference(built):
    rng = np.random.default_rng(70)
    with _sim(_small(COLL)) as s:
        s.init()
        state = []
        for sp in range(2):
            pos, _ = s.particles(sp)
            vel = 0.15 * rng.standard_normal(pos.shape)
            s.set_particles(sp, pos, vel)
            state.append((pos, vel))
        total = [[0, 0], [0, 0]]
        worst = 1.0
        for step in (0, 1):
            s.op("collide")
            for sp in range(2):
                pos, vel = state[sp]
                res = CR.collide(vel, PARAMS[sp], CR.key(SEED, step, 0, sp))
                worst = min(worst, CR.min_margin(res))
                x, got = s.particles(sp)
                np.testing.assert_array_equal(x, pos)
                CR.check(got, vel, res, PARAMS[sp], f"step {step}, species {sp}")
                for k in range(2):
                    total[sp][k] += res.counts[k]
                assert list(s.collisions(sp)) == total[sp], (step, sp)
                state[sp] = (pos, got)
        assert worst > 1e-9, worst
        assert total[0][0] > 0 and total[0][1] == 0 and total[1][0] > 0 and total[1][1] > 0


def _three_steps(cfg):
    from pinc_amd import Sim
    ini = configs.write_ini(cfg)
    try:
        with Sim(ini, maxwell=False, perturb=False) as s:
            s.init()
            s.step(3)
            parts = [s.particles(sp) for sp in range(2)]
            ke, pe, kes = s.energy()
            refused = False
            try:
                s.op("collide")
            except ValueError:
                refused = True
            return parts, s.grid(0), (ke, pe) + tuple(kes), [s.collisions(sp) for sp in range(2)], refused
    finally:
        os.unlink(ini)


def test_zero_rates_change_nothing(built):
    zero = {"elasticNu": "0,0", "cexNu": "0,0", "elasticSigma": "0,0", "cexSigma": "0,0", "neutralMass": repr(MN),
            "neutralVth": "0.01"}
    a = _three_steps(_small(fused="0"))
    b = _three_steps(_small(zero, fused="0"))
    assert len(a[0][0][0]) == len(a[0][1][0]) == 4096
    for (xa, va), (xb, vb) in zip(a[0], b[0]):
        np.testing.assert_array_equal(xa, xb)
        np.testing.assert_array_equal(va, vb)
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2] == b[2], (a[2], b[2])
    assert a[3] == b[3] == [(0, 0), (0, 0)]
    assert a[4] and b[4]          # neither has a collision operator


def test_op_collide_without_collisions(built):
    with _sim(_small()) as s:
        s.init()
        with pytest.raises(ValueError):
            s.op("collide")
        assert s.collisions(0) == (0, 0)
        with pytest.raises(ValueError):
            s.collisions(5)


@pytest.mark.parametrize("layout", ["reference", "tiled"])
def test_charge_exchange_count_over_a_run(built, layout):
    nu, steps = 0.05, 20
    cfg = configs.bench_config("c4", size=16, ppc=8, mg="plain", layout=layout, sort_interval=8, sort_fraction=0.0)
    cfg["multigrid"]["mgLevels"] = "3"
    cfg["collisions"] = {"cexNu": f"0,{nu}", "neutralVth": "0.001", "seed": "3"}
    with _sim(cfg, device_init=True) as s:
        s.init()
        n = [s.count(sp) for sp in range(2)]
        assert n[1] == 16 ** 3 * 8
        s.step(steps)
        el, cx = s.collisions(1)
        P = -np.expm1(-nu)
        mean, sigma = steps * n[1] * P, np.sqrt(steps * n[1] * P * (1 - P))
        print(f"{layout}: {cx} charge exchanges, expected {mean:.0f} +- {sigma:.0f}")
        assert el == 0 and abs(cx - mean) <= 5 * sigma
        assert s.collisions(0) == (0, 0)
        assert [s.count(sp) for sp in range(2)] == n
        # the ions have been cooled towards the neutrals' temperature or not:
        # either way every velocity is finite
        assert np.all(np.isfinite(s.particles(1)[1]))


def _worker(kind, cfg):
    ini = configs.write_ini(cfg)
    try:
        return subprocess.run([sys.executable, WORKER, kind, "--ini", ini], capture_output=True, text=True, timeout=240,
                              env=dict(os.environ, PYTHONPATH=str(ROOT)))
    finally:
        os.unlink(ini)


def test_collide_with_a_fused_push_pending_is_an_error(built):
    r = _worker("pending", _small(COLL))
    assert r.returncode != 0 and "REACHED-END" not in r.stdout, (r.stdout[-800:], r.stderr[-800:])
    assert "ERROR" in r.stderr and "mccCollide" in r.stderr and "puMove" in r.stderr, r.stderr[-800:]


def test_a_neutral_above_maxvel_stops_the_run(built):
    """charge exchange with neutrals drifting at 1.5 cells/step, population:maxVel = 1"""
    r = _worker("maxvel", _small({"cexNu": "0,30", "neutralDrift": "1.5,0,0"}))
    assert r.returncode != 0 and "REACHED-END" not in r.stdout, (r.stdout[-800:], r.stderr[-800:])
    assert "ERROR" in r.stderr and "maxVel" in r.stderr, r.stderr[-800:]


@pytest.mark.parametrize("bad,word", [({"cexNu": "0,-0.1"}, "cexNu"), ({"elasticNu": "0.1"}, "elasticNu"),
                                      ({"neutralMass": "0"}, "neutralMass"), ({"neutralDrift": "0.1,0"}, "neutralDrift"),
                                      ({"elasticRate": "0.1,0.1"}, "elasticrate"),       # no key of the section
                                      ({"neutralMassFraction": "0.5,0.5"}, "neutralMassFraction")])  # the library's own
def test_bad_ini_values_are_refused(built, bad, word):
    r = _worker("create", _small(dict(COLL, **bad)))
    assert r.returncode != 0 and "REACHED-END" not in r.stdout, (r.stdout[-800:], r.stderr[-800:])
    assert "ERROR" in r.stderr and word in r.stderr, r.stderr[-800:]
