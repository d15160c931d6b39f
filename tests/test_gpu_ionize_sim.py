"""Ionisation through the whole stack: the ini's collisions:ion* keys,
Sim.op("ionize"), Sim.ionizations, the step's call after puMigrate, and the
operator's refusals.  8^3 cells, 8 particles per cell of electrons and of ions
of the opposite charge, room for twice as many.

  * population:layout = reference: set_particles, op("ionize"), then both
    species against tests/ionize_ref.py slot for slot: the parents, the born
    electrons behind the electrons and the born ions behind the ions, at the
    kernel test's tolerance; everything else bit for bit.  The init sequence
    ionises once, so the op is call 1 of rank 0's key;
  * the tiled and fused default, 3 full steps with ionNu = 0.05: both species
    grow by the same number each step, which is Sim.ionizations(0)'s
    increment; the charge summed over the true nodes stays what it was to
    1e-12 of sum|rho| (the pair is neutral and its charge is deposited in the
    step that bore it); the energies are finite;
  * the same 3 steps in layout = reference, run twice, give bit-identical
    populations.  That run weights to the nearest grid point (puDistrND0,
    puAccND0KE): the order-1 deposit adds with float atomics whose order
    changes from run to run (the finding of tests/test_gpu_collide_sim.py),
    and with it two runs of this test had the same births at the same slots
    but 3 of 14823 coordinates one ulp apart after the 3 steps.  One unit per
    particle makes every node sum an exact integer, so the run is
    reproducible wherever the ionisation is, and a placement that depended
    on the scheduling would still show: it permutes the born particles;
  * ionNu without ionSpecies, ionSpecies equal to the projectile or no
    species, an unknown key of [collisions], and op("ionize") with a fused
    push pending end with msg(ERROR): in subprocesses.
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ionize_ref as IR
from pinc_amd import configs

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SEED = 29
N0 = 8 ** 3 * 8


def _cfg(ion, layout="reference", **pop):
    cfg = configs.config("c3", true_size=(8, 8, 8), ppc=8, nalloc_pc=16)
    if layout == "tiled":
        # the bench's layout (configs.bench_config): tiled, sorted by the fused push
        cfg["population"].update({"layout": "tiled", "sortInterval": "8", "sortInPush": "1", "sortFraction": "0.8",
                                  "sortMax": "32"})
    cfg["population"].update(pop)
    cfg["collisions"] = ion
    return cfg


def _sim(cfg, **kw):
    from pinc_amd import Sim
    ini = configs.write_ini(cfg)
    try:
        return Sim(ini, perturb=False, seed=5, **kw)
    finally:
        os.unlink(ini)


ION = {"ionNu": "0.05,0", "ionSigma": "0.3,0", "ionThreshold": "0.2,0", "ionSpecies": "1,0", "neutralVth": "0.01",
       "neutralDrift": "0.01,0,-0.01", "seed": str(SEED)}
PAR = IR.Params(nu=0.05, sig=0.3, wth=0.2, vth=0.01, drift=(0.01, 0.0, -0.01), target=1)


def _close(got, want, bound, what):
    ratio = float(np.max(np.abs(got.astype(IR.LD) - want) / bound)) if len(want) else 0.0
    print(f"{what}: largest error / bound = {ratio:.4f}")
    assert ratio <= 1.0, what


def test_op_ionize_against_the_reference(built):
    rng = np.random.default_rng(73)
    with _sim(_cfg(ION), maxwell=True) as s:
        s.init()
        state = []
        for sp in range(2):
            pos, _ = s.particles(sp)
            # every other particle far below the threshold speed 0.2, the others far above it:
            # G - W of an ioniser is most of G whatever the number of particles the init left
            vel = rng.standard_normal(pos.shape)
            vel *= (np.where(np.arange(len(vel)) % 2, 0.5, 0.05) / np.sqrt(np.sum(vel * vel, axis=1)))[:, None]
            s.set_particles(sp, pos, vel)
            state.append((pos, vel))
        before = s.ionizations(0)
        s.op("ionize")
        (pos, vel), (ipos, ivel) = state
        ref = IR.ionize(vel, PAR, IR.key(SEED, 1, 0, 0))
        assert IR.min_margin(ref) > 1e-9 and IR.min_rem_share(ref) >= 0.5
        assert not np.any(ref.hit[::2]) and np.all(ref.extra["G"][1::2] > ref.extra["W"])
        nb, n, ni = ref.births, len(vel), len(ivel)
        assert 50 < nb < n // 2
        assert s.ionizations(0) - before == nb and s.ionizations(1) == 0
        assert [s.count(0), s.count(1)] == [n + nb, ni + nb]
        x, v = s.particles(0)
        ix, iv = s.particles(1)
        bound = IR.bound(ref, PAR, 3)
        # the electrons: positions kept, the parents rewritten, the born behind them in birth order
        np.testing.assert_array_equal(x[:n], pos)
        np.testing.assert_array_equal(np.any(v[:n] != vel, axis=1), ref.hit)
        _close(v[:n][ref.parents], ref.vel[ref.parents], bound, "parents")
        np.testing.assert_array_equal(x[n:], pos[ref.parents])
        _close(v[n:], ref.electrons, bound, "born electrons")
        # the ions: untouched, the born behind them
        np.testing.assert_array_equal(ix[:ni], ipos)
        np.testing.assert_array_equal(iv[:ni], ivel)
        np.testing.assert_array_equal(ix[ni:], pos[ref.parents])
        _close(iv[ni:], ref.ions, bound, "born ions")


RATE = {"ionNu": "0.05,0", "ionSpecies": "1,0", "neutralVth": "0.01", "seed": str(SEED)}


def _true_charge(s):
    rho = s.grid(0)[1:-1, 1:-1, 1:-1]
    return float(rho.sum()), float(np.abs(rho).sum())


def test_three_steps_in_the_tiled_fused_default(built):
    with _sim(_cfg(RATE, layout="tiled"), maxwell=True) as s:
        s.init()
        q0, _ = _true_charge(s)
        total = 0
        for step in range(3):
            n = [s.count(0), s.count(1)]
            born = s.ionizations(0)
            s.step(1)
            grew = [s.count(0) - n[0], s.count(1) - n[1]]
            q, a = _true_charge(s)
            print(f"step {step}: {grew} born, sum rho {q:.3e} (before the run {q0:.3e}), sum|rho| {a:.3e}")
            assert grew[0] == grew[1] == s.ionizations(0) - born
            assert abs(q - q0) <= 1e-12 * a
            total += grew[0]
        # about 5 % of the electrons each step
        assert 3 * 0.03 * N0 < total < 3 * 0.08 * N0
        assert s.ionizations(1) == 0
        ke, pe, kes = s.energy()
        assert np.isfinite(ke) and np.isfinite(pe) and np.all(np.isfinite(kes))
        for sp in range(2):
            x, v = s.particles(sp)
            assert np.all(np.isfinite(x)) and np.all(np.isfinite(v))


def _run_reference_layout():
    cfg = _cfg(RATE)
    cfg["methods"].update({"acc": "puAccND0KE", "distr": "puDistrND0"})
    with _sim(cfg, maxwell=True) as s:
        s.init()
        s.step(3)
        return [s.particles(sp) for sp in range(2)], s.ionizations(0)


def test_two_runs_are_bit_identical(built):
    a, na = _run_reference_layout()
    b, nb = _run_reference_layout()
    assert na == nb and na > 0
    for (xa, va), (xb, vb) in zip(a, b):
        assert xa.shape == xb.shape
        np.testing.assert_array_equal(xa.view(np.uint64), xb.view(np.uint64))
        np.testing.assert_array_equal(va.view(np.uint64), vb.view(np.uint64))


def _worker(script, kind, cfg):
    ini = configs.write_ini(cfg)
    try:
        return subprocess.run([sys.executable, str(ROOT / "tests" / script), kind, "--ini", ini], capture_output=True,
                              text=True, timeout=240, env=dict(os.environ, PYTHONPATH=str(ROOT)))
    finally:
        os.unlink(ini)


@pytest.mark.parametrize("ion,word", [({"ionNu": "0.05,0"}, "ionSpecies"),                          # no ionSpecies
                                      ({"ionNu": "0.05,0", "ionSpecies": "0,0"}, "projectile"),
                                      ({"ionNu": "0.05,0", "ionSpecies": "2,0"}, "no species"),
                                      ({"ionSigma": "0.05", "ionSpecies": "1,0"}, "ionSigma"),       # one value, two species
                                      ({"ionNu": "0.05,0", "ionSpecies": "1,0", "ionThreshold": "-1,0"}, "ionThreshold"),
                                      ({"ionNu": "0.05,0", "ionSpecies": "1,0", "ionRate": "1,1"}, "ionrate")])
def test_bad_ini_values_are_refused(built, ion, word):
    r = _worker("collide_worker.py", "create", _cfg(ion))
    assert r.returncode != 0 and "REACHED-END" not in r.stdout, (r.stdout[-800:], r.stderr[-800:])
    assert "ERROR" in r.stderr and word in r.stderr, r.stderr[-800:]


def test_ionize_with_a_fused_push_pending_is_an_error(built):
    r = _worker("ionize_worker.py", "pending", _cfg(RATE))
    assert r.returncode != 0 and "REACHED-END" not in r.stdout, (r.stdout[-800:], r.stderr[-800:])
    assert "ERROR" in r.stderr and "mccIonize" in r.stderr and "puMigrate" in r.stderr, r.stderr[-800:]
