"""Two populations that kick with one E (tests/c_driver/pinc_twopop.c).

The host layer keeps state outside a population: the E grid's cache of every
species' rescaled E (PincDevGrid.scaledAll, filled by each fused push from the
pushing population's q/m), the registry of pending pushes that a grid write
walks (g_pendPop), and process-wide values such as the velocity bound.  With
one population none of it can go wrong.  Here population A's sorting puAcc
leaves its move pending, population B then pushes with the same E, and A is
read, its move dropped, or E rewritten: each re-applies A's kick
(pinc_pending_vel), which must use A's own charge-to-mass chain.

A: 2 species (electrons, ions), 16^3 cells, 8 particles per cell per species,
layout = tiled, fused = 1, sortInterval = 1 (every push sorts, so no species
is left in order and each takes the re-kick).  B: 1, 2 or 3 species (one
fewer: only the low entries of the cache are overwritten; one more: the cache
is reallocated) whose q/m has the opposite sign and four times the size of A's
at every shared index, so a borrowed chain moves velocities by the size of
the kick itself.

Figures of the configuration (CPU checker, test_oracle_kick_is_far_above_the_
bound; the device gives the same): kick 1.5e-3 (electrons) and 8.2e-7 (ions)
cells/step, at least 1.45e-3 and 7.9e-7 in every component, against max|v|
0.204 and 5.9e-3: 7.1e9 and 1.3e8 times the bound 1e-12 max|v|.  A pure
lattice with equal counts is neutral node by node: E = 0 exactly and no kick
at all, which is why the driver displaces A's electrons in one octant (by a
dyadic step, so that every deposit sum is exact and E is the same bit for
bit in every process).  With the cache borrowed from B (the library before
the fix) A's electrons come out 7.5e-3 off, five times the kick: -4 x in
place of 1 x.

Every run is a fresh process of the driver; runs are shared between the tests
(module cache).  Particles are compared as sets, rows sorted by position then
velocity: a sorting push orders the particles of one cell arbitrarily.
"""
import math
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from pinc_amd import configs

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "c_driver"))

NB = [2, 1, 3]  # B's species: equal to A's, one fewer, one more
SEED_A, SEED_B = 11, 23
SHIFT = 0.25  # pinc_twopop.c's displacement of A's electrons (cells)
# fused against unfused velocities (tests/test_gpu_parity.py,
# test_pending_sorting_push_read_and_dropped): 1e-12 max|v|
VEL_RTOL = 1e-12

_E, _ME, _EPS = configs.ELEMENTARY_CHARGE, configs.ELECTRON_MASS, configs.VACUUM_PERMITTIVITY


def _base():
    """The warm 16^3 plasma in SI form: what methods:normalization = semiSI
    makes of charge -1,1 / mass 1,1836 / timeStep 0.1 (units.c:159-189), so
    that B's species 0 may carry a positive charge."""
    cfg = configs.config("warm", true_size=(16, 16, 16), ppc=8, nalloc_pc=16, levels=3)
    wpe = math.sqrt(_E ** 2 * 1e11 / (_EPS * _ME))
    cfg["methods"]["normalization"] = "SI"
    cfg["time"]["timeStep"] = repr(0.1 / wpe)
    cfg["population"].update({"layout": "tiled", "sortInterval": "1", "fused": "1"})
    return cfg


def cfg_a(fused="1"):
    cfg = _base()
    cfg["population"].update({"charge": f"{-_E!r},{_E!r}", "mass": f"{_ME!r},{1836 * _ME!r}", "fused": fused})
    return cfg


def cfg_b(nb):
    """B: q/m of the opposite sign and 4 times A's at indices 0 and 1 (equal
    densities and counts: the same units as A's dictionary)."""
    cfg = _base()
    ve, vi = cfg["population"]["thermalVelocity"].split(",")
    charge = [_E, -_E, _E][:nb]
    mass = [_ME / 4, 1836 * _ME / 4, 100 * _ME][:nb]
    cfg["population"].update({
        "nSpecies": str(nb), "charge": ",".join(map(repr, charge)), "mass": ",".join(map(repr, mass)),
        "density": ",".join(["1e11"] * nb), "thermalVelocity": ",".join([ve, vi, vi][:nb]),
        "perturbAmplitude": ",".join(["0"] * 3 * nb), "perturbMode": ",".join(["0"] * 3 * nb)})
    return cfg


class _Run:
    def __init__(self, proc, out):
        self.returncode, self.stdout, self.stderr, self.out = proc.returncode, proc.stdout, proc.stderr, out

    def qm(self, who):
        rows = re.findall(rf"^TWOPOP: qm {who} (\d+) (\S+)$", self.stdout, flags=re.M)
        return np.array([float(v) for _, v in rows])

    def has(self, who, when):
        return (self.out / f"{who}_{when}_s0_pos.f64").exists()

    def particles(self, who, when, s):
        pos = np.fromfile(self.out / f"{who}_{when}_s{s}_pos.f64", dtype="<f8").reshape(-1, 3)
        vel = np.fromfile(self.out / f"{who}_{when}_s{s}_vel.f64", dtype="<f8").reshape(-1, 3)
        assert pos.shape == vel.shape and pos.shape[0] > 0
        return pos, vel


@pytest.fixture(scope="module")
def driver(built, tmp_path_factory):
    """run(scenario, nb, then=None, fused="1") -> _Run, each distinct run made
    once: a fresh process of the driver under its own time limit."""
    import build as cbuild
    exe = cbuild.build("pinc_twopop")
    base = tmp_path_factory.mktemp("twopop")
    inis = {("A", f): configs.write_ini(cfg_a(f), str(base / f"A{f}.ini")) for f in ("0", "1")}
    inis.update({("B", nb): configs.write_ini(cfg_b(nb), str(base / f"B{nb}.ini")) for nb in NB})
    cache = {}

    def run(scenario, nb, then=None, fused="1", ok=True):
        key = (scenario, nb, then, fused)
        if key not in cache:
            out = base / "_".join(map(str, key))
            out.mkdir()
            over = [f"twopop:scenario={scenario}", f"twopop:seedA={SEED_A}", f"twopop:seedB={SEED_B}"]
            if then:
                over.append(f"twopop:then={then}")
            env = dict(os.environ, PINC_QUIET="1")
            p = subprocess.run([str(exe), inis["A", fused], inis["B", nb], str(out), *over], capture_output=True,
                               text=True, timeout=120, env=env)
            cache[key] = _Run(p, out)
        r = cache[key]
        if ok:
            assert r.returncode == 0, (key, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        return r

    return run


def _as_set(pos, vel):
    o = np.lexsort(np.vstack([vel.T[::-1], pos.T[::-1]]))
    return pos[o], vel[o]


def _assert_same_set(got, want, what):
    (pg, vg), (pw, vw) = _as_set(*got), _as_set(*want)
    np.testing.assert_array_equal(pg, pw, err_msg=f"{what}: positions")
    if not np.array_equal(vg, vw):
        # (the figures the summary quotes)
        d = np.abs(vg - vw)
        print(f"{what}: max|dv| {d.max():.6e}, max|v| {np.abs(vw).max():.6e}, rows differing "
              f"{int((d > 0).any(axis=1).sum())} of {len(d)}")
    np.testing.assert_array_equal(vg, vw, err_msg=f"{what}: velocities")


# ------------------------------------------------------------ the set-up --
def _displaced(pos_global, size=16.0):
    """pinc_twopop.c's lattice_maxwell: the particles it displaces."""
    return (pos_global < 0.5 * size).all(axis=1)


def test_oracle_kick_is_far_above_the_bound():
    """The CPU checker on A's ini, seed and displacement: distr, solve,
    efield, acc.  A test of the re-kick sees nothing unless the kick itself
    is far above the comparison bound: at least 1e6 times 1e-12 max|v| for
    each species and component.  (Without the displacement the kick is
    exactly zero: the species share their lattice sites.)"""
    import orc
    ini = configs.write_ini(cfg_a())
    try:
        kicks = {}
        for shift in (0.0, SHIFT):
            w = orc.World(ini)
            w.init(perturb=False, maxwell=True, seed=SEED_A)
            p, v, ids = w.particles(0)
            # (the checker's local frame is the global one plus the ghost layer)
            sel = _displaced((p - 1.0) % 16.0)
            assert 0 < sel.sum() < len(sel)
            p = p.copy()
            p[sel] += shift
            w.set_particles(0, p, v, ids)
            for op in ("distr", "solve", "efield"):
                w.op(op)
            v0 = [w.particles(s)[1].copy() for s in range(2)]
            w.op("acc")
            kicks[shift] = [(np.abs(w.particles(s)[1] - v0[s]).max(axis=0), np.abs(w.particles(s)[1]).max())
                            for s in range(2)]
            w.close()
    finally:
        os.unlink(ini)
    for s in range(2):
        kick, vmax = kicks[SHIFT][s]
        print(f"species {s}: kick per component {kick}, max|v| {vmax:.6e}, kick / bound {kick.min() / (VEL_RTOL * vmax):.3e}")
        assert kick.min() >= 1e6 * VEL_RTOL * vmax, (s, kick, vmax)
        assert kicks[0.0][s][0].max() == 0.0, "a pure lattice is no longer neutral: say so in the module docstring"


@pytest.mark.gpu
@pytest.mark.parametrize("nb", NB)
def test_b_charge_to_mass_differs_grossly(driver, nb):
    """The normalised q/m the two populations push with: opposite sign and a
    factor of at least 3 at every shared species index."""
    r = driver("read", nb)
    qa, qb = r.qm("A"), r.qm("B")
    assert len(qa) == 2 and len(qb) == nb
    for s in range(min(2, nb)):
        assert qa[s] * qb[s] < 0 and abs(qb[s]) >= 3 * abs(qa[s]), (s, qa, qb)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", NB)
@pytest.mark.parametrize("scenario", ["read", "drop", "ewrite"])
def test_kick_is_far_above_the_bound(driver, scenario, nb):
    """On the device: max|v_end - v_init| of A is at least 1e6 times the bound
    of the comparisons below.  The move is pending or dropped, so A's
    positions are the initial ones; the rows pair by position, then velocity
    (the particles that share a lattice site get the same kick, which keeps
    their order)."""
    r = driver(scenario, nb)
    for s in range(2):
        (p0, v0), (p1, v1) = _as_set(*r.particles("A", "init", s)), _as_set(*r.particles("A", "end", s))
        np.testing.assert_array_equal(p1, p0)
        kick = np.abs(v1 - v0).max()
        print(f"{scenario} nB={nb} species {s}: kick {kick:.6e}, max|v| {np.abs(v1).max():.6e}")
        assert kick >= 1e6 * VEL_RTOL * np.abs(v1).max(), (s, kick)


# ------------------------------------------------------------- isolation --
@pytest.mark.gpu
@pytest.mark.parametrize("nb", NB)
@pytest.mark.parametrize("scenario", ["read", "drop", "ewrite"])
def test_a_is_isolated_from_b_bit_for_bit(driver, scenario, nb):
    """A after puAcc(A), puAcc(B) and the read, the dropped move or the write
    of E equals, bit for bit, A after the same without B's push."""
    r, alone = driver(scenario, nb), driver("alone", 2, then=scenario)
    for s in range(2):
        _assert_same_set(r.particles("A", "end", s), alone.particles("A", "end", s), f"{scenario} nB={nb} species {s}")


@pytest.mark.gpu
@pytest.mark.parametrize("nb", NB)
def test_rekick_equals_committed_kick(driver, nb):
    """The velocities read while A's sorted move is pending (re-kicked) are
    those puMove commits, bit for bit, with B's push in between.  The push
    really permuted every species of A: in array order the two differ."""
    r, moved = driver("read", nb), driver("move", nb)
    for s in range(2):
        v1, v2 = r.particles("A", "end", s)[1], moved.particles("A", "end", s)[1]
        assert not np.array_equal(v1, v2), f"species {s}: the sorting push left it in order"
        o1, o2 = np.lexsort(v1.T[::-1]), np.lexsort(v2.T[::-1])
        if not np.array_equal(v1[o1], v2[o2]):
            print(f"read/move nB={nb} species {s}: max|dv| {np.abs(v1[o1] - v2[o2]).max():.6e}")
        np.testing.assert_array_equal(v1[o1], v2[o2])


@pytest.mark.gpu
@pytest.mark.parametrize("nb", NB)
@pytest.mark.parametrize("scenario", ["read", "drop", "ewrite"])
def test_a_matches_unfused_reference(driver, scenario, nb):
    """An independent reference: A alone with fused = 0, whose kick_chain
    rebuilds the chain from A's own q/m and never touches the cache.
    Positions bit for bit, velocities to 1e-12 max|v|."""
    r, ref = driver(scenario, nb), driver("alone", 2, then="read", fused="0")
    for s in range(2):
        (pg, vg), (pw, vw) = _as_set(*r.particles("A", "end", s)), _as_set(*ref.particles("A", "end", s))
        np.testing.assert_array_equal(pg, pw)
        err, bound = np.abs(vg - vw).max(), VEL_RTOL * np.abs(vw).max()
        print(f"{scenario} nB={nb} species {s}: max|dv| {err:.6e}, bound {bound:.6e}")
        assert err <= bound, (scenario, nb, s, err, bound)


# ----------------------------------------------------------- B, registry --
@pytest.mark.gpu
@pytest.mark.parametrize("nb", NB)
@pytest.mark.parametrize("scenario", ["read", "free"])
def test_b_is_unharmed(driver, scenario, nb):
    """B after A's push and its own (read), and after pFree(A) and a write of
    E (free: A leaves the registry, the write re-kicks B alone), equals B
    when B is the only population pushed."""
    r = driver(scenario, nb)
    only = driver("bonly", nb, then="read" if scenario == "read" else "ewrite")
    assert r.has("A", "end") == (scenario == "read")
    for s in range(nb):
        _assert_same_set(r.particles("B", "end", s), only.particles("B", "end", s), f"{scenario} nB={nb} B species {s}")


@pytest.mark.gpu
def test_ninth_pending_population_ends_the_run(driver):
    """The registry of pending pushes holds 8 populations: the ninth sorting
    puAcc ends the run in msg(ERROR)."""
    r = driver("nine", 2, ok=False)
    assert r.returncode not in (0, None) and r.returncode > 0, (r.returncode, r.stderr[-2000:])
    assert "more than 8 populations" in r.stderr, r.stderr[-2000:]
    assert "without an error" not in r.stdout
