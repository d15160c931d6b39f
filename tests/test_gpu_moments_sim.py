"""Sim.moments through the whole stack: the operator's choice of velocity
arrays while a fused push is pending, the fold, the schedule left untouched,
diagnostics:moments and pinc_amd.moments.derive.

Runs are the bench's warm plasma (configs.bench_config("c4")) and its
two-stream variant at 16^3 cells, 16 particles per cell and species, tiled
layout, fused push, the in-push sort every third push (sortInterval = 3,
sortFraction = 0: the fixed schedule sort, plain, count; at sortInterval = 2
it alternates sort and count and no plain push occurs), so that within 4
steps a plain, a counting and a sorting push have each been the pending one.
The Poisson solver is the plain multigrid at 3 levels (16 is no multiple of 2^5; the solver is not what is
tested here).

Sim.moments(s) is compared with tests/moments_ref.py of Sim.particles(s),
folded, within moments_ref's bound (k + 8) eps sum|terms|.
"""
import os

import numpy as np
import pytest

import moments_ref as MR
from pinc_amd import configs

pytestmark = pytest.mark.gpu

SEED = 5
S = 16
GEOM = (S, S, S)


def _cfg(workload="c4", **kw):
    cfg = configs.bench_config(workload, size=S, ppc=16, mg="plain", sort_interval=3, sort_fraction=0.0, **kw)
    cfg["multigrid"]["mgLevels"] = "3"
    return cfg


def _sim(cfg):
    from pinc_amd import Sim
    ini = configs.write_ini(cfg)
    try:
        return Sim(ini, maxwell=True, perturb=False, device_init=True, seed=SEED)
    finally:
        os.unlink(ini)


def _check_all(s, what):
    for sp in range(s.nspecies):
        M = s.moments(sp)
        pos, vel = s.particles(sp)
        assert M.shape == (S, S, S, 10)
        MR.check(M, MR.folded(MR.moments_reference(pos, vel, GEOM), S), f"{what}, species {sp}")


def _state(s):
    ke, pe, kes = s.energy()
    return (ke, pe) + tuple(kes)


def _particles(s):
    return [s.particles(sp) for sp in range(s.nspecies)]


def _bit_equal(pa, pb):
    for (xa, va), (xb, vb) in zip(pa, pb):
        np.testing.assert_array_equal(xa, xb)
        np.testing.assert_array_equal(va, vb)


# Two runs of this configuration that never ask for moments are themselves
# not bit-identical: the charge deposit adds with float atomics, whose order
# changes from run to run (measured on this workload: PE 541.893725350873 and
# 541.8937253508728, one species' KE 394194.86177395756 and 394194.8617739575,
# and particles that differ in the last bit, between two plain runs).  So
# "bit-identical to a run that never asked" is asserted where the program is
# deterministic: the population is bit for bit the same before and after a
# request, the pending move applied after it is x + v bit for bit, and the
# kind of every push (plain, count, sort) is the same as in the run that never
# asked.  The energies of the two runs are compared to ENERGY_RTOL: a node's
# charge differs by summation order by at most (k + 4) eps (the push test's
# bound; k <= 8 * 16 contributions here: 3e-14), the net charge of the
# quasi-neutral plasma is the difference of two species' sums about 16 / 4
# times larger than it (ppc over its noise), PE is quadratic in it, and four
# steps repeat this: 2 * 4 * 4 * 3e-14 = 1e-12, rounded up.
ENERGY_RTOL = 1e-11
KINDS = ("push_plain", "push_count", "push_sort")


def _kinds():
    from pinc_amd import _lib
    return tuple(_lib.probe_read(k)["launches"] for k in KINDS)


def _pending_move_is_x_plus_v(s, before):
    """the fused push left pending (a plain one: the order is kept) still
    applies after the request: x' = x + v, wrapped in place by +-T"""
    s.op("move")
    for (x0, v0), (x1, v1) in zip(before, _particles(s)):
        xp = x0 + v0
        assert np.all((x1 == xp) | (x1 == xp + S) | (x1 == xp - S))
        np.testing.assert_array_equal(v1, v0)


@pytest.fixture(scope="module")
def plain_run(built):
    """4 steps without a single request for moments: the energies and the
    kinds of its pushes, step by step"""
    from pinc_amd import _lib
    with _sim(_cfg()) as s:
        s.init()
        _lib.probe_start("all", 64)
        kinds = []
        for _ in range(4):
            s.step()
            kinds.append(_kinds())
        return _state(s), kinds


def test_moments_at_every_step_and_schedule_untouched(built, plain_run):
    from pinc_amd import _lib
    with _sim(_cfg()) as s:
        s.init()
        _lib.probe_start("all", 64)
        _check_all(s, "after init")
        kinds = []
        for n in range(1, 5):
            s.step()
            kinds.append(_kinds())
            before = _particles(s)
            _check_all(s, f"after step {n}")
            s.op("moments")
            _bit_equal(before, _particles(s))
        got = _state(s)
        # each kind of push was the pending one at some request, and the
        # schedule is the one of the run that never asked
        assert all(v > 0 for v in kinds[-1]), kinds
        assert kinds == plain_run[1], (kinds, plain_run[1])
        print(f"energies {got} / {plain_run[0]}")
        np.testing.assert_allclose(got, plain_run[0], rtol=ENERGY_RTOL, atol=0)
        _pending_move_is_x_plus_v(s, before)


def test_op_between_acc_and_move(built):
    """the step as single operators, with and without the moments between
    acc and move"""
    ops = ("move", "extract", "migrate", "distr", "solve", "efield_fused", "acc")
    res = []
    for ask in (True, False):
        with _sim(_cfg()) as s:
            s.init()
            for _ in range(4):
                for op in ops:
                    s.op(op)
                if ask:
                    before = _particles(s)
                    s.op("moments")
                    _bit_equal(before, _particles(s))
                s.op("energy")
            res.append(_state(s))
            if ask:
                _pending_move_is_x_plus_v(s, before)
    print(f"energies {res[0]} / {res[1]}")
    np.testing.assert_allclose(res[0], res[1], rtol=ENERGY_RTOL, atol=0)


@pytest.mark.parametrize("variant", ["reference", "unfused"])
def test_other_layouts(built, variant):
    cfg = _cfg(layout="reference")
    if variant == "unfused":
        cfg["population"]["fused"] = "0"
    with _sim(cfg) as s:
        s.init()
        _check_all(s, f"{variant}, after init")
        s.step()
        _check_all(s, f"{variant}, after a step")


def test_two_stream_bulk_velocities(built):
    from pinc_amd.moments import derive
    with _sim(_cfg("c4ts")) as s:
        s.init()
        s.step(2)
        assert s.nspecies == 3
        _, mass = s.species()
        for sp, drift in ((0, 0.1), (1, -0.1)):
            d = derive(s.moments(sp), mass[sp], 3)
            u = np.nanmean(d.u.reshape(-1, 3), axis=0)
            print(f"beam {sp}: mean bulk velocity {u}, mean T {np.nanmean(d.T):.3e}")
            assert np.all(np.abs(u - drift) < 1e-3), (sp, u)
            assert np.all(d.n > 0) and np.nanmean(d.T) > 0
        _check_all(s, "two-stream, after 2 steps")


def test_output_files(built, tmp_path):
    from pinc_amd.sim import h5_available, h5_read
    if not h5_available():
        pytest.skip("no libhdf5 on this machine (PINC_HDF5_LIB)")
    cfg = _cfg()
    cfg["files"] = {"output": str(tmp_path) + "/"}
    cfg["diagnostics"] = {"moments": "2"}
    refs = {}
    with _sim(cfg) as s:
        s.init()
        for n in range(1, 5):
            s.step()
            s.write_output(n)
            if n % 2 == 0:
                refs[n] = [MR.folded(MR.moments_reference(*s.particles(sp), GEOM), S) for sp in range(s.nspecies)]
                live = [s.moments(sp) for sp in range(s.nspecies)]
                for sp in range(s.nspecies):
                    MR.check(live[sp], refs[n][sp], f"Sim.moments, step {n}, species {sp}")
    for sp in range(2):
        f = tmp_path / f"moments{sp}.grid.h5"
        assert f.exists()
        for n in (2, 4):
            a = h5_read(f, f"/n={n}.0")
            assert a.shape == (S, S, S, 10)
            MR.check(a, refs[n][sp], f"file, step {n}, species {sp}")
        for n in (1, 3):
            with pytest.raises(KeyError):
                h5_read(f, f"/n={n}.0")


def test_feature_off_allocates_nothing(built, tmp_path):
    """without diagnostics:moments no moments file appears"""
    from pinc_amd.sim import h5_available
    if not h5_available():
        pytest.skip("no libhdf5 on this machine (PINC_HDF5_LIB)")
    cfg = _cfg()
    cfg["files"] = {"output": str(tmp_path) + "/"}
    with _sim(cfg) as s:
        s.init()
        s.step()
        s.write_output(1)
    assert (tmp_path / "rho.grid.h5").exists()
    assert not list(tmp_path.glob("moments*"))
