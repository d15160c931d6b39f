"""Sim.phase_space through the whole stack: the operator's choice of velocity
arrays while a fused push is pending, the global frame, the schedule left
untouched, diagnostics:phaseSpace and its files.

The configuration is tests/test_gpu_moments_sim.py's: the bench's warm plasma
and its two-stream variant at 16^3 cells, 16 particles per cell and species,
tiled layout, fused push, sortInterval = 3 and sortFraction = 0 (the fixed
schedule sort, plain, count), plain multigrid at 3 levels: within 4 steps a
plain, a counting and a sorting push have each been the pending one.

Sim.phase_space(s) is compared exactly with tests/phase_ref.py of
Sim.particles(s) and Sim.offset: counts are integers.
"""
import os

import numpy as np
import pytest

import phase_ref as PR
from pinc_amd import configs

pytestmark = pytest.mark.gpu

SEED = 5
S = 16
# global-frame positions lie in [-0.5, 15.5); velocities: v_th = 0.05
SPECS = [(("x", "vx"), (32, 24), (-0.5, -0.2), (15.5, 0.2)),
         (("vx",), (64,), (-0.25,), (0.25,)),
         (("z", "vy"), (16, 16), (0.0, -0.1), (12.0, 0.1))]
KINDS = ("push_plain", "push_count", "push_sort")


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


def _check_all(s, what, specs=SPECS):
    for sp in range(s.nspecies):
        pos, vel = s.particles(sp)
        for axes, bins, lo, hi in specs:
            h, out = s.phase_space(sp, axes, bins, lo, hi)
            ref, ref_out = PR.sim_histogram(pos, vel, s.offset, axes, bins, lo, hi)
            assert h.shape == tuple(reversed(bins)) and h.dtype == np.float64
            assert h.sum() + out == len(pos), (what, sp, axes)
            assert out == ref_out, (what, sp, axes, out, ref_out)
            np.testing.assert_array_equal(h, ref, err_msg=f"{what}, species {sp}, {axes}")


def _particles(s):
    return [s.particles(sp) for sp in range(s.nspecies)]


def _bit_equal(pa, pb):
    for (xa, va), (xb, vb) in zip(pa, pb):
        np.testing.assert_array_equal(xa, xb)
        np.testing.assert_array_equal(va, vb)


def _kinds():
    from pinc_amd import _lib
    return tuple(_lib.probe_read(k)["launches"] for k in KINDS)


def _pending_move_is_x_plus_v(s, before):
    """the fused push left pending still applies after the request:
    x' = x + v, wrapped in place by +-T (a plain push keeps the order)"""
    s.op("move")
    for (x0, v0), (x1, v1) in zip(before, _particles(s)):
        xp = x0 + v0
        assert np.all((x1 == xp) | (x1 == xp + S) | (x1 == xp - S))
        np.testing.assert_array_equal(v1, v0)


@pytest.fixture(scope="module")
def plain_kinds(built):
    """the kinds of the pushes of 4 steps without a single request"""
    from pinc_amd import _lib
    with _sim(_cfg()) as s:
        s.init()
        _lib.probe_start("all", 64)
        kinds = []
        for _ in range(4):
            s.step()
            kinds.append(_kinds())
        return kinds


def test_histograms_at_every_step_and_schedule_untouched(built, plain_kinds):
    from pinc_amd import _lib
    cfg = _cfg()
    cfg["diagnostics"] = {"phaseSpace": "1000", "phaseSpaceAxes": "x,vx", "phaseSpaceBins": "32,24",
                          "phaseSpaceMin": "-0.5,-0.2", "phaseSpaceMax": "15.5,0.2"}
    with _sim(cfg) as s:
        s.init()
        _lib.probe_start("all", 64)
        _check_all(s, "after init")
        out_total = 0
        kinds = []
        for n in range(1, 5):
            s.step()
            kinds.append(_kinds())
            before = _particles(s)
            _check_all(s, f"after step {n}")
            s.op("phase")
            _bit_equal(before, _particles(s))
            out_total += sum(s.phase_space(sp, *SPECS[2])[1] for sp in range(s.nspecies))
        # each kind of push was the pending one at some request, and the
        # schedule is the one of the run that never asked
        assert all(v > 0 for v in kinds[-1]), kinds
        assert kinds == plain_kinds, (kinds, plain_kinds)
        assert out_total > 0            # (z, vy)'s range is narrower than the data
        _pending_move_is_x_plus_v(s, before)


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
        s.step()
        _check_all(s, f"{variant}, after two steps")


def test_two_stream_beams(built):
    from pinc_amd.moments import derive
    from pinc_amd.phase import density, edges
    bins, lo, hi = (80,), (-0.5,), (0.5,)      # 8 sigma around either drift
    width = (hi[0] - lo[0]) / bins[0]
    with _sim(_cfg("c4ts")) as s:
        s.init()
        s.step(2)
        assert s.nspecies == 3
        _, mass = s.species()
        for sp, drift in ((0, 0.1), (1, -0.1)):
            h, out = s.phase_space(sp, "vx", bins, lo, hi)
            assert out == 0 and h.sum() == s.count(sp)
            e = edges(bins, lo, hi)[0]
            f = density(h, bins, lo, hi)
            mean = float(np.sum(0.5 * (e[1:] + e[:-1]) * f) * width)
            M = s.moments(sp).reshape(-1, 10).sum(axis=0)
            bulk = M[1] / M[0]
            print(f"beam {sp}: mean of f(vx) {mean:.5f}, bulk velocity {bulk:.5f}, bin width {width}")
            assert abs(mean - drift) < width
            assert abs(mean - bulk) < width
        _check_all(s, "two-stream, after 2 steps", SPECS[:2])


def test_output_files(built, tmp_path):
    from pinc_amd.sim import h5_available, h5_read
    if not h5_available():
        pytest.skip("no libhdf5 on this machine (PINC_HDF5_LIB)")
    axes, bins, lo, hi = SPECS[0]
    cfg = _cfg()
    cfg["files"] = {"output": str(tmp_path) + "/"}
    cfg["diagnostics"] = {"phaseSpace": "2", "phaseSpaceAxes": ",".join(axes), "phaseSpaceBins": "32,24",
                          "phaseSpaceMin": "-0.5,-0.2", "phaseSpaceMax": "15.5,0.2"}
    live = {}
    with _sim(cfg) as s:
        s.init()
        for n in range(1, 5):
            s.step()
            s.write_output(n)
            if n % 2 == 0:
                live[n] = [s.phase_space(sp, axes, bins, lo, hi) for sp in range(s.nspecies)]
                for sp in range(s.nspecies):
                    ref, ref_out = PR.sim_histogram(*s.particles(sp), s.offset, axes, bins, lo, hi)
                    np.testing.assert_array_equal(live[n][sp][0], ref)
                    assert live[n][sp][1] == ref_out
    for sp in range(2):
        f = tmp_path / f"phase{sp}.ps.h5"
        assert f.exists()
        for n in (2, 4):
            a = h5_read(f, f"/n={n}.0")
            assert a.shape == (24, 32)
            np.testing.assert_array_equal(a, live[n][sp][0])
        for n in (1, 3):
            with pytest.raises(KeyError):
                h5_read(f, f"/n={n}.0")
        assert h5_read(f, "axes", attr=True)[0] == 0.0          # x
        assert h5_read(f, "min", attr=True)[0] == -0.5 and h5_read(f, "max", attr=True)[0] == 15.5


def test_feature_off_writes_nothing(built, tmp_path):
    """without diagnostics:phaseSpace no phase file appears"""
    from pinc_amd.sim import h5_available
    if not h5_available():
        pytest.skip("no libhdf5 on this machine (PINC_HDF5_LIB)")
    cfg = _cfg()
    cfg["files"] = {"output": str(tmp_path) + "/"}
    with _sim(cfg) as s:
        s.init()
        s.step()
        s.write_output(1)
        with pytest.raises(ValueError):
            s.op("phase")                       # no spec in the ini
    assert (tmp_path / "rho.grid.h5").exists()
    assert not list(tmp_path.glob("phase*"))


def test_bad_spec_raises(built):
    with _sim(_cfg()) as s:
        s.init()
        ok = dict(axes=("x", "vx"), bins=(8, 8), lo=(0.0, -1.0), hi=(16.0, 1.0))
        h, out = s.phase_space(0, **ok)
        assert h.shape == (8, 8)
        for bad in (dict(axes=("x", "w")), dict(axes=("x", "vx", "vy")), dict(bins=(8, 0)), dict(bins=(8,)),
                    dict(hi=(0.0, 1.0)), dict(lo=(0.0, 2.0)), dict(bins=(1 << 13, 1 << 12)),
                    dict(hi=(np.nan, 1.0))):
            with pytest.raises(ValueError):
                s.phase_space(0, **{**ok, **bad})
        for sp in (-1, 2, 7):
            with pytest.raises(ValueError):
                s.phase_space(sp, **ok)
