"""Coulomb collisions in the tiled layout with the sort riding in the push
(population:sortInPush, sortInterval = 2: a counting push and a sorting push
alternate), 8^3 cells, 8 particles per cell and species, 6 steps.

The in-push sort keys a particle by the cell of x + v, and the counting push
counts those keys with the velocities it left.  mccCoulomb changes velocities
between that push and the sorting one, so it drops the counts of the species
it touched and the sorting push counts again; with stale counts a collider
whose x + v changed brick would be placed in a range reserved without it.

Checked after every step, whatever order the sort left:
  * the multiset of particles is intact: the positions read after step k + 1
    are, per dimension and as multisets, the positions read after step k moved
    by the velocities read with them (the fused push's move is still pending
    when particles are read, and the collisions of step k + 1 come after it and
    write no position), modulo the periodic length, to 1e-9;
  * the rule holds: each pair's collisions of the step are what the rule pairs
    in the cells of the positions the step left; the particle counts stay; the
    velocities are finite and below population:maxVel.
"""
import os

import numpy as np
import pytest

import coulomb_ref as CR
from pinc_amd import configs
from test_gpu_coulomb_sim import _pairs_of

pytestmark = pytest.mark.gpu
T = (8, 8, 8)


def _moved(x, v):
    """per dimension, the sorted coordinates of x + v folded into [0, T)"""
    return [np.sort(np.mod(x[:, d] + v[:, d] + 0.37, T[d])) for d in range(3)]


def test_six_steps_across_count_and_sort_pushes(built):
    from pinc_amd import Sim
    cfg = configs.config("c3", true_size=T, ppc=8, nalloc_pc=16)
    cfg["population"].update({"layout": "tiled", "sortInterval": "2", "sortInPush": "1"})
    cfg["collisions"] = {"coulombLog": "10,12,12,15", "seed": "3"}
    ini = configs.write_ini(cfg)
    try:
        with Sim(ini, maxwell=True, perturb=False, seed=5) as s:
            s.init()
            n = [s.count(0), s.count(1)]
            count = {p: s.coulomb_count(*p) for p in ((0, 0), (0, 1), (1, 1))}
            state = [s.particles(sp) for sp in range(2)]
            for step in range(6):
                s.step(1)
                assert [s.count(0), s.count(1)] == n
                new = [s.particles(sp) for sp in range(2)]
                for sp in range(2):
                    want = _moved(*state[sp])
                    got = _moved(new[sp][0], np.zeros_like(new[sp][0]))
                    for d in range(3):
                        # no coordinate within 1e-6 of the fold's seam, where the two sides would sort apart
                        assert min(want[d][0], T[d] - want[d][-1]) > 1e-6
                        np.testing.assert_allclose(got[d], want[d], rtol=0, atol=1e-9,
                                                   err_msg=f"step {step}, species {sp}, dimension {d}")
                    assert np.all(np.isfinite(new[sp][1])) and np.max(np.abs(new[sp][1])) < 1.0
                cells = [CR.cells(new[sp][0], T) for sp in range(2)]
                for (a, b), old in count.items():
                    now = s.coulomb_count(a, b)
                    assert now - old == _pairs_of(cells[a], None if a == b else cells[b], 512), (step, a, b)
                    count[(a, b)] = now
                state = new
    finally:
        os.unlink(ini)
