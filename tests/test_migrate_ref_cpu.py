"""The migration reference (tests/migrate_ref.py) pinned on the CPU: the
literal serial back-fill loop equals its sparse form on every flag pattern
of up to ten particles and on every named pattern, and equals the oracle's
C restatement of puExtractEmigrants (oracle/orc_pusher.c), which passes the
reference's own known-answer case (tests/test_oracle_kat.py).
"""
import itertools

import numpy as np
import pytest

import migrate_ref as M


def _same(flags, centre):
    a = M.serial_backfill(flags, centre)
    b = M.serial_backfill_sparse(flags, centre)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    emig = np.flatnonzero(flags != centre)
    # a permutation: every survivor in one slot, every emigrant extracted once
    assert np.array_equal(np.sort(a[1]), emig)
    assert np.array_equal(np.sort(a[0]), np.setdiff1d(np.arange(len(flags)), emig))
    return a


def test_literal_equals_sparse_exhaustively():
    """all 2^n patterns, n = 1..10 (two flag values: only leaving or staying matters to the loop)"""
    for n in range(1, 11):
        for bits in itertools.product((13, 5), repeat=n):
            _same(np.array(bits, dtype=np.uint8), 13)


@pytest.mark.parametrize("n", [1, 2, 65, 2049, 6000])
def test_literal_equals_sparse_on_named_patterns(n):
    rng = np.random.default_rng(100 + n)
    names = []
    for name, flags in M.patterns(n, M.centre(3), M.codes(3), rng):
        slots, order = _same(flags, M.centre(3))
        idx, ne, count = M.bucket(order, flags)
        assert np.array_equal(np.sort(idx), np.sort(order)) and np.all(np.diff(ne.astype(int)) >= 0)
        assert count.sum() == len(order) and count[M.centre(3)] == 0
        for c in np.unique(ne):                       # stable: extraction order inside a direction
            assert np.array_equal(idx[ne == c], order[flags[order] == c])
        names.append(name)
    assert names == M.pattern_names(n)
    if n == 6000:
        assert names == list(M.PATTERN_NAMES[:-1])
    if n == 1:
        assert "head_block" not in names and "alternating" not in names


def test_every_pattern_exists_at_some_n():
    seen = set()
    for n in (1, 2, 63, 64, 65, 2047, 2048, 2049, 4096, 6000):
        seen.update(M.pattern_names(n))
    assert seen == set(M.PATTERN_NAMES)


def test_codes():
    assert M.codes(1).tolist() == [0, 2, 27] and M.centre(1) == 1
    assert M.codes(2).tolist() == [0, 1, 2, 3, 5, 6, 7, 8, 27] and M.centre(2) == 4
    assert M.codes(3).tolist() == [c for c in range(27) if c != 13] + [27] and M.centre(3) == 13


def test_pack_and_import_restatements():
    """hand-worked records: direction 5 = digits (2, 1, 0) shifts by (-T0, 0, +T2)"""
    buf = np.arange(24.0).reshape(6, 4)
    ne = np.array([5, 13, 0, 26], dtype=np.uint8)
    T = (20, 12, 16)
    rec = M.pack_ref(buf, ne, 0, 4, 3)
    assert rec[0].tolist() == [0, 4, 8, 12, 16, 20, 5]
    assert M.pack_ref(buf, ne, 1, 2, 2)[1].tolist() == [2, 6, 0, 14, 18, 0, 0]
    x, v = M.import_ref(buf, ne, 0, 4, 3, T, 7)
    assert x.tolist() == [[0 - 20, 4, 8 + 16], [1, 5, 9], [2 + 20, 6 + 12, 10 + 16], [3 - 20, 7 - 12, 11 - 16]]
    assert v.tolist() == [[12, 16, 20], [13, 17, 21], [14, 18, 22], [15, 19, 23]]
    x5, _ = M.import_ref(buf, ne, 0, 4, 3, T, 5)
    assert x5[:, 1].tolist() == [4, 5, 6, 7] and np.array_equal(x5[:, [0, 2]], x[:, [0, 2]])
    xr, vr = M.import_rec_ref(rec, 3, T)
    assert np.array_equal(xr, x) and np.array_equal(vr, v)
    assert M.import_ref(buf, ne, 2, 0, 3, T, 7)[0].shape == (0, 3)


def test_reference_equals_the_oracle(tmp_path):
    """serial_backfill + bucket against op("extract") of a one-rank cold3d
    World: about 200 particles per species placed so that the oracle's own
    classification gives the chosen flags, the species and original index in
    the velocity; survivors slot by slot, emigrants[ne] record by record
    (species after species, extraction order inside)."""
    import orc
    from pinc_amd import configs
    ini = configs.write_ini(configs.config("cold3d"), str(tmp_path / "cold3d.ini"))
    w = orc.World(ini)
    try:
        w.init()
        assert w.nranks == 1 and w.ndims == 3 and w.nspecies == 2
        t = np.zeros(6)
        orc.LIB.orc_mpi_thresholds(w._h, 0, t.ctypes.data)
        alloc = np.zeros(27, dtype=np.int64)
        orc.LIB.orc_mpi_alloc(w._h, 0, alloc.ctypes.data)
        n = 203
        assert np.all(t[3:] - t[:3] > 2)
        # a coordinate per base-3 digit: below the lower threshold, between the two, at or above the upper
        place = np.stack([t[:3] - 0.75, t[:3] + 1.0, t[3:] + 0.25])
        codes = M.codes(3)[:-1]                         # the oracle has no object sink
        for names in (("emigrant_at_m", "survivor_at_m"), ("random_0.5", "tail_block"), ("head_block", "all")):
            rng = np.random.default_rng(7)
            flags, pos, vel = [], [], []
            for s, name in enumerate(names):
                f = M.pattern(name, n + s, 13, codes, rng)
                dig = np.stack([(f.astype(int) // 3 ** d) % 3 for d in range(3)], 1)
                i = np.arange(len(f))
                p = place[dig, np.arange(3)] + (i / 4096.0)[:, None]
                flags.append(f)
                pos.append(p)
                vel.append(np.stack([np.full(len(f), float(s)), i.astype(float), -i.astype(float)], 1))
                w.set_particles(s, p, vel[s])
            cuts = [M.bucket(M.serial_backfill(f, 13)[1], f) for f in flags]
            total = sum(c[2][:27] for c in cuts)
            assert total[13] == 0 and np.all(np.delete(total < alloc, 13)), "the oracle's emigrant buffers are too small"
            w.op("extract")
            counts = w.emigrants()
            for s in range(2):
                slots, _ = M.serial_backfill(flags[s], 13)
                assert w.count(s) == len(slots)
                po, vo, _ = w.particles(s)
                np.testing.assert_array_equal(po, pos[s][slots])
                np.testing.assert_array_equal(vo, vel[s][slots])
                np.testing.assert_array_equal(counts[:, s], cuts[s][2][:27])
            for ne in range(27):
                want = [np.concatenate([pos[s][c[0][c[1] == ne]], vel[s][c[0][c[1] == ne]]], 1)
                        for s, c in enumerate(cuts)]
                np.testing.assert_array_equal(w.emigrant_records(ne), np.concatenate(want))
    finally:
        w.close()
