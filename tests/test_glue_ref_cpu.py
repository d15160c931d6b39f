"""The restatements of tests/glue_ref.py themselves (no GPU): on the very
inputs the GPU tests use, each restatement differs from at least one
deliberate mutant of it -- by a bit where the GPU test is bitwise, by more
than 1e-6 relative where it uses a bound -- and the planted inputs do what
they are planted for.
"""
import numpy as np
import pytest

import glue_ref as G
import migrate_ref as M
from gpu_buf import same_bits

LD = G.LD
GAP = 1e-6


def floor_int(x):
    return np.floor(x).astype(np.int64)


def rint_int(x):
    return np.rint(x).astype(np.int64)


# ---------------------------------------------------------------- objects ---
@pytest.fixture(scope="module")
def obj():
    pos, planted = G.obj_particles()
    return pos, planted, G.obj_mask()


def test_object_mask_and_planted_particles(obj):
    pos, pl, (mask, sy, sz, nn) = obj
    assert mask.shape == (14, 12, 18) and (sy, sz, nn) == (18, 216, 3024)
    assert [int((mask == k).sum()) for k in (1, 2, 3)] == [27, 1, 1] and mask[0, 0, 0] == 3
    ids = lambda p: G.obj_ids(p, mask, sy, sz, nn)
    assert ids(pl.on).tolist() == [1, 1, 1, 2]          # a coordinate exactly on the node's integer
    assert not ids(pl.below).any()                      # one step below it: the neighbouring cell
    assert ids(pl.neg).tolist() == [3, 3, 3, 3]         # (-1, 0) truncates to cell 0
    assert not ids(pl.far).any()
    c = G.trunc_int(pl.far)
    node = c[:, 0] + c[:, 1] * sy + c[:, 2] * sz
    assert node[0] < 0 and node[1] >= nn
    flags, cc, cnt = G.obj_flag(pos, mask, sy, sz, nn)
    assert cc.tolist() == [G.CHUNK, 0, 9]               # a chunk of hits, a chunk without, a partial one
    assert cnt.sum() == cc.sum() and np.all(cnt > 0)
    for row in np.concatenate([pl.on, pl.below, pl.neg, pl.far]):
        assert np.any(np.all(pos == row, axis=1))


def test_object_flag_mutants(obj):
    pos, _, (mask, sy, sz, nn) = obj
    flags, cc, cnt = G.obj_flag(pos, mask, sy, sz, nn)
    # floor for truncation
    f2, c2, n2 = G.obj_flag(pos, mask, sy, sz, nn, to_int=floor_int)
    assert not np.array_equal(f2, flags) and not np.array_equal(c2, cc) and not np.array_equal(n2, cnt)
    # chunk counts taken from slot 0 instead of iStart
    f3, c3, _ = G.obj_flag(pos, mask, sy, sz, nn, first=G.START)
    assert np.array_equal(f3, flags) and not np.array_equal(c3[:len(cc)], cc)
    # no range test: the two far particles would read outside the table
    c = G.trunc_int(pos)
    node = c[:, 0] + c[:, 1] * sy + c[:, 2] * sz
    assert (node < 0).sum() == 1 and (node >= nn).sum() == 1


def test_object_chain_has_holes_and_a_tail(obj):
    """the flags leave work for the back-fill: holes below the survivor count
    and survivors above it, so the survivors' order is not the input's"""
    pos, _, (mask, sy, sz, nn) = obj
    flags, _, _ = G.obj_flag(pos, mask, sy, sz, nn)
    slots, order = M.serial_backfill(flags, G.CENTRE3)
    m = len(slots)
    assert m == G.N_PART - G.CHUNK - 9 and len(order) == G.CHUNK + 9
    assert not np.array_equal(slots, np.flatnonzero(flags == G.CENTRE3))


@pytest.mark.parametrize("n", G.SURFACE_N)
def test_surface_mutants(n):
    c = G.surface_case(n)
    assert len(set(c.idx[c.idx >= 0].tolist())) == int((c.idx >= 0).sum())
    want = G.obj_correct(c.M, c.phiS, c.phiC, c.idx, c.rho)
    live = c.idx >= 0
    if n > 1:
        # M transposed: far outside the bound, and other bits
        mut = G.obj_correct(c.M.T.copy(), c.phiS, c.phiC, c.idx, c.rho)
        assert not same_bits(mut, want)
        _, S = G.obj_correct_ld(c.M, c.phiS, c.phiC)
        d = np.abs(mut - want)[c.idx[live]]
        assert np.max(d / S[live].astype(np.float64)) > GAP
        # rows with idx < 0 must add nothing: a mutant that clamps them to node 0 changes node 0
        assert (~live).any()
    # the restatement meets its own bound against the long-double sum
    ref, S = G.obj_correct_ld(c.M, c.phiS, c.phiC)
    err = np.abs(want[c.idx[live]].astype(LD) - (c.rho[c.idx[live]].astype(LD) + ref[live]))
    assert np.all(err <= (n + 2) * G.EPS * S[live])
    assert np.all(np.abs(c.rho[c.idx[live]]) <= 0.25 * S[live])
    # gather: +0.0, not -0.0 or the node's value, where idx < 0
    g = G.obj_gather(c.grid, c.idx)
    assert same_bits(g[~live], np.zeros(int((~live).sum())))
    # add: only the listed nodes move
    a = G.obj_add(c.grid, c.idx, c.v)
    moved = np.flatnonzero(a != c.grid)
    assert sorted(moved.tolist()) == sorted(c.idx[live].tolist())


# ---------------------------------------------------------------- order 0 ---
@pytest.mark.parametrize("name", list(G.NGP_GEOMS))
def test_ngp_planted_and_mutants(name):
    Tl = G.ngp_local(name)
    nd = len(Tl)
    pos = G.ngp_particles(name)
    assert pos.shape == (G.N_PART, nd)
    j = G.nearest(pos)
    for d in range(nd):
        t = Tl[d]
        assert j[:, d].min() == 0 and j[:, d].max() == t + 1
        for x, node in ((0.0, 0), (0.5, 1), (2.5, 3), (t + 0.5, t + 1), (np.nextafter(2.5, 0.0), 2),
                        (np.nextafter(t + 1.5, 0.0), t + 1), (float(t + 1), t + 1)):
            rows = np.flatnonzero(pos[:, d] == x)
            assert len(rows) >= 1 and np.all(j[rows, d] == node), (d, x)
    rho0 = G.ngp_rho0(Tl)
    assert np.all(rho0 == np.rint(rho0))
    E = G.ngp_field(Tl)
    vel = np.random.default_rng(3).uniform(-0.6, 0.6, size=pos.shape)
    v1, ke, mag = G.ngp_accelerate(pos, vel, E, Tl)
    assert len(ke) == 3
    for literal in (0, 1, 2):
        want = G.ngp_deposit(pos, Tl, literal, rho0)
        assert np.all(want == np.rint(want)) and np.abs(want).max() < 2.0 ** 40
        if nd == 1 and literal == 2:
            assert same_bits(want, rho0)     # (2^0 - 1): nothing to add in 1-D
            continue
        # np.rint for (int)(x + 0.5): 0.5 and 2.5 go to the even node
        assert not same_bits(G.ngp_deposit(pos, Tl, literal, rho0, to_int=rint_int), want)
    assert want.shape == G.slab_shape(Tl)
    v2, ke2, _ = G.ngp_accelerate(pos, vel, E, Tl, to_int=rint_int)
    assert not same_bits(v2, v1)
    # a block that owned other particles (chunks from slot 0 of the arrays): outside the bound
    shifted = vel.astype(LD) * v1.astype(LD)
    other = np.array([shifted[max(b * G.CHUNK - G.START % G.CHUNK, 0):(b + 1) * G.CHUNK - G.START % G.CHUNK].sum()
                      for b in range(3)])
    assert np.all(np.abs(other - ke) > (G.CHUNK + 4) * G.EPS * mag)


def test_ngp_literal_factors_are_small_integers():
    seen = set()
    for name in G.NGP_GEOMS:
        Tl = G.ngp_local(name)
        j = G.nearest(G.ngp_particles(name))
        for literal in (0, 1, 2):
            seen |= set(G.O.literal_factor(j, Tl, literal).astype(np.float64).tolist())
    assert seen <= {0, 1, 2, 3, 4, 6, 7, 8, 14} and {0, 1, 2, 3, 4, 6} <= seen


# ------------------------------------------------------------ device init ---
def test_mixer_known_values():
    """splitmix64's first outputs from state 0 (its published test vector)"""
    inc = 0x9E3779B97F4A7C15
    got = [int(G.mix64(np.array([(k * inc) % 2 ** 64], dtype=np.uint64))[0]) for k in range(3)]
    assert got == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    u = G.uni(G.INIT_SEED, np.arange(100000, dtype=np.uint64))
    assert 0 < u.min() and u.max() < 1 and abs(u.mean() - 0.5) < 0.01


INIT_CASES = [(nd, n) for nd in (1, 2, 3) for n in G.INIT_NGLOBAL]


@pytest.mark.parametrize("nd,n", INIT_CASES)
def test_lattice_partitions(nd, n):
    """every lattice index has exactly one owner, in each decomposition"""
    L = G.INIT_L[nd]
    l = G.lattice_step(L, n)
    one, _ = G.lattice(L, n, l, (0,) * nd, (1,) * nd)
    assert np.array_equal(one, np.arange(n))
    decs = [(1,) * (nd - 1) + (2,)] + ([(2, 1, 2)] if nd == 3 else [])
    for n_sub in decs:
        parts = [G.lattice(L, n, l, sub, n_sub)[0] for sub, _ in G.decomposition(L, n_sub)]
        assert np.array_equal(np.sort(np.concatenate(parts)), np.arange(n))
        if n >= 2047:
            assert all(len(p) for p in parts)
            # interleaved (but in 1-D, where a slab is one run): the compaction has gaps to close
            assert nd == 1 or np.any(np.diff(parts[0]) > 1)


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_init_mutants(nd):
    L = G.INIT_L[nd]
    n = G.INIT_NGLOBAL[-1]
    l = G.lattice_step(L, n)
    n_sub = (1,) * (nd - 1) + (2,)
    (sub0, off0), (sub1, off1) = G.decomposition(L, n_sub)
    want = G.init_species(L, n, l, sub1, n_sub, off1, 1, 1, 1)
    m = len(want.idx)
    assert m > 2048
    xtol = 16 * G.EPS * max(G.INIT_AMP) + G.EPS * np.abs(want.glob)
    vtol = 32 * G.EPS * G.INIT_VTH * want.R + G.EPS * np.abs(want.v)

    def far(a, b, tol, scale):
        return np.max(np.abs(a - b) / scale) > GAP and np.any(np.abs(a - b) > 1e6 * tol)

    # the RNG counter from the local slot
    mut = G.init_species(L, n, l, sub1, n_sub, off1, 1, 1, 1, counter=lambda idx: np.arange(len(idx)))
    assert far(mut.v, want.v, vtol, G.INIT_VTH)
    # a missing 2 pi
    mut = G.init_species(L, n, l, sub1, n_sub, off1, 1, 1, 1, two_pi=False)
    assert far(mut.v, want.v, vtol, G.INIT_VTH)
    mut = G.init_species(L, n, l, sub1, n_sub, off1, 1, 1, 1, mode=tuple(k / (2 * np.pi) for k in G.INIT_MODE))
    assert far(mut.x, want.x, xtol, max(G.INIT_AMP))
    # an unstable compaction: two neighbours swapped inside a chunk
    plain = G.init_species(L, n, l, sub1, n_sub, off1, 1, 0, 0)
    swapped = plain.x.copy()
    swapped[[7, 8]] = swapped[[8, 7]]
    assert not same_bits(swapped, plain.x)
    assert same_bits(np.sort(swapped, axis=0), np.sort(plain.x, axis=0))   # a set comparison would not see it
    # floor and truncation agree on the owner test (x >= 0); another species draws other numbers
    mut = G.init_species(L, n, l, sub1, n_sub, off1, 0, 1, 1)
    assert far(mut.v, want.v, vtol, G.INIT_VTH)
    assert same_bits(G.init_species(L, n, l, sub1, n_sub, off1, 1, 0, 0).v, np.zeros((m, nd)))


# ------------------------------------------------------- rescaling chains ---
@pytest.mark.parametrize("ns", G.CHAIN_NS)
def test_chain_mutants(ns):
    c = G.chain_inputs(ns, 1023)
    want = G.rho_combine(c.acc, c.q)
    assert np.all(np.abs(np.log2(np.abs(c.q))) % 1 != 0)       # no powers of two
    if ns > 1:
        # the chain multiplied in the other order
        r = c.acc[0].copy()
        for s in range(1, ns):
            r = r * (c.q[s - 1] * (1.0 / c.q[s])) + c.acc[s]
        assert not same_bits(r * c.q[ns - 1], want)
        # a division in place of the reciprocal
        r = c.acc[0].copy()
        for s in range(1, ns):
            r = (r * c.q[s - 1]) / c.q[s] + c.acc[s]
        assert not same_bits(r * c.q[ns - 1], want)
    # the plain sum of q_s acc_s is close, and other bits
    plain = sum(c.q[s] * c.acc[s] for s in range(ns))
    assert np.allclose(plain, want, rtol=1e-12, atol=1e-12)
    if ns > 1:
        assert not same_bits(plain, want)
    for pre in G.CHAIN_PRE:
        Es = G.field_chain_all(c.E, c.qm, c.mq, pre)
        assert Es.shape == (ns, 1023)
        assert same_bits(Es[0], (c.E * pre) * c.qm[0])
        if ns > 1:
            v = c.E * pre
            out = [v * c.qm[0]]
            for s in range(1, ns):
                v = v * (c.qm[s - 1] * c.mq[s - 1])
                out.append(v * c.qm[s])
            assert not same_bits(np.stack(out), Es)
            assert not same_bits(Es[1], (c.E * pre) * c.qm[1])


# ------------------------------------------------------- velocity assert ---
@pytest.mark.parametrize("nd", [1, 2, 3])
def test_vel_assert_mutants(nd):
    cases = G.vel_cases(nd)
    assert len(cases) == 1 + 3 * 2 * nd
    for name, vel, bad in cases:
        assert G.vel_assert(vel, G.MAX_VEL, 0) == int(bad) and G.vel_assert(vel, G.MAX_VEL, 6) == 6 + int(bad), name
        ge = bool(np.any(vel >= G.MAX_VEL))                 # >= for >
        mag = bool(np.any(np.abs(vel) > G.MAX_VEL))         # magnitude for signed
        if name.startswith("equal"):
            assert ge and not bad
        if name.startswith("negative"):
            assert mag and not bad
        if name.startswith("above"):
            assert bad and np.count_nonzero(vel > G.MAX_VEL) == 1
