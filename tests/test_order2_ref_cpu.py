"""The restatement tests/order2_ref.py itself (no GPU): the properties of the
quadratic spline that pin the reference the GPU tests compare against.

Bounds are in long double ulps (e = order2_ref.EPS_LD), from the roundings of
the restatement.  One dimension: 0.5 -+ dl rounds once, its square once, the
half is exact: w[0], w[2] <= 1/2 err by <= 1.5 e; dl^2 <= 1/4 and the
subtraction from 0.75 round once each: w[1] errs by <= 1 e.  So the three
weights sum to 1 within 4 e plus two additions: 6 e.  A node weight is a
product of nd of them (nd - 1 roundings, the factor 1 is exact).
"""
import numpy as np
import pytest

import order2_ref as O

LD = O.LD
E = O.EPS_LD
GEOMS = [(8,), (8, 6), (8, 6, 5)]


@pytest.fixture(scope="module", params=GEOMS, ids=["1d", "2d", "3d"])
def case(request):
    T = request.param
    pos = O.particles(T, 600, 11 + len(T))
    pos.setflags(write=False)
    return T, pos


def test_weights_sum_to_one(case):
    T, pos = case
    nd = len(T)
    _, w1 = O.split(pos, T)
    assert np.all(w1 >= 0)
    assert np.max(np.abs(w1.sum(axis=-1) - 1)) <= 6 * E
    # nodes: the product of nd sums within 6 e each, nd - 1 roundings per
    # product and 3^nd - 1 additions of terms that sum to about 1
    w = O.node_weights(w1)
    assert w.shape == (len(pos), 3 ** nd)
    assert np.max(np.abs(w.sum(axis=1) - 1)) <= (6 * nd + (nd - 1) + 3 ** nd) * E


def test_first_moment_is_the_position(case):
    T, pos = case
    j, w1 = O.split(pos, T)
    for d in range(len(T)):
        nodes = (j[:, d, None] - 1 + np.arange(3)).astype(LD)
        m = (w1[:, d] * nodes).sum(axis=1)
        # three weights within 1.5 e times nodes <= T + 1, three products and two additions
        lim = (3 * 1.5 + 3 + 2) * (T[d] + 1) * E
        inside = (pos[:, d] >= 0.5) & (pos[:, d] < T[d] + 0.5)
        assert inside.sum() > 500
        assert np.max(np.abs(m[inside] - pos[inside, d].astype(LD))) <= lim


@pytest.mark.parametrize("T", [3, 8, 20])
def test_clamp_is_continuous(T):
    top = T + 0.5
    below = np.nextafter(top, 0.0)
    j, w = O.split(np.array([[top], [below], [0.5], [np.nextafter(0.5, 0.0)], [np.nextafter(0.5, 1.0)]]), (T,))
    assert j[:, 0].tolist() == [T, T, 1, 1, 1]
    # x = T + 0.5 is clamped to j = T with dl = 1/2: nodes T, T + 1 get 1/2 each,
    # what dl = -1/2 about the unclamped j = T + 1 gives them
    assert w[0, 0].tolist() == [0.0, 0.5, 0.5]
    _, free = O.split(np.array([[top]]), (T + 1,))
    assert free[0, 0].tolist() == [0.5, 0.5, 0.0]
    assert w[2, 0].tolist() == [0.5, 0.5, 0.0]
    # one float64 step in x moves a weight by |dw/dx| <= 1 times that step, plus the 1.5 e of each weight
    assert np.max(np.abs(w[0, 0] - w[1, 0])) <= (top - below) + 3 * E
    for other in (3, 4):
        step = abs(0.5 - [0, 0, 0, np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0)][other])
        assert np.max(np.abs(w[2, 0] - w[other, 0])) <= step + 3 * E


@pytest.mark.parametrize("literal", [0])
def test_total_deposited_is_the_particle_count(case, literal):
    T, pos = case
    n, nd = pos.shape
    ref = O.deposit(pos, T, literal)
    assert ref.M.shape == O.padded_shape(T)
    assert int(ref.k.sum()) <= n * 3 ** nd
    # each particle's nodes sum to 1 within the bound above; n 3^nd terms added one by one
    lim = ((6 * nd + (nd - 1) + 3 ** nd) + n * 3 ** nd) * n * E
    assert abs(ref.M.sum() - n) <= lim
    s = O.slab(ref, T)
    assert s.M.shape == tuple([T[-1] + 2] + [T[d] for d in range(nd - 2, -1, -1)])
    assert abs(s.M.sum() - n) <= lim
    f = O.folded(s, T[-1])
    assert abs(f.M.sum() - n) <= lim and int(f.k.sum()) == int(ref.k.sum())


def test_literal_factors():
    """literal 1 counts a periodic ghost node 2^g times; literal 2 is what a
    second fold still misses: plain + literal 2 folded once more = literal 1
    folded twice, node by node (one rank, slab self-periodic)"""
    T = (4, 3, 3)
    pos = O.particles(T, 200, 5)
    nl = T[-1]
    plain, lit1, lit2 = (O.slab(O.deposit(pos, T, l), T).M for l in (0, 1, 2))

    def fold_keep(a):
        a = a.copy()
        a[nl] += a[0]
        a[1] += a[nl + 1]
        return a
    twice = fold_keep(fold_keep(lit1))[1:nl + 1]
    second = fold_keep(fold_keep(plain) + lit2)[1:nl + 1]
    scale = np.abs(twice).max()
    assert np.max(np.abs(twice - second)) <= 64 * 200 * E * scale
