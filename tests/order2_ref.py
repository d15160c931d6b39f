"""A numpy restatement of the order-2 (quadratic spline) weighting of
include/pinc_hip.h (pinc_hip_deposit_tsc, pinc_hip_accelerate_tsc).  No GPU.

Per dimension d, T_d true nodes (nloc in the slab dimension, the last one):

    j    = min(max((int)(x_d + 0.5), 1), T_d)
    dl   = x_d - j
    w[0] = 0.5 (0.5 - dl)^2     node j - 1
    w[1] = 0.75 - dl^2          node j
    w[2] = 0.5 (0.5 + dl)^2     node j + 1

j and dl are computed in float64 as the kernels do: x + 0.5 rounds the same
way, and x - j is exact (|x - j| <= 1/2 <= x, so the difference is a multiple
of x's ulp that fits the format).  The weights, their products and every sum
are np.longdouble.

Layouts.  T is the tuple of true sizes, x first.  A padded array has numpy
shape (T[nd-1] + 2, ..., T[0] + 2) (ghost node 0 and T + 1 in every
dimension); a slab array is push_ref.slab_shape(T): the last dimension keeps
its ghost planes, the others are periodic and stored without ghosts (padded
node p at (p - 1) mod T).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps
EPS_LD = np.finfo(LD).eps


def split(pos, T):
    """nearest true node j (n, nd) int64 and the one-dimensional weights
    (n, nd, 3) long double of nodes j - 1, j, j + 1"""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    Tn = np.asarray(T, dtype=np.int64)
    j = np.clip((pos + 0.5).astype(np.int64), 1, Tn)
    dl = (pos - j).astype(LD)
    half, q = LD(0.5), LD(0.75)
    w = np.stack([half * ((half - dl) * (half - dl)), q - dl * dl, half * ((half + dl) * (half + dl))], axis=-1)
    return j, w


def stencil(nd):
    """the 3^nd stencil indices (i_0, .., i_nd-1), node c = sum i_d 3^d"""
    return [tuple((c // 3 ** d) % 3 for d in range(nd)) for c in range(3 ** nd)]


def node_weights(w1):
    """(n, 3^nd) products of the one-dimensional weights (n, nd, 3)"""
    n, nd, _ = w1.shape
    out = np.ones((n, 3 ** nd), dtype=LD)
    for c, idx in enumerate(stencil(nd)):
        for d in range(nd - 1, -1, -1):
            out[:, c] = w1[:, d, idx[d]] * out[:, c]
    return out


def literal_factor(p, T, literal):
    """literal_node_factor of k_particles.hip for padded node coordinates p
    (n, nd): 1 plain; literal 1: 2^g, g the ghost coordinates in the non-slab
    dimensions; literal 2: (2^g - 1), doubled on a slab ghost plane"""
    n, nd = p.shape
    if not literal:
        return np.ones(n, dtype=LD)
    m = np.ones(n, dtype=LD)
    for d in range(nd - 1):
        m = m * np.where((p[:, d] == 0) | (p[:, d] == T[d] + 1), 2, 1)
    if literal == 1:
        return m
    mz = np.where((p[:, nd - 1] == 0) | (p[:, nd - 1] == T[nd - 1] + 1), 2, 1)
    return (m - 1) * mz


def padded_shape(T):
    return tuple(t + 2 for t in reversed(T))


def deposit(pos, T, literal=0):
    """per padded node: M the sum of the weights, A the sum of their
    magnitudes, k the number of terms that are not zero"""
    nd = len(T)
    j, w1 = split(pos, T)
    w = node_weights(w1)
    M = np.zeros(padded_shape(T), dtype=LD)
    A = np.zeros(padded_shape(T), dtype=LD)
    k = np.zeros(padded_shape(T), dtype=np.int64)
    for c, idx in enumerate(stencil(nd)):
        p = j - 1 + np.array(idx, dtype=np.int64)
        assert p.min() >= 0 and np.all(p <= np.asarray(T) + 1)
        term = w[:, c] * literal_factor(p, T, literal)
        at = tuple(p[:, d] for d in range(nd - 1, -1, -1))
        np.add.at(M, at, term)
        np.add.at(A, at, np.abs(term))
        np.add.at(k, at, (term != 0).astype(np.int64))
    return SimpleNamespace(M=M, A=A, k=k)


def to_slab(a, T):
    """a padded array in the slab layout: the ghost nodes of the periodic
    (non-slab) dimensions added to the true nodes they stand for"""
    nd = len(T)
    for d in range(nd - 1):
        ax = nd - 1 - d
        a = np.moveaxis(a, ax, 0).copy()
        a[T[d]] += a[0]
        a[1] += a[T[d] + 1]
        a = np.moveaxis(a[1:T[d] + 1], 0, ax)
    return a


def slab(ref, T):
    return SimpleNamespace(M=to_slab(ref.M, T), A=to_slab(ref.A, T), k=to_slab(ref.k, T))


def fold(a, nloc):
    """the slab fold of one self-periodic rank: plane 0 into nloc, plane
    nloc + 1 into 1; the true planes"""
    a = a.copy()
    a[nloc] += a[0]
    a[1] += a[nloc + 1]
    return a[1:nloc + 1]


def folded(ref, nloc):
    return SimpleNamespace(M=fold(ref.M, nloc), A=fold(ref.A, nloc), k=fold(ref.k, nloc))


def charge_chain(refs, q):
    """rho of the species' slab (or folded) sums refs with charges q: the
    device chain gZero; per species gMul(1/q_s), deposit, gMul(q_s) is
    sum_s q_s dep_s.  M the value, A = sum_s |q_s| A_s, k = sum_s k_s."""
    M = sum(LD(qs) * r.M for qs, r in zip(q, refs))
    A = sum(abs(LD(qs)) * r.A for qs, r in zip(q, refs))
    k = sum(r.k for r in refs)
    return SimpleNamespace(M=M, A=A, k=k)


def slab_index(p, T):
    """index tuple (numpy order) of padded node coordinates p (n, nd) in a slab array"""
    nd = len(T)
    return tuple(p[:, d] if d == nd - 1 else (p[:, d] - 1) % T[d] for d in range(nd - 1, -1, -1))


def gather(pos, Es, T):
    """dv (n, nd) = sum over the 3^nd nodes of w Es[node], and sum |w Es|,
    both long double; Es a slab array with nd values per node"""
    nd = len(T)
    j, w1 = split(pos, T)
    w = node_weights(w1)
    dv = np.zeros(pos.shape, dtype=LD)
    mag = np.zeros(pos.shape, dtype=LD)
    for c, idx in enumerate(stencil(nd)):
        p = j - 1 + np.array(idx, dtype=np.int64)
        t = w[:, c, None] * Es[slab_index(p, T)].astype(LD)
        dv += t
        mag += np.abs(t)
    return dv, mag


# ------------------------------------------------------------- inputs -----
def planted(T, rng):
    """positions (m, nd) whose coordinates, per dimension, run through the
    rule's edges: exactly 0.5, nextafter(T + 0.5, 0), exactly T + 0.5 (the
    clamp), integers, half-integers and both neighbours of a half-integer;
    the other coordinates uniform"""
    nd = len(T)
    rows = []
    for d in range(nd):
        t = float(T[d])
        h = 1.5 if T[d] < 3 else 2.5
        vals = [0.5, np.nextafter(t + 0.5, 0.0), t + 0.5, 1.0, t, float((T[d] + 1) // 2), h, t - 0.5 if T[d] > 1 else 1.5,
                np.nextafter(h, 0.0), np.nextafter(h, 10.0), np.nextafter(0.5, 1.0), np.nextafter(1.0, 0.0)]
        for v in vals:
            p = [0.5 + rng.random() * T[e] for e in range(nd)]
            p[d] = v
            rows.append(p)
    return np.array(rows)


def particles(T, n, seed):
    """n positions: the planted ones, then uniform in [0.5, T + 0.5)"""
    rng = np.random.default_rng(seed)
    nd = len(T)
    pl = planted(T, rng)
    Tn = np.asarray(T, dtype=np.float64)
    u = 0.5 + rng.random((n - len(pl), nd)) * Tn
    u = np.minimum(u, np.nextafter(Tn + 0.5, 0.0))
    return np.concatenate([pl, u])


def node_sorted(pos, T):
    """pos ordered by nearest node (x fastest)"""
    j, _ = split(pos, T)
    key = np.zeros(len(pos), dtype=np.int64)
    for d in range(len(T) - 1, -1, -1):
        key = key * (T[d] + 2) + j[:, d]
    return pos[np.argsort(key, kind="stable")]
