"""A plain numpy restatement of the velocity moments (pinc_hip_moments,
include/pinc_hip.h).  No GPU.

For species particles (x_p, v_p), node j and the CIC weight w_j(x_p) (the
2^nd products of dec_d = x_d - (int)x_d and 1 - dec_d, push_ref._weights_ld):

    M[0]           = sum_p w_j(x_p)
    M[1 + i]       = sum_p w_j(x_p) v_p,i          i < nd
    M[1 + nd + k]  = sum_p w_j(x_p) v_p,i v_p,j    i <= j, row-major upper
                     triangle (xx xy xz yy yz zz; xx xy yy; xx)

Weights, velocity factors, terms and sums are np.longdouble.  The grid is
push_ref's slab layout (slab_shape, _corner_nodes) with NM values per node,
value-major.  Per node and moment the reference gives the value, the sum of
the |terms| and the count k of contributions (weights that are not zero),
from which the tests take the bound

    |M - M_ref| <= (k + 8) eps sum|terms|,   exactly 0 where k = 0:

k roundings from the sum in any order, at most 8 from the fp64 weight (2 or
3), the velocity product (1), the term (1) and the adds of the flush and of
the halo fold (3).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import push_ref as R

LD = np.longdouble
EPS = np.finfo(np.float64).eps


def n_moments(nd):
    return 1 + nd + nd * (nd + 1) // 2


def factors(vel):
    """(n, NM) long double: 1, v_i, v_i v_j (i <= j)"""
    n, nd = vel.shape
    v = vel.astype(LD)
    cols = [np.ones(n, dtype=LD)] + [v[:, d] for d in range(nd)]
    cols += [v[:, i] * v[:, j] for i in range(nd) for j in range(i, nd)]
    return np.stack(cols, axis=1)


def moments_reference(pos, vel, geom):
    """M, A = sum|terms| (slab_shape + (NM,), long double) and k (slab_shape,
    int64) of the particles pos, vel (n, nd) on one rank's slab of true sizes
    geom; ghost planes unfolded."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    vel = np.ascontiguousarray(vel, dtype=np.float64)
    geom = tuple(int(t) for t in geom)
    nd = len(geom)
    nm = n_moments(nd)
    shape = R.slab_shape(geom)
    M = np.zeros(shape + (nm,), dtype=LD)
    A = np.zeros(shape + (nm,), dtype=LD)
    k = np.zeros(shape, dtype=np.int64)
    if pos.shape[0]:
        cell, w = R._weights_ld(pos)
        f = factors(vel)
        for c in range(1 << nd):
            idx = R._corner_nodes(geom, cell, c)
            t = w[:, c, None] * f
            np.add.at(M, idx, t)
            np.add.at(A, idx, np.abs(t))
            np.add.at(k, idx, (w[:, c] != 0).astype(np.int64))
    return SimpleNamespace(M=M, A=A, k=k)


def fold(a, nloc):
    """gHaloOp(addSlice, FROMHALO) of a one-rank slab (slab dimension first):
    ghost plane nloc + 1 into plane 1, ghost plane 0 into plane nloc; returns
    the true planes."""
    a = a.copy()
    a[1] += a[nloc + 1]
    a[nloc] += a[0]
    return a[1:nloc + 1]


def folded(ref, nloc):
    return SimpleNamespace(M=fold(ref.M, nloc), A=fold(ref.A, nloc), k=fold(ref.k, nloc))


def add(a, b):
    """the reference of two accumulating calls"""
    return SimpleNamespace(M=a.M + b.M, A=a.A + b.A, k=a.k + b.k)


def check(M, ref, what=""):
    """asserts the bound above for a device result M (float64, ref.M's shape);
    prints the worst error over the bound first"""
    M = np.asarray(M)
    assert M.shape == ref.M.shape, (what, M.shape, ref.M.shape)
    err = np.abs(M.astype(LD) - ref.M)
    lim = (ref.k[..., None] + 8) * EPS * ref.A
    touched = np.broadcast_to(ref.k[..., None] > 0, M.shape)
    worst = float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1), 0), initial=0.0))
    print(f"{what}: moments error / bound {worst:.3f}")
    assert np.all(M[~touched] == 0), what
    assert np.all(err <= lim), (what, worst)
