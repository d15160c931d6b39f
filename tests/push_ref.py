"""A plain numpy reference for one fused push (pinc_hip_push,
include/pinc_hip.h) and for the sort key of the in-push sort.  No GPU.

push_reference restates, per particle and in this order:

  1. kick     puInterp3D1 / puInterpND1 weights at the pre-move position,
              v' = v + dv, KE term v.(v + dv)
  2. drift    x' = x + v'
  3. classify digit_d = 1 - (x' < lo_d) + (x' >= up_d)
  4. wrap     wrap_mask bit d: x'_d += (1 - digit_d) T_d in place, digit_d = 1
  5. flag     ne = sum_d digit_d 3^d
  6. sink     a stayer whose cell's lower node has an object id > 0 is flagged
              NE_SINK and counted per id
  7. deposit  CIC weights of every particle whose flag is the centre, into the
              slab layout

Positions, velocities and flags are float64 with exactly these operations
(the kick in the reference's expression order: the nested form of
puInterp3D1 in 3-D, puInterpND1Inner's recursion order otherwise).  dv, the
deposited weights and the KE sum are np.longdouble: for positions >= 0.5
the fractions dec = x - (int)x and 1 - dec are multiples of 2^-53 below 1,
so the long double factors are exact and each product errs by 2^-64.

Slab layout (single rank): the last dimension keeps its ghost planes
(nloc + 2 planes, stored as they are), the others are periodic and stored
without ghosts: padded node j of such a dimension is stored at (j - 1) mod T.
A 3-D slab is [nloc + 2][Ty][Tx] (numpy shape, x fastest); E holds nd values
per node, value-major.

geom is the tuple of true sizes per dimension (x first); one rank, so the
slab dimension's nloc is its last entry.  thr is [lo(nd), up(nd), hi(nd)]
as MpiInfo.thresholds.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

PINC_CHUNK = 2048
NE_SINK = 27
LD = np.longdouble


def slab_shape(geom):
    """numpy shape of a scalar slab grid."""
    nd = len(geom)
    return (geom[nd - 1] + 2,) + tuple(geom[d] for d in range(nd - 2, -1, -1))


def centre(nd):
    return sum(3 ** d for d in range(nd))


def _storage(geom, d, j):
    """storage coordinate of padded node coordinates j along dimension d"""
    return j if d == len(geom) - 1 else (j - 1) % geom[d]


def _corner_nodes(geom, cell, c):
    """index tuple (numpy order, slab dimension first) of corner c of cells
    `cell` (n, nd), corner bit d = the upper node along dimension d"""
    nd = len(geom)
    return tuple(_storage(geom, d, cell[:, d] + ((c >> d) & 1)) for d in range(nd - 1, -1, -1))


def _fractions(x, dtype):
    cell = x.astype(np.int64)               # (int)x, x >= 0
    dec64 = x - cell                        # exact
    dec = dec64.astype(dtype)
    return cell, dec, 1 - dec


def kick_f64(pos, Es, geom):
    """dv in float64, the reference's expression order (pusher.c:1089-1162):
    the kick the kernels restate without contraction."""
    n, nd = pos.shape
    cell, dec, comp = _fractions(pos, np.float64)
    f = [Es[_corner_nodes(geom, cell, c)] for c in range(1 << nd)]   # (n, nd) each
    if nd == 3:
        x, y, z = (dec[:, d, None] for d in range(3))
        xc, yc, zc = (comp[:, d, None] for d in range(3))
        return (zc * (yc * (xc * f[0] + x * f[1]) + y * (xc * f[2] + x * f[3])) +
                z * (yc * (xc * f[4] + x * f[5]) + y * (xc * f[6] + x * f[7])))
    dv = np.zeros((n, nd))
    for c in range(1 << (nd - 1)):
        fac = np.ones(n)
        cc = 0
        for d in range(nd - 1, 0, -1):
            bit = (c >> (d - 1)) & 1
            fac = (dec[:, d] if bit else comp[:, d]) * fac
            cc |= bit << d
        dv = dv + (comp[:, 0] * fac)[:, None] * f[cc]
        dv = dv + (dec[:, 0] * fac)[:, None] * f[cc | 1]
    return dv


def _weights_ld(x):
    """the 2^nd CIC weights (n, 2^nd) in long double and the cells"""
    n, nd = x.shape
    cell, dec, comp = _fractions(x, LD)
    w = np.ones((n, 1 << nd), dtype=LD)
    for c in range(1 << nd):
        for d in range(nd):
            w[:, c] *= dec[:, d] if (c >> d) & 1 else comp[:, d]
    return cell, w


def kick_ld(pos, Es, geom):
    """dv in long double: sum over the corners of weight times E"""
    n, nd = pos.shape
    cell, w = _weights_ld(pos)
    dv = np.zeros((n, nd), dtype=LD)
    for c in range(1 << nd):
        dv += w[:, c, None] * Es[_corner_nodes(geom, cell, c)].astype(LD)
    return dv


def push_reference(pos, vel, Es, geom, thr, wrap_mask, kick, obj=None):
    """One push of n particles.  pos, vel: (n, nd) float64; Es: slab E
    (slab_shape + (nd,)) or None without kick; obj: None or a mapping with
    `inside` (uint8 ids of the padded nodes, numpy shape [Tz+2][Ty+2][Tx+2]),
    `lo`, `hi` (inclusive bounding box, padded node coordinates, x first) and
    `n` (number of ids)."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    vel = np.ascontiguousarray(vel, dtype=np.float64)
    n, nd = pos.shape
    geom = tuple(int(t) for t in geom)
    thr = np.asarray(thr, dtype=np.float64)
    lo, up, hi = thr[:nd], thr[nd:2 * nd], thr[2 * nd:3 * nd]
    T = (hi - 1.0 + 0.5).astype(np.int64)
    # 1. kick
    if kick:
        v_ld = vel.astype(LD) + kick_ld(pos, Es, geom)
        terms = vel.astype(LD) * v_ld
        v64 = vel + kick_f64(pos, Es, geom)
    else:
        v_ld = vel.astype(LD)
        terms = np.zeros((n, nd), dtype=LD)
        v64 = vel.copy()
    # 2. drift
    x = pos + v64
    changed = np.any(x.astype(np.int64) != pos.astype(np.int64), axis=1)
    # 3.-5. classify, wrap, flag
    dig = 1 - (x < lo).astype(np.int64) + (x >= up).astype(np.int64)
    for d in range(nd):
        if (wrap_mask >> d) & 1:
            x[:, d] = np.where(dig[:, d] != 1, x[:, d] + ((1 - dig[:, d]) * T[d]).astype(np.float64), x[:, d])
            dig[:, d] = 1
    flag = (dig * 3 ** np.arange(nd)).sum(axis=1)
    c0 = centre(nd)
    # 6. object sink
    obj_count = None
    if obj is not None:
        cell = x.astype(np.int64)
        inbb = flag == c0
        for d in range(nd):
            inbb &= (cell[:, d] >= obj["lo"][d]) & (cell[:, d] <= obj["hi"][d])
        ids = np.zeros(n, dtype=np.int64)
        cb = cell[inbb]
        ids[inbb] = obj["inside"][tuple(cb[:, d] for d in range(nd - 1, -1, -1))]
        flag = np.where(ids > 0, NE_SINK, flag)
        obj_count = np.bincount(ids[ids > 0] - 1, minlength=obj["n"])
    # 7. deposit of the stayers
    stay = flag == c0
    rho = np.zeros(slab_shape(geom), dtype=LD)
    contrib = np.zeros(slab_shape(geom), dtype=np.int64)
    cell, w = _weights_ld(x[stay])
    for c in range(1 << nd):
        idx = _corner_nodes(geom, cell, c)
        np.add.at(rho, idx, w[:, c])
        np.add.at(contrib, idx, (w[:, c] > 0).astype(np.int64))
    nchunks = (n + PINC_CHUNK - 1) // PINC_CHUNK
    return SimpleNamespace(
        x=x, v=v_ld, v64=v64, flag=flag.astype(np.uint8), changed=changed, rho=rho, contrib=contrib,
        ke=terms.sum(), ke_abs=np.abs(terms).sum(),
        chunk_emig=np.bincount(np.nonzero(~stay)[0] // PINC_CHUNK, minlength=nchunks),
        moved=int(np.count_nonzero(stay & changed)), emig_total=int(np.count_nonzero(~stay)),
        obj_count=obj_count)


def tile_geo(geom, tile_width):
    """tiles per dimension, largest cell index per dimension, log2 brick
    extents and the number of keys of the tiled layout (make_tile_geo)"""
    nd = len(geom)
    lw = 0
    while (1 << lw) < tile_width:
        lw += 1
    brick = (1 << lw) == tile_width
    nt = [(t + 1) // tile_width + 1 for t in geom]
    cmax = [t + 1 for t in geom]
    bs = [lw if brick and d < nd - 1 else 0 for d in range(nd)]
    return nt, cmax, bs, int(np.prod(nt)) * tile_width ** nd


def cell_keys(c, geom, tile_width):
    """tile_key_of: the sort key of clamped cell coordinates c (n, nd): tiles
    along a serpentine (x rows alternate direction, y columns alternate per
    z plane), the slab layers of odd tiles reversed, x fastest in a tile."""
    n, nd = c.shape
    tw = tile_width
    nt = tile_geo(geom, tw)[0]
    t = c // tw
    inn = c - t * tw
    if nd == 1:
        tile = t[:, 0]
    elif nd == 2:
        tile = t[:, 1] * nt[0] + np.where(t[:, 1] & 1, nt[0] - 1 - t[:, 0], t[:, 0])
    else:
        ty = np.where(t[:, 2] & 1, nt[1] - 1 - t[:, 1], t[:, 1])
        r = t[:, 2] * nt[1] + ty
        tile = r * nt[0] + np.where(r & 1, nt[0] - 1 - t[:, 0], t[:, 0])
    if nd > 1:
        inn[:, nd - 1] = np.where(tile & 1, tw - 1 - inn[:, nd - 1], inn[:, nd - 1])
    cellk = np.zeros(n, dtype=np.int64)
    for d in range(nd):
        cellk += inn[:, d] * tw ** d
    return tile * tw ** nd + cellk


def brick_keys(pos, vel, geom, tile_width):
    """brick_first_key(sort_cell(x, v)): the key of the first cell of the
    brick (one layer of a tile, tw^(nd-1) cells) holding the cell of x + v,
    clamped to the grid."""
    n, nd = pos.shape
    _, cmax, bs, _ = tile_geo(geom, tile_width)
    c = (pos + vel).astype(np.int64)        # (int)(x + v)
    f = np.empty_like(c)
    for d in range(nd):
        f[:, d] = (np.clip(c[:, d], 0, cmax[d]) >> bs[d]) << bs[d]
    return cell_keys(f, geom, tile_width)


# ------------------------------------------------------------- inputs -----
# The generators of tests/test_gpu_push_kernel.py, here so that the CPU tests
# check the error bounds on the same inputs.  Thresholds at half a cell:
# [0.5, T + 0.5), frame [0, T + 1].  With a kick the input speeds stay below
# 0.95 - E_MAX, so |v'| <= 0.95 < maxVel = 1.
E_MAX = 0.25
V_MAX = 0.95


def thresholds(geom):
    nd = len(geom)
    return np.array([0.5] * nd + [t + 0.5 for t in geom] + [t + 1.0 for t in geom])


def random_E(geom, rng, wrap_mask):
    """uniform in [-E_MAX, E_MAX].  With the slab dimension wrapped in place
    (one rank) the slab's ghost planes are the periodic copies the host's E
    has (plane 0 = plane nloc, plane nloc + 1 = plane 1); otherwise they are
    a neighbour's values: independent."""
    nd = len(geom)
    E = rng.uniform(-E_MAX, E_MAX, size=slab_shape(geom) + (nd,))
    if (wrap_mask >> (nd - 1)) & 1:
        E[0] = E[geom[nd - 1]]
        E[geom[nd - 1] + 1] = E[1]
    return E


def uniform_particles(geom, n, rng, vmax):
    """order (a): uniform over [lo, up) with |v_d| <= vmax"""
    nd = len(geom)
    thr = thresholds(geom)
    pos = thr[:nd] + rng.random((n, nd)) * (thr[nd:2 * nd] - thr[:nd])
    pos = np.minimum(pos, np.nextafter(thr[nd:2 * nd], -np.inf))
    return pos, rng.uniform(-vmax, vmax, size=(n, nd))


def cell_sorted(pos, vel, geom, tile_width):
    """the particles in the order of their cell's sort key (what
    pinc_hip_sort_tiles produces, up to the order inside a cell)"""
    nd = len(geom)
    c = np.clip(pos.astype(np.int64), 0, np.array(geom) + 1)
    o = np.argsort(cell_keys(c, geom, tile_width), kind="stable")
    return pos[o], vel[o]


def generate(order, geom, n, kick, seed, tile_width=4):
    """orders a (uniform, fast), b (cell order, |v| <= 0.05), c (first half
    as b, second half as a)"""
    rng = np.random.default_rng(seed)
    vfast = V_MAX - E_MAX if kick else V_MAX
    if order == "a":
        return uniform_particles(geom, n, rng, vfast)
    pos, vel = uniform_particles(geom, n, rng, 0.05)
    pos, vel = cell_sorted(pos, vel, geom, tile_width)
    if order == "c":
        h = n // 2
        pa, va = uniform_particles(geom, n - h, rng, vfast)
        pos = np.concatenate([pos[:h], pa])
        vel = np.concatenate([vel[:h], va])
    return pos, vel


def edge_particles(geom):
    """hand-placed particles at dyadic values (every sum exact): x' on lo, on
    up, one ulp below each, x on a node, v = 0, two and three faces crossed
    at a corner.  (pos, vel), nd columns; the other coordinates mid-domain."""
    nd = len(geom)
    lo, up = 0.5, geom[0] + 0.5
    mid = [float(t // 2) + 0.25 for t in geom]
    rows = []

    def add(x0, v0, others=None):
        p = list(mid)
        v = [0.0] * nd
        p[0], v[0] = x0, v0
        for d, (xd, vd) in (others or {}).items():
            if d < nd:
                p[d], v[d] = xd, vd
        rows.append((p, v))

    add(1.0, -0.5)                                         # x' == lo: stays
    add(up - 0.5, 0.5)                                     # x' == up: leaves upward
    add(lo, -2.0 ** -54)                                   # x' = nextafter(lo, -inf): leaves downward
    add(np.nextafter(up, -np.inf) - 0.25, 0.25)            # x' = nextafter(up, -inf): stays
    add(3.0, 0.0)                                          # on a node, weights exactly 1 and 0
    add(2.5, 0.0)                                          # v = 0
    add(0.75, -0.5, {1: (0.75, -0.5)})                     # a corner: two faces at once
    add(0.75, -0.5, {1: (0.75, -0.5), 2: (geom[-1] + 0.25, 0.5)})   # three faces (3-D)
    pos = np.array([r[0] for r in rows])
    vel = np.array([r[1] for r in rows])
    assert np.all(pos[:, 0] + vel[:, 0] == np.array([lo, up, np.nextafter(lo, -np.inf), np.nextafter(up, -np.inf),
                                                     3.0, 2.5, 0.25, 0.25]))
    return pos, vel
