"""Plain numpy restatement of the multigrid operators of k_mg.hip, on
periodic grids stored [z][y][x] (an nd-dimensional array, x last).  No
project code.

Every function takes a dtype.  With np.float64 each value is formed in the
kernels' expression order (k_mg.hip is compiled without contraction, so the
device's values can be compared with these bit for bit); with np.longdouble
the same formulas are the high-precision yardstick.  Only sums over a whole
grid (the means of the neutralisations) have no fixed order.
"""
import numpy as np

F64 = np.float64
LD = np.longdouble


def _ax(nd, d):
    """array axis of dimension d (0 = x)"""
    return nd - 1 - d


def _up(a, d):
    """a at the periodic neighbour +1 along dimension d"""
    return np.roll(a, -1, _ax(a.ndim, d))


def _dn(a, d):
    return np.roll(a, 1, _ax(a.ndim, d))


def colour_mask(shape, colour):
    """points whose coordinates sum to colour (mod 2)"""
    return (np.indices(shape).sum(0) & 1) == colour


def gs_colour(a, rho, colour, nd, gs3d, mu=0, dtype=F64):
    """One colour pass of the red-black Gauss-Seidel smoother (k_gs_pass).
    The grid is stored raw; every read of the other colour is (raw - mu).
    gs3d: (1/6) (x+ + x- + y+ + y- + z+ + z- + rho), left to right; else per
    dimension v += up + dn, then + rho, then times 1/(2 nd)."""
    a = np.asarray(a, dtype)
    rho = np.asarray(rho, dtype)
    assert a.ndim == nd
    s = a - dtype(mu)
    if gs3d:
        assert nd == 3
        v = (dtype(1) / dtype(6)) * (_up(s, 0) + _dn(s, 0) + _up(s, 1) + _dn(s, 1) + _up(s, 2) + _dn(s, 2) + rho)
    else:
        v = np.zeros_like(a)
        for d in range(nd):
            v = v + (_up(s, d) + _dn(s, d))
        v = v + rho
        v = v * (dtype(1) / dtype(2 * nd))
    return np.where(colour_mask(a.shape, colour), v, a)


def materialize(a, last, mu_a, mu_b, dtype=F64):
    """The pending means applied after the last pass (k_gs_materialize): the
    colour of the last pass owes mu_b, the other colour mu_a and then mu_b."""
    a = np.asarray(a, dtype)
    return np.where(colour_mask(a.shape, last), a - dtype(mu_b), (a - dtype(mu_a)) - dtype(mu_b))


def gs_eager(a, rho, nd, gs3d, mus, dtype=F64):
    """len(mus) colour passes (colour k & 1), each followed at once by the
    subtraction of mus[k] from every point, as the reference code neutralises.
    Returns the grid and, per pass, the grid before its mean was subtracted."""
    a = np.asarray(a, dtype)
    seen = []
    for k, mu in enumerate(mus):
        a = gs_colour(a, rho, k & 1, nd, gs3d, 0, dtype)
        seen.append(a)
        a = a - dtype(mu)
    return a, seen


def gs_lazy(a, rho, nd, gs3d, npass, dtype=F64):
    """The device's protocol for the same smoothing (pinc_mg.c: smooth): the
    grid stays raw, pass k reads the other colour less the mean of pass k - 1
    and yields the mean of the grid it leaves (the other colour still less
    that mean), and the last two means are applied at the end.  Returns the
    materialised grid and the means."""
    a = np.asarray(a, dtype)
    mus = []
    for k in range(npass):
        prev = mus[-1] if k else dtype(0)
        a = gs_colour(a, rho, k & 1, nd, gs3d, prev, dtype)
        left = np.where(colour_mask(a.shape, k & 1), a, a - dtype(prev))
        mus.append(left.sum(dtype=dtype) / dtype(a.size))
    return materialize(a, (npass - 1) & 1, mus[-2], mus[-1], dtype), mus


def residual(a, rho, nd, dtype=F64):
    """rho + Laplacian(a) (residual_at): -2 nd a, += the neighbour sum (3-D:
    one left-to-right sum of the six; else up + dn per dimension), + rho."""
    a = np.asarray(a, dtype)
    rho = np.asarray(rho, dtype)
    assert a.ndim == nd
    r = dtype(-2 * nd) * a
    if nd == 3:
        r = r + (_up(a, 0) + _dn(a, 0) + _up(a, 1) + _dn(a, 1) + _up(a, 2) + _dn(a, 2))
    else:
        for d in range(nd):
            r = r + (_up(a, d) + _dn(a, d))
    return r + rho


def restrict(fine, nd, hw3d, dtype=F64):
    """Half-weight restriction onto the even points (k_restrict).  hw3d:
    (1/12) (6 f + x+ + x- + y+ + y- + z+ + z-) left to right; else 2 nd f,
    += up + dn per dimension, times 1/(4 nd)."""
    f = np.asarray(fine, dtype)
    assert f.ndim == nd and all(t % 2 == 0 for t in f.shape)
    if hw3d:
        assert nd == 3
        v = (dtype(1) / dtype(12)) * (dtype(6) * f + _up(f, 0) + _dn(f, 0) + _up(f, 1) + _dn(f, 1) + _up(f, 2) +
                                      _dn(f, 2))
    else:
        v = dtype(2 * nd) * f
        for d in range(nd):
            v = v + (_up(f, d) + _dn(f, d))
        v = v * (dtype(1) / dtype(4 * nd))
    return v[(slice(None, None, 2),) * nd].copy()


def _interp(g, axis, dtype):
    """double the grid along one axis: even points copy, odd points are
    0.5 (lower + upper) with the upper neighbour wrapped"""
    shape = list(g.shape)
    shape[axis] *= 2
    out = np.empty(shape, dtype)
    ev = [slice(None)] * g.ndim
    od = [slice(None)] * g.ndim
    ev[axis] = slice(0, None, 2)
    od[axis] = slice(1, None, 2)
    out[tuple(ev)] = g
    out[tuple(od)] = dtype(0.5) * (g + np.roll(g, -1, axis))
    return out


def prolong(coarse, nd, dtype=F64):
    """Bilinear prolongation with prol_low's nesting: the highest dimension
    is interpolated first (z, then y, then x), each odd point 0.5 (a + b) of
    values already interpolated along the higher dimensions."""
    g = np.asarray(coarse, dtype)
    assert g.ndim == nd
    for d in range(nd - 1, -1, -1):
        g = _interp(g, _ax(nd, d), dtype)
    return g


def neutralize(a, dtype=F64):
    a = np.asarray(a, dtype)
    return a - a.sum(dtype=dtype) / dtype(a.size)


def _smooth(phi, rho, n, nd, gs3d, dtype):
    for _ in range(n):
        for colour in (0, 1):
            phi = gs_colour(phi, rho, colour, nd, gs3d, 0, dtype)
    return phi


def coarse_cycle(rho, levels, nPre, nPost, nCoarse, hw3d, gs3d, dtype=F64):
    """The V-cycle of the single-workgroup coarse solve (coarse_body): on the
    way down neutralise rho, pre-smooth from zero, residual, restriction
    times 4; at the bottom neutralise rho, smooth, neutralise phi; on the way
    up prolong-add, post-smooth, neutralise phi.  levels: (Tx, Ty, Tz) tuples,
    finest first.  Returns level 0's correction."""
    nd = len(levels[0])
    nl = len(levels)
    r = [None] * nl
    p = [None] * nl
    r[0] = np.asarray(rho, dtype).reshape(levels[0][::-1])
    for l in range(nl - 1):
        r[l] = neutralize(r[l], dtype)
        p[l] = _smooth(np.zeros_like(r[l]), r[l], nPre, nd, gs3d, dtype)
        r[l + 1] = restrict(residual(p[l], r[l], nd, dtype), nd, hw3d, dtype) * dtype(4)
        assert r[l + 1].shape == tuple(levels[l + 1][::-1])
    b = nl - 1
    r[b] = neutralize(r[b], dtype)
    p[b] = neutralize(_smooth(np.zeros_like(r[b]), r[b], nCoarse, nd, gs3d, dtype), dtype)
    for l in range(nl - 2, -1, -1):
        p[l] = p[l] + prolong(p[l + 1], nd, dtype)
        p[l] = neutralize(_smooth(p[l], r[l], nPost, nd, gs3d, dtype), dtype)
    return p[0]


# ---------------------------------------------------------------- z-slabs ---
# Level 0 of rank `rank` of P: its nloc = Tz / P planes extended by hz halo
# planes on each side, periodic in x and y only.

def extended_slab(glob, rank, nloc, hz):
    """planes (rank nloc - hz + k) mod Tz, k = 0 .. nloc + 2 hz - 1"""
    tz = glob.shape[0]
    return glob[(rank * nloc - hz + np.arange(nloc + 2 * hz)) % tz].copy()


def residual_slab(phi_x, rho_x, zlo, zhi, dtype=F64):
    """the residual on planes [zlo, zhi) of an extended slab, the z
    neighbours read from the slab itself (k_residual_slab)"""
    a = np.asarray(phi_x, dtype)
    rho = np.asarray(rho_x, dtype)
    assert 1 <= zlo < zhi <= a.shape[0] - 1
    c = a[zlo:zhi]
    r = dtype(-6) * c
    r = r + (_up(c, 0) + _dn(c, 0) + _up(c, 1) + _dn(c, 1) + a[zlo + 1:zhi + 1] + a[zlo - 1:zhi - 1])
    return r + rho[zlo:zhi]


def restrict_slab(fine_x, zf0, ncz, hw3d, dtype=F64):
    """coarse (x, y, z) <- fine (2x, 2y, zf0 + 2z) of an extended slab, z = 0
    .. ncz - 1, times 4 (k_restrict_slab)"""
    f = np.asarray(fine_x, dtype)
    assert zf0 >= 1 and zf0 + 2 * ncz <= f.shape[0]
    z = zf0 + 2 * np.arange(ncz)
    c, zp, zm = f[z], f[z + 1], f[z - 1]
    if hw3d:
        v = (dtype(1) / dtype(12)) * (dtype(6) * c + _up(c, 0) + _dn(c, 0) + _up(c, 1) + _dn(c, 1) + zp + zm)
    else:
        v = dtype(6) * c
        v = v + (_up(c, 0) + _dn(c, 0))
        v = v + (_up(c, 1) + _dn(c, 1))
        v = v + (zp + zm)
        v = v * (dtype(1) / dtype(12))
    return (v[:, ::2, ::2] * dtype(4)).copy()


def prolong_slab(coarse, z0, nplanes, dtype=F64):
    """the prolongated global level 1 on the planes of an extended slab: slab
    plane k is global plane (z0 + k) mod Tz (k_prolong_add_slab)"""
    p = prolong(coarse, 3, dtype)
    return p[(z0 + np.arange(nplanes)) % p.shape[0]].copy()


def prolong_own(coarse_x, nz, dtype=F64):
    """the prolongated level 1 on a rank's nz owned planes, from its nz / 2
    level-1 planes with one halo plane on each side (k_prolong_add_own): owned
    plane k is plane k + 2 of the frame whose coarse plane 0 is the lower halo
    plane"""
    cx = np.asarray(coarse_x, dtype)
    assert nz % 2 == 0 and cx.shape[0] == nz // 2 + 2
    return prolong(cx, 3, dtype)[2:nz + 2].copy()
