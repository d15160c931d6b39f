"""Plain numpy restatements of the field stage: the grid glue of k_grid.hip
(E = h (phi[+1] - phi[-1]) on a slab, slab gather, ghost fold, plane add and
copy, the two-stage sum) and the spectral Poisson solve of k_spectral.hip
(whole domain, and split over P z-slabs).  No GPU, no torch.

Shapes are (Tx, Ty, Tz); arrays are [z][y][x], a trailing axis holds the
values of a node.  A geometry is (T, off, nloc): the slab dimension is the
last of T (axis 0 of the array), the slab holds planes 0 .. nloc + 1, plane p
at the global coordinate wrap(off + p - 1).
"""
import numpy as np

F64 = np.float64
LD = np.longdouble


# ------------------------------------------------------------------ slabs ---

def slab_planes(geom, shift=0):
    """global coordinate of each slab plane 0 .. nloc + 1"""
    T, off, nloc = geom
    return (off + np.arange(nloc + 2) - 1 + shift) % T[-1]


def efield_slab(phi_global, geom, h, planes=slab_planes, swap=False):
    """E[idx * ND + d] = h * (phi[up_d] - phi[dn_d]) on the slab's planes, in
    fp64 and the kernel's expression order"""
    T = geom[0]
    nd = len(T)
    phi = np.asarray(phi_global, F64)
    assert phi.shape == tuple(T)[::-1]
    comp = []
    for d in range(nd):
        ax = nd - 1 - d
        up, dn = np.roll(phi, -1, ax), np.roll(phi, 1, ax)
        if swap:
            up, dn = dn, up
        comp.append(F64(h) * (up - dn))
    return np.stack(comp, axis=-1)[planes(geom)]


def slab_from_global(glob, geom, nv, planes=slab_planes):
    """slab[idx * nv + v] = glob[gi * nv + v]; glob is [z][y][x][nv]"""
    g = np.asarray(glob, F64)
    assert g.shape == tuple(geom[0])[::-1] + (nv,)
    return g[planes(geom)].copy()


def fold_self(slab, geom, nv=1, reverse=False):
    """the slab sending its ghost planes to itself: the upper ghost plane is
    added into plane 1, then the lower ghost plane into plane nloc"""
    nloc = geom[2]
    out = np.array(slab, F64)
    assert out.shape[0] == nloc + 2
    adds = [(1, nloc + 1), (nloc, 0)]
    for dst, src in (adds[::-1] if reverse else adds):
        out[dst] = out[dst] + out[src]
    return out


def add_plane(slab, plane, inp):
    out = np.array(slab, F64)
    out[plane] = out[plane] + np.asarray(inp, F64)
    return out


def copy_plane(slab, plane):
    return np.array(np.asarray(slab, F64)[plane])


# ------------------------------------------------------------- reductions ---

def tree_sum(a, b=None, div=1.0):
    """k_sum + k_reduce addition by addition: per thread a serial sum over
    the grid stride, the 6-stage xor butterfly of a wave, the 4 waves of a
    block in order, then the same over the block partials in one block, then
    the division.  Returns (value, partials)."""
    a = np.asarray(a, F64)
    n = a.size
    v = a if b is None else a * np.asarray(b, F64)
    nb = min(max(-(-n // 2048), 1), 1024)

    def blocks(v, nblocks):
        """the block sums of nblocks blocks of 256 threads over v"""
        g = nblocks * 256
        t = -(-v.size // g)
        pad = np.zeros(t * g)
        pad[:v.size] = v
        s = np.zeros(g)
        for row, cnt in zip(pad.reshape(t, g), np.minimum(g, np.maximum(0, v.size - g * np.arange(t)))):
            s[:cnt] = s[:cnt] + row[:cnt]
        w = s.reshape(-1, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            w = w + w[:, lane ^ o]
        w = w[:, 0].reshape(nblocks, 4)
        r = np.zeros(nblocks)
        for i in range(4):
            r = r + w[:, i]
        return r

    part = blocks(v, nb)
    return blocks(part, 1)[0] / F64(div), part


def tree_depth(n, product=False, division=False):
    """the most roundings one term passes through in tree_sum"""
    nb = min(max(-(-n // 2048), 1), 1024)
    serial = -(-n // (nb * 256)) - 1  # the first add, to 0, is exact
    stage2 = -(-nb // 256) - 1
    return serial + 6 + 3 + stage2 + 6 + 3 + int(product) + int(division)


# --------------------------------------------------------------- spectral ---

def pi_of(dtype):
    return dtype(np.pi) if dtype is F64 else dtype(4) * np.arctan(dtype(1))


def signed_freq(i, T):
    """iy <= Ty / 2 ? iy : iy - Ty"""
    i = np.asarray(i)
    return np.where(i <= T // 2, i, i - T)


def kfactor_at(n, T, discrete, dtype, ntot=None):
    """k_spectral_scale's factor at the frequencies n = (nx, ny, nz) (integer
    arrays that broadcast) of a (Tx, Ty, Tz) grid, in the kernel's expression
    order; the DC mode is not treated here"""
    nd = len(T)
    two_pi = dtype(2) * pi_of(dtype)
    ntot = dtype(int(np.prod(T)) if ntot is None else ntot)
    ang = [two_pi * np.asarray(n[d]).astype(dtype) / dtype(T[d]) for d in range(nd)]
    with np.errstate(divide="ignore", invalid="ignore"):
        if discrete:
            s = dtype(2) - dtype(2) * np.cos(ang[0])
            for d in range(1, nd):
                s = s + (dtype(2) - dtype(2) * np.cos(ang[d]))
            return dtype(1) / s / ntot
        if nd == 1:
            f = dtype(T[0]) / (two_pi * np.asarray(n[0]).astype(dtype))
            return f * f / dtype(T[0])
        k2 = ang[0] * ang[0] + ang[1] * ang[1]
        if nd == 3:
            k2 = k2 + ang[2] * ang[2]
        return dtype(1) / k2 / ntot


def kfactor(shape, discrete, dtype, half=False, Tf=None, freq=signed_freq, ntot=None, dc=0):
    """the factor on the whole spectrum [Tz][Ty][Tx] (half: [Tz][Ty][Tx/2+1]),
    DC set to 0.  x takes the signed frequency too: the factor is even in it,
    and the kernel only sees ix <= Tx / 2.  Tf, freq, ntot and dc = None are
    for deliberate defects: other extents inside the factor, another
    frequency rule for y and z, another N, the DC mode left as computed."""
    T = tuple(shape)
    Tf = T if Tf is None else tuple(Tf)
    nd = len(T)
    ext = [T[0] // 2 + 1 if half else T[0]] + list(T[1:])
    n = [(freq if d else signed_freq)(np.arange(ext[d]), Tf[d]).reshape([-1 if a == nd - 1 - d else 1 for a in range(nd)])
         for d in range(nd)]
    n[0] = np.abs(n[0])
    f = np.array(np.broadcast_to(kfactor_at(n, Tf, discrete, dtype, ntot), ext[::-1]))
    if dc is not None:
        f[(0,) * nd] = dc
    return f


def dft_matrix(n, dtype, sign=-1):
    """exp(sign 2 pi i j k / n), the angle reduced mod n first"""
    jk = np.outer(np.arange(n), np.arange(n)) % n
    ang = dtype(2) * pi_of(dtype) * jk.astype(dtype) / dtype(n)
    return np.cos(ang) + (1j if dtype is F64 else np.clongdouble(1j)) * (dtype(sign) * np.sin(ang))


def dft_axes(a, axes, dtype, sign=-1):
    """the unnormalised dense DFT of a along the given axes"""
    a = np.asarray(a).astype(np.complex128 if dtype is F64 else np.clongdouble)
    for ax in axes:
        a = np.moveaxis(np.tensordot(dft_matrix(a.shape[ax], dtype, sign), a, axes=(1, ax)), 0, ax)
    return a


def poisson(rho, shape, discrete, dtype=LD, factor=None):
    """-lap(phi) = rho on the whole periodic domain by dense separable DFT
    matrices in dtype: spectrum times the factor (which holds 1 / N and the
    zeroed DC mode), unnormalised inverse"""
    rho = np.asarray(rho)
    assert rho.shape == tuple(shape)[::-1]
    axes = range(rho.ndim)
    f = kfactor(shape, discrete, dtype) if factor is None else factor
    return np.real(dft_axes(dft_axes(rho.astype(dtype), axes, dtype) * f, axes, dtype, +1)).astype(dtype)


def poisson_fft64(rho, shape, discrete, factor=None):
    """the same solve with numpy.fft in fp64 on the half spectrum"""
    rho = np.asarray(rho, F64)
    assert rho.shape == tuple(shape)[::-1]
    f = kfactor(shape, discrete, F64, half=True) if factor is None else factor
    axes = tuple(range(rho.ndim))
    return np.fft.irfftn(np.fft.rfftn(rho, axes=axes) * f, s=rho.shape, axes=axes, norm="forward")


def laplacian(phi):
    """the periodic 3-, 5- or 7-point Laplacian"""
    return sum(np.roll(phi, k, ax) for ax in range(phi.ndim) for k in (-1, 1)) - phi.dtype.type(2 * phi.ndim) * phi


# ------------------------------------------------------ slab-distributed ---

def slab_spectrum_blocks(rho_slab, T, P, dtype=F64, swapped=False):
    """S[q][zl][yl][kx] of one rank's forward call: the 2-D half spectrum of
    each of its planes, regrouped by destination ky block (numpy.fft in fp64,
    the dense DFT otherwise)"""
    nloc, Ty, Tx = np.shape(rho_slab)
    Mx, Tyl = Tx // 2 + 1, Ty // P
    assert (Tx, Ty) == tuple(T[:2]) and Tyl * P == Ty
    if dtype is F64:
        A = np.fft.rfft2(np.asarray(rho_slab, F64))
    else:
        A = dft_axes(np.asarray(rho_slab).astype(dtype), (1, 2), dtype)[:, :, :Mx]
    S = A.reshape(nloc, P, Tyl, Mx).transpose(1, 0, 2, 3)
    if swapped:  # a block laid out [yl][zl][kx]: Tyl and nloc exchanged
        S = S.transpose(0, 2, 1, 3).reshape(P, nloc, Tyl, Mx)
    return np.ascontiguousarray(S)


def slab_poisson(rho, T, P, discrete, y0_of=lambda rank, tyl: rank * tyl, Tf=None, freq=signed_freq, ntot=None, dc=0):
    """the slab-distributed solve, all P ranks in turn, in fp64 with
    numpy.fft: forward blocks, all-to-all, transform along z, the factor at
    (kx, y0 + yl, kz) with the DC mode zeroed where that is (0, 0, 0),
    inverse along z, all-to-all back, unpack, inverse 2-D transform.  y0_of
    and kfactor's hooks are for deliberate defects."""
    Tx, Ty, Tz = T
    Tf = tuple(T) if Tf is None else tuple(Tf)
    nloc, Tyl, Mx = Tz // P, Ty // P, Tx // 2 + 1
    rho = np.asarray(rho, F64)
    S = [slab_spectrum_blocks(rho[r * nloc:(r + 1) * nloc], T, P) for r in range(P)]
    B = [np.concatenate([S[r][q] for r in range(P)], axis=0) for q in range(P)]  # [z][yl][kx]
    for q in range(P):
        iy = y0_of(q, Tyl) + np.arange(Tyl)
        n = [np.arange(Mx).reshape(1, 1, -1), freq(iy, Tf[1]).reshape(1, -1, 1),
             freq(np.arange(Tz), Tf[2]).reshape(-1, 1, 1)]
        f = np.array(np.broadcast_to(kfactor_at(n, Tf, discrete, F64, ntot), (Tz, Tyl, Mx)))
        if dc is not None:
            f[0, iy == 0, 0] = dc
        B[q] = np.fft.ifft(np.fft.fft(B[q], axis=0) * f, axis=0, norm="forward")
    phi = np.empty_like(rho)
    for r in range(P):
        A = np.concatenate([B[q][r * nloc:(r + 1) * nloc] for q in range(P)], axis=1)  # [zl][y][kx]
        phi[r * nloc:(r + 1) * nloc] = np.fft.irfft2(A, s=(Ty, Tx), norm="forward")
    return phi
