"""The multigrid restatement (tests/mg_ref.py) without a GPU: anchored to
dense operators built from 1-D matrices, to constants, and its slab forms to
the plane ranges of the global forms; and a list of deliberate mutants, each
of which the comparisons of tests/test_gpu_mg_transfer_kernels.py must tell
from the true restatement on every shape those tests use.
"""
import functools

import numpy as np
import pytest

import mg_cases as K
import mg_ref as MR

LD = np.longdouble
F64 = np.float64
EPS_LD = float(np.finfo(LD).eps)


# ------------------------------------------------------- dense operators ---

def _shift(n, k):
    """(S v)[i] = v[(i + k) mod n]"""
    s = np.zeros((n, n), LD)
    s[np.arange(n), (np.arange(n) + k) % n] = 1
    return s


def _p1(n):
    """1-D prolongation, n -> 2n"""
    p = np.zeros((2 * n, n), LD)
    i = np.arange(n)
    p[2 * i, i] = 1
    p[2 * i + 1, i] += LD(0.5)
    p[2 * i + 1, (i + 1) % n] += LD(0.5)
    return p


def _inj1(n):
    """1-D injection of the even points, 2n -> n"""
    r = np.zeros((n, 2 * n), LD)
    r[np.arange(n), 2 * np.arange(n)] = 1
    return r


def _kron(ms):
    """kron over the dimensions, the highest (slowest) first"""
    return functools.reduce(np.kron, ms)


SMALL = [(2,), (3,), (8,), (2, 2), (3, 5), (4, 2), (2, 2, 2), (3, 2, 4), (4, 3, 2)]


@pytest.mark.parametrize("cshape", SMALL)
def test_prolongation_is_the_kron_of_1d_operators(cshape):
    nd = len(cshape)
    (c,) = K.fields([cshape], 1)
    P = _kron([_p1(t) for t in cshape[::-1]])
    want = (P @ c.astype(LD).ravel()).reshape(K.fine_of(cshape)[::-1])
    got = MR.prolong(c, nd, LD)
    assert got.dtype == LD
    np.testing.assert_allclose(got, want, rtol=0, atol=8 * EPS_LD * np.max(np.abs(c)))
    # and the fp64 form is the same operator in another rounding
    np.testing.assert_allclose(MR.prolong(c, nd, F64), want.astype(F64), rtol=0, atol=8 * 2.3e-16 * np.max(np.abs(c)))


@pytest.mark.parametrize("cshape", SMALL)
def test_restriction_is_injection_of_the_half_weight_stencil(cshape):
    nd = len(cshape)
    fshape = K.fine_of(cshape)
    (f,) = K.fields([fshape], 2)
    n = f.size
    eye = [np.eye(t, dtype=LD) for t in fshape[::-1]]
    S = LD(2 * nd) * np.eye(n, dtype=LD)
    for ax in range(nd):
        for k in (1, -1):
            S = S + _kron([_shift(fshape[::-1][a], k) if a == ax else eye[a] for a in range(nd)])
    S = S / LD(4 * nd)
    R = _kron([_inj1(t) for t in cshape[::-1]])
    want = (R @ (S @ f.astype(LD).ravel())).reshape(cshape[::-1])
    atol = 16 * EPS_LD * np.max(np.abs(f))
    for hw3d in ((0, 1) if nd == 3 else (0,)):
        np.testing.assert_allclose(MR.restrict(f, nd, hw3d, LD), want, rtol=0, atol=atol)
        np.testing.assert_allclose(MR.restrict(f, nd, hw3d, F64), want.astype(F64), rtol=0,
                                   atol=16 * 2.3e-16 * np.max(np.abs(f)))


@pytest.mark.parametrize("shape", [(3,), (8,), (3, 5), (4, 2), (3, 2, 4), (2, 2, 2)])
def test_residual_is_the_dense_laplacian_plus_rho(shape):
    nd = len(shape)
    a, rho = K.fields([shape, shape], 3)
    eye = [np.eye(t, dtype=LD) for t in shape[::-1]]
    A = LD(-2 * nd) * np.eye(a.size, dtype=LD)
    for ax in range(nd):
        for k in (1, -1):
            A = A + _kron([_shift(shape[::-1][q], k) if q == ax else eye[q] for q in range(nd)])
    want = (A @ a.astype(LD).ravel()).reshape(a.shape) + rho
    np.testing.assert_allclose(MR.residual(a, rho, nd, LD), want, rtol=0, atol=16 * EPS_LD * np.max(np.abs(a)))
    np.testing.assert_allclose(MR.residual(a, rho, nd, F64), want.astype(F64), rtol=0,
                               atol=16 * 2.3e-16 * np.max(np.abs(a)))


@pytest.mark.parametrize("shape", [(4,), (6, 4), (4, 6, 2)])
def test_gs_colour_solves_its_points_equation(shape):
    """after a colour pass the residual vanishes on that colour (to
    rounding) and the other colour is untouched, in both forms"""
    nd = len(shape)
    a, rho = K.fields([shape, shape], 4)
    for gs3d in ((0, 1) if nd == 3 else (0,)):
        for colour in (0, 1):
            for mu in (0.0, 0.375):
                b = MR.gs_colour(a, rho, colour, nd, gs3d, mu, LD)
                m = MR.colour_mask(a.shape, colour)
                np.testing.assert_array_equal(b[~m], a.astype(LD)[~m])
                shifted = np.where(m, b, b - LD(mu))
                r = MR.residual(shifted, rho, nd, LD)
                assert np.max(np.abs(r[m])) <= 64 * EPS_LD * np.max(np.abs(a))


# ------------------------------------------------------------- constants ---

@pytest.mark.parametrize("shape", [(6,), (4, 6), (4, 6, 2)])
@pytest.mark.parametrize("dtype", [F64, LD])
def test_constants(shape, dtype):
    nd = len(shape)
    c = np.full(shape[::-1], 1.5)
    for hw3d in ((0, 1) if nd == 3 else (0,)):
        r = MR.restrict(c, nd, hw3d, dtype)
        assert r.shape == K.coarse_of(shape)[::-1]
        np.testing.assert_allclose(r, 1.5, rtol=2 * float(np.finfo(dtype).eps), atol=0)
    (f0,) = K.fields([K.fine_of(shape)], 5)
    np.testing.assert_array_equal(f0.astype(dtype) + MR.prolong(c, nd, dtype), f0.astype(dtype) + dtype(1.5))
    np.testing.assert_array_equal(MR.residual(c, np.zeros_like(c), nd, dtype), 0)
    # a constant is a fixed point of the smoother with zero source, and the
    # pending mean shifts what is read, not what is stored
    for gs3d in ((0, 1) if nd == 3 else (0,)):
        g = MR.gs_colour(c, np.zeros_like(c), 0, nd, gs3d, 0.5, dtype)
        np.testing.assert_allclose(g, np.where(MR.colour_mask(c.shape, 0), 1.0, 1.5), rtol=2 * float(np.finfo(dtype).eps))


# ------------------------------------------------------------ slab forms ---

@pytest.mark.parametrize("T,P,hz", K.SLABS)
def test_slab_forms_are_plane_ranges_of_the_global_forms(T, P, hz):
    phi, rho, corr = K.fields([T, T, K.coarse_of(T)], K.SEED["slab"])
    tz = T[2]
    nloc = tz // P
    res = MR.residual(phi, rho, 3)
    pro = phi + MR.prolong(corr, 3)
    for rank in range(P):
        px = MR.extended_slab(phi, rank, nloc, hz)
        rx = MR.extended_slab(rho, rank, nloc, hz)
        assert px.shape == (nloc + 2 * hz, T[1], T[0])
        np.testing.assert_array_equal(px[hz:hz + nloc], phi[rank * nloc:(rank + 1) * nloc])
        np.testing.assert_array_equal(px[0], phi[(rank * nloc - hz) % tz])
        own = (rank * nloc + np.arange(-1, nloc)) % tz
        rs = MR.residual_slab(px, rx, hz - 1, hz + nloc)
        np.testing.assert_array_equal(rs, res[own])
        resx = np.full_like(px, np.nan)
        resx[hz - 1:hz + nloc] = rs
        for hw3d in (0, 1):
            want = (MR.restrict(res, 3, hw3d) * 4.0)[rank * nloc // 2:(rank + 1) * nloc // 2]
            np.testing.assert_array_equal(MR.restrict_slab(resx, hz, nloc // 2, hw3d), want)
        z0 = rank * nloc - hz
        np.testing.assert_array_equal(px + MR.prolong_slab(corr, z0, nloc + 2 * hz), MR.extended_slab(pro, rank, nloc, hz))
        cx = MR.extended_slab(corr, rank, nloc // 2, 1)
        np.testing.assert_array_equal(px[hz:hz + nloc] + MR.prolong_own(cx, nloc),
                                      pro[rank * nloc:(rank + 1) * nloc])


# ------------------------------------------------------------- smoothing ---

@pytest.mark.parametrize("shape", K.GS_SHAPES)
def test_lazy_means_equal_eager_neutralisation(shape):
    """the device's protocol (raw grid, means pending, materialised at the
    end) gives bit for bit the grid of a neutralisation after every colour,
    given the same means"""
    nd = len(shape)
    a, rho = K.fields([shape, shape], K.SEED["gs"])
    for gs3d in ((0, 1) if nd == 3 else (0,)):
        lazy, mus = MR.gs_lazy(a, rho, nd, gs3d, 6)
        eager, seen = MR.gs_eager(a, rho, nd, gs3d, mus)
        np.testing.assert_array_equal(lazy, eager)
        for k in range(6):
            assert mus[k] == seen[k].sum() / a.size


# --------------------------------------------------------------- mutants ---
# Deliberate defects of the restatement.  Each must be told from the true
# form, by the comparison the GPU test makes, on every shape that test uses.

def restrict_w5(fine, nd, hw3d, dtype=F64):
    """the centre weight one too small"""
    f = np.asarray(fine, dtype)
    nb = sum(np.roll(f, k, ax) for ax in range(nd) for k in (-1, 1))
    if hw3d:
        v = (dtype(1) / dtype(12)) * (dtype(5) * f + nb)
    else:
        v = (dtype(2 * nd - 1) * f + nb) * (dtype(1) / dtype(4 * nd))
    return v[(slice(None, None, 2),) * nd].copy()


def restrict_slab_w5(fine_x, zf0, ncz, hw3d, dtype=F64):
    f = np.asarray(fine_x, dtype)
    z = zf0 + 2 * np.arange(ncz)
    c = f[z]
    nb = np.roll(c, -1, 2) + np.roll(c, 1, 2) + np.roll(c, -1, 1) + np.roll(c, 1, 1) + f[z + 1] + f[z - 1]
    return ((dtype(1) / dtype(12)) * (dtype(5) * c + nb))[:, ::2, ::2] * dtype(4)


def prolong_badwrap(coarse, nd, dtype=F64):
    """the wrap of the upper neighbour b[D] lands one plane off (on coarse
    plane 1 instead of 0), along the highest dimension"""
    g = np.asarray(coarse, dtype)
    up = np.roll(g, -1, 0)
    up[-1] = g[1 % g.shape[0]]
    out = np.empty((2 * g.shape[0],) + g.shape[1:], dtype)
    out[0::2] = g
    out[1::2] = dtype(0.5) * (g + up)
    for d in range(nd - 2, -1, -1):
        out = MR._interp(out, nd - 1 - d, dtype)
    return out


def prolong_slab_z0(coarse, z0, nplanes, dtype=F64):
    """z0 off by one"""
    return MR.prolong_slab(coarse, z0 + 1, nplanes, dtype)


def prolong_own_no2(coarse_x, nz, dtype=F64):
    """the frame's + 2 dropped"""
    return MR.prolong(coarse_x, 3, dtype)[0:nz].copy()


_true_gs = MR.gs_colour


def gs_flipped(a, rho, colour, nd, gs3d, mu=0, dtype=F64):
    return _true_gs(a, rho, 1 - colour, nd, gs3d, mu, dtype)


def gs_reads_raw(a, rho, colour, nd, gs3d, mu=0, dtype=F64):
    """mu not applied to the reads"""
    return _true_gs(a, rho, colour, nd, gs3d, 0, dtype)


def differ(a, b):
    """what assert_array_equal would report: any element unequal"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape != b.shape or bool(np.any(a != b))


def test_prolong_badwrap_is_the_true_form_without_the_defect():
    """the mutant's scaffolding restates prolong: with the wrap entry put
    right it is the true prolongation"""
    for cshape in [(3,), (3, 2), (2, 3, 4)]:
        (c,) = K.fields([cshape], 6)
        m = prolong_badwrap(c, len(cshape))
        t = MR.prolong(c, len(cshape))
        assert differ(m, t)
        np.testing.assert_array_equal(m[:-1], t[:-1])


@pytest.mark.parametrize("cshape", K.RESTRICT_COARSE)
def test_mutant_restriction_weight(cshape):
    nd = len(cshape)
    (f,) = K.fields([K.fine_of(cshape)], K.SEED["restrict"])
    for hw3d in ((0, 1) if nd == 3 else (0,)):
        assert differ(restrict_w5(f, nd, hw3d), MR.restrict(f, nd, hw3d))


@pytest.mark.parametrize("fshape", K.RESID_RESTRICT_FINE)
def test_mutant_restriction_weight_after_the_residual(fshape):
    phi, rho = K.fields([fshape, fshape], K.SEED["resid_restrict"])
    res = MR.residual(phi, rho, 3)
    for hw3d in (0, 1):
        for scale in (1.0, 4.0):
            assert differ(restrict_w5(res, 3, hw3d) * scale, MR.restrict(res, 3, hw3d) * scale)


@pytest.mark.parametrize("fshape", K.PROLONG_FINE)
def test_mutant_prolongation_wrap(fshape):
    nd = len(fshape)
    f0, c = K.fields([fshape, K.coarse_of(fshape)], K.SEED["prolong"])
    assert differ(f0 + prolong_badwrap(c, nd), f0 + MR.prolong(c, nd))


@pytest.mark.parametrize("T,P,hz", K.SLABS)
def test_mutants_of_the_slab_forms(T, P, hz):
    phi, rho, corr = K.fields([T, T, K.coarse_of(T)], K.SEED["slab"])
    nloc = T[2] // P
    res = MR.residual(phi, rho, 3)
    for rank in range(P):
        px = MR.extended_slab(phi, rank, nloc, hz)
        rx = MR.extended_slab(rho, rank, nloc, hz)
        resx = MR.extended_slab(res, rank, nloc, hz)  # every plane valid, for the shifted reads
        z0 = rank * nloc - hz
        nx = nloc + 2 * hz
        for hw3d in (0, 1):
            true = MR.restrict_slab(resx, hz, nloc // 2, hw3d)
            assert differ(restrict_slab_w5(resx, hz, nloc // 2, hw3d), true)
            assert differ(MR.restrict_slab(resx, hz - 1, nloc // 2, hw3d), true)  # zf0 off by one
        true = px + MR.prolong_slab(corr, z0, nx)
        assert differ(px + prolong_slab_z0(corr, z0, nx), true)
        bad = prolong_badwrap(corr, 3)[(z0 + np.arange(nx)) % T[2]]
        assert differ(px + bad, true)
        cx = MR.extended_slab(corr, rank, nloc // 2, 1)
        own = px[hz:hz + nloc]
        assert differ(own + prolong_own_no2(cx, nloc), own + MR.prolong_own(cx, nloc))
        # the residual's planes one off
        assert differ(MR.residual_slab(px, rx, hz, hz + nloc + 1), MR.residual_slab(px, rx, hz - 1, hz + nloc))


@pytest.mark.parametrize("mutant", [gs_flipped, gs_reads_raw])
@pytest.mark.parametrize("shape", K.GS_SHAPES)
def test_mutants_of_the_smoother(shape, mutant, monkeypatch):
    """the GPU test's comparison: the materialised grid of the device's
    protocol against the eager reference with the protocol's own means"""
    nd = len(shape)
    a, rho = K.fields([shape, shape], K.SEED["gs"])
    for gs3d in ((0, 1) if nd == 3 else (0,)):
        with monkeypatch.context() as mp:
            mp.setattr(MR, "gs_colour", mutant)
            got, mus = MR.gs_lazy(a, rho, nd, gs3d, 6)
        want, _ = MR.gs_eager(a, rho, nd, gs3d, mus)
        assert differ(got, want)
        if mutant is gs_flipped:  # the single pass without means
            assert differ(mutant(a, rho, 0, nd, gs3d), MR.gs_colour(a, rho, 0, nd, gs3d))


@pytest.mark.parametrize("case", K.COARSE, ids=[str(c[0][0]) + f"-{c[1]}{c[2]}" for c in K.COARSE])
def test_mutants_of_the_coarse_cycle(case, monkeypatch):
    """the GPU test's comparison: within the measured bound of the fp64
    cycle.  Every mutant of an operator the case uses lands outside it."""
    levels, hw3d, gs3d = case
    rho, ref, d, tol = K.coarse_reference(case)
    assert ref.shape == levels[0][::-1] and d > 0
    # the bound is rounding-sized
    assert tol <= 1e-12 * np.max(np.abs(ref))
    pre, post, nc = K.COARSE_SMOOTH
    # In 1-D red-black Gauss-Seidel with the half-weight restriction is cyclic
    # reduction: the cycle solves its equation outright, whichever colour
    # goes first, so the colour order cannot show there (it is pinned by the
    # smoother's own cases, and by the 2-D and 3-D cycles here).
    nd = len(levels[0])
    if nd == 1:
        assert np.max(np.abs(MR.residual(ref, MR.neutralize(rho), 1))) <= 1e-13 * np.max(np.abs(rho))
    muts = [("gs_colour", gs_flipped)] if nd > 1 else []
    if len(levels) > 1:
        muts += [("restrict", restrict_w5), ("prolong", prolong_badwrap)]
    for name, m in muts:
        with monkeypatch.context() as mp:
            mp.setattr(MR, name, m)
            bad = MR.coarse_cycle(rho, levels, pre, post, nc, hw3d, gs3d)
        assert np.max(np.abs(bad - ref)) > tol, name
    # the correction is neutral
    assert abs(ref.mean()) <= ref.size * np.finfo(F64).eps * np.max(np.abs(ref))
