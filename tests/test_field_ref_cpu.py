"""The field-stage restatement (tests/field_ref.py) without a GPU: anchored to
the checker (oracle/) on four configurations, to properties that do not use
the restatement's own transforms, and a list of deliberate mutants, each of
which the comparisons of tests/test_gpu_grid_kernels.py and
tests/test_gpu_spectral_kernels.py must tell from the true restatement on the
cases of tests/field_cases.py.
"""
import numpy as np
import pytest

import field_cases as K
import field_ref as FR
import orc
from pinc_amd import configs

LD = np.longdouble
F64 = np.float64
EPS_LD = float(np.finfo(LD).eps)

ORACLE = [("langmuir1d", {}), ("langmuir2d", {}), ("cold3d", {}), ("cold3d", {"true_size": (32, 24, 16)})]


def _world(name, kw):
    cfg = configs.config(name, **kw)
    cfg["methods"]["poisson"] = "sSolver"
    return orc.World(configs.write_ini(cfg))


def _set_true(w, which, vals):
    g = w.grid(which)
    g[tuple([slice(1, -1)] * (g.ndim - 1)) + (0,)] = vals
    w.set_grid(which, g)


# ----------------------------------------------------- against the oracle ---

@pytest.mark.parametrize("name,kw", ORACLE)
def test_efield_slab_is_the_oracles_efield(name, kw):
    """op("efield") on random phi: gFinDiff1st, the halo, gMul(E, -1).  The
    restatement with h = -0.5 on the whole domain equals it bit for bit on
    the true nodes and on both ghost planes of the slab dimension."""
    w = _world(name, kw)
    nd = w.ndims
    shape = w.grid(1).shape[:-1]
    phi = K.normals([n - 2 for n in shape], 11)
    _set_true(w, 1, phi)
    w.op("efield")
    E = w.grid(2)[(slice(None),) + (slice(1, -1),) * (nd - 1)]
    w.close()
    T = phi.shape[::-1]
    mine = FR.efield_slab(phi, K.whole(*T), -0.5)
    assert mine.shape == E.shape
    np.testing.assert_array_equal(mine, E)


@pytest.mark.parametrize("name,kw", ORACLE)
def test_poisson_is_the_oracles_solve(name, kw):
    w = _world(name, kw)
    nd = w.ndims
    shape = w.grid(0).shape[:-1]
    rho = K.normals([n - 2 for n in shape], 11)
    _set_true(w, 0, rho)
    w.op("solve")
    phio = w.grid(1)[tuple([slice(1, -1)] * nd) + (0,)]
    w.close()
    T = rho.shape[::-1]
    top = np.abs(phio).max()
    assert np.abs(FR.poisson(rho, T, 0, F64) - phio).max() <= 1e-11 * top
    assert np.abs(FR.poisson_fft64(rho, T, 0) - phio).max() <= 1e-11 * top


# ------------------------------------------------- independent properties ---

@pytest.mark.parametrize("T", K.SPECTRAL + [t for t, _ in K.SLAB_SPECTRAL], ids=K.shape_id)
def test_discrete_symbol_inverts_the_stencil(T):
    """-laplacian(phi) == rho - mean(rho) with the 3-, 5- or 7-point stencil,
    in long double.  An extent of 2 makes both neighbours one node: the
    stencil's 2 phi[+1] - 2 phi is the symbol 2 - 2 cos(pi) = 4 all the same."""
    rho, phi, _, _, top = K.spectral_reference(T, 1)
    r = rho.astype(LD)
    want = r - r.sum() / LD(r.size)
    assert phi.dtype == LD
    assert np.max(np.abs(-FR.laplacian(phi) - want)) <= 64 * EPS_LD * max(1.0, top) * len(T)
    assert abs(phi.sum()) <= 64 * EPS_LD * top * phi.size


def _modes(T):
    """signed modes that include Nyquist in x and frequencies above T/2 (as
    stored) in y and z"""
    out = [tuple(1 if t > 2 else 0 for t in T), tuple([T[0] // 2] + [-(t // 2) for t in T[1:]])]
    if len(T) > 1:
        out.append(tuple([1] + [-1] * (len(T) - 1)))
        out.append(tuple([0] + [-(t // 2) for t in T[1:]]))
    return [m for m in dict.fromkeys(out) if any(m)]


@pytest.mark.parametrize("T", K.SPECTRAL + [t for t, _ in K.SLAB_SPECTRAL], ids=K.shape_id)
def test_continuous_symbol_on_single_modes(T):
    """rho = cos(2 pi sum_d m_d x_d / T_d) gives phi = rho / |k|^2 with
    k_d = 2 pi m_d / T_d, m the signed mode: b < 0 is stored at b + Ty > Ty/2"""
    nd = len(T)
    pi = FR.pi_of(LD)
    grids = np.meshgrid(*[np.arange(t) for t in T[::-1]], indexing="ij")[::-1]  # x, y, z
    for m in _modes(T):
        # the angle reduced exactly in integers before it meets pi
        num = sum(m[d] * grids[d] * (int(np.prod(T)) // T[d]) for d in range(nd)) % int(np.prod(T))
        rho = np.cos(LD(2) * pi * num.astype(LD) / LD(int(np.prod(T))))
        k2 = sum((LD(2) * pi * LD(m[d]) / LD(T[d])) ** 2 for d in range(nd))
        phi = FR.poisson(rho, T, 0, LD)
        assert np.max(np.abs(phi - rho / k2)) <= 256 * EPS_LD / float(k2), m


def test_fft64_is_the_same_operator():
    for T in K.SPECTRAL:
        for disc in K.SYMBOLS:
            rho, hi, d, tol, top = K.spectral_reference(T, disc)
            assert d <= 64 * K.EPS * top and tol <= 1e-11 * top and tol >= 64 * K.EPS * top


@pytest.mark.parametrize("T,P", K.SLAB_SPECTRAL)
def test_slab_solve_is_the_whole_domain_solve(T, P):
    for disc in K.SYMBOLS:
        rho, hi, d, tol, top = K.spectral_reference(T, disc, K.SEED["slab_spectral"])
        assert np.max(np.abs(FR.slab_poisson(rho, T, P, disc) - hi)) <= tol
        nloc = T[2] // P
        for r in range(P):
            S, dS, tolS, _ = K.slab_block_reference(T, P, r)
            assert S.shape == (P, nloc, T[1] // P, T[0] // 2 + 1)
            got = FR.slab_spectrum_blocks(rho[r * nloc:(r + 1) * nloc], T, P)
            assert np.max(np.abs(got - S)) <= tolS
            # the block of ky rows q is what numpy's fftn holds there
            full = np.fft.fft2(rho[r * nloc:(r + 1) * nloc])
            for q in range(P):
                np.testing.assert_allclose(got[q], full[:, q * (T[1] // P):(q + 1) * (T[1] // P), :T[0] // 2 + 1],
                                           rtol=0, atol=tolS)


def test_tree_sum_is_a_sum():
    for n in K.N_ELEMENTS:
        a, b = K.normals((2, n), K.SEED["reduce"])
        for bb, div in ((None, 1.0), (None, 3.0), (b, 1.0)):
            v, part = FR.tree_sum(a, bb, div)
            terms = a.astype(LD) * (1 if bb is None else bb.astype(LD))
            D = FR.tree_depth(n, bb is not None, div != 1.0)
            assert abs(LD(v) - terms.sum() / LD(div)) <= D * K.EPS * float(np.abs(terms).sum()) / div
            assert part.size == min(max(-(-n // 2048), 1), 1024)
    assert FR.tree_depth(K.N_ELEMENTS[-1]) == 29 and FR.tree_depth(K.N_ELEMENTS[-1], True, True) == 31
    assert FR.tree_depth(1) == 18


# --------------------------------------------------------------- mutants ---
# Deliberate defects of the restatement.  Each must be told from the true
# form by the comparison the GPU test makes: unequal bits where that test is
# bit for bit, outside its bound where it has one.  A defect that is the
# identity on a case by construction (Ty == Tz for the swap, ...) is skipped
# there and must show on the others.

def differ(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape != b.shape or bool(np.any(a != b))


def outside(got, ref, tol):
    """the GPU test's assertion fails: not (all finite and max dev <= tol)"""
    return not (np.all(np.isfinite(got)) and np.max(np.abs(got - ref)) <= tol)


def unsigned(i, T):
    return np.asarray(i)


def planes_off_by_one(geom):
    return FR.slab_planes(geom, 1)


@pytest.mark.parametrize("geom", K.GEOMS, ids=K.geom_id)
def test_mutants_of_the_efield(geom):
    T = geom[0]
    phi = K.normals(T[::-1], K.SEED["efield"])
    for h in K.H:
        true = FR.efield_slab(phi, geom, h)
        assert true.shape == K.slab_shape(geom, len(T))
        if max(T) > 2:  # with every extent 2, up == dn and E is zero
            assert differ(FR.efield_slab(phi, geom, h, planes=planes_off_by_one), true)
            assert differ(FR.efield_slab(phi, geom, h, swap=True), true)
        else:
            assert not np.any(true)
    assert FR.efield_slab(phi, geom, -0.5).tobytes() == (-FR.efield_slab(phi, geom, 0.5)).tobytes()


@pytest.mark.parametrize("geom", K.GEOMS, ids=K.geom_id)
def test_mutant_of_the_slab_gather(geom):
    for nv in K.NVALUES:
        glob = K.normals(geom[0][::-1] + (nv,), K.SEED["slab"])
        true = FR.slab_from_global(glob, geom, nv)
        assert true.shape == K.slab_shape(geom, nv)
        assert differ(FR.slab_from_global(glob, geom, nv, planes=planes_off_by_one), true)


@pytest.mark.parametrize("geom", K.FOLD_GEOMS, ids=K.geom_id)
def test_mutant_of_the_fold_order(geom):
    """with nloc == 1 both adds land in plane 1: (p1 + p2) + p0 against
    (p1 + p0) + p2 differ in bits; with nloc > 1 the order cannot show"""
    for nv in K.NVALUES:
        slab = K.normals(K.slab_shape(geom, nv), K.SEED["fold"])
        true, rev = FR.fold_self(slab, geom, nv), FR.fold_self(slab, geom, nv, reverse=True)
        np.testing.assert_array_equal(true[[0, -1]], slab[[0, -1]])
        if geom[2] == 1:
            np.testing.assert_array_equal(true[1], (slab[1] + slab[2]) + slab[0])
            # one node is too few to tell (a 1-D plane); three values are not
            assert differ(rev, true) or true[1].size == 1
        else:
            assert not differ(rev, true)
    assert any(g[2] == 1 for g in K.FOLD_GEOMS)
    assert {len(g[0]) for g in K.FOLD_GEOMS if g[2] == 1} == {1, 2, 3}


def test_fold_order_shows_in_every_dimension_count():
    """the 1-D nloc == 1 plane is one node; with 3 values per node and this
    seed the two orders differ there too"""
    for geom in K.NLOC1:
        slab = K.normals(K.slab_shape(geom, 3), K.SEED["fold"])
        assert differ(FR.fold_self(slab, geom, 3, reverse=True), FR.fold_self(slab, geom, 3))


def _factor_mutants(T, disc):
    """(name, kfactor keywords, is the identity on T by construction)"""
    nd = len(T)
    swapped = (T[0], T[2], T[1]) if nd == 3 else T
    return [("Ty and Tz swapped", dict(Tf=swapped), nd < 3 or T[1] == T[2]),
            # frequencies above T/2 exist from an extent of 3 on; the cosine of
            # the discrete symbol has the period that makes both rules one
            ("unsigned frequency", dict(freq=unsigned), disc or nd == 1 or max(T[1:]) < 3),
            ("DC not zeroed", dict(dc=None), False),
            ("Ntot replaced by the plane size", dict(ntot=int(np.prod(T[:-1]))), False)]


@pytest.mark.parametrize("T", K.SPECTRAL, ids=K.shape_id)
def test_mutants_of_the_factor(T):
    seen = set()
    for disc in K.SYMBOLS:
        rho, hi, d, tol, top = K.spectral_reference(T, disc)
        assert not outside(FR.poisson_fft64(rho, T, disc), hi, tol)
        for name, kw, identity in _factor_mutants(T, disc):
            if name.startswith("Ntot") and len(T) == 1 and not disc:
                continue  # the 1-D continuous factor is written with Tx, not Ntot
            if identity:
                continue
            with np.errstate(invalid="ignore"):  # the DC factor left as computed is 1 / 0
                bad = FR.poisson_fft64(rho, T, disc, factor=FR.kfactor(T, disc, F64, half=True, **kw))
            assert outside(bad, hi, tol), (name, disc)
            seen.add(name)
    assert {"DC not zeroed", "Ntot replaced by the plane size"} <= seen


def test_every_factor_mutant_shows_on_some_single_plan_case():
    names = {n for T in K.SPECTRAL for n, _, identity in _factor_mutants(T, 0) if not identity}
    assert len(names) == 4


@pytest.mark.parametrize("T,P", K.SLAB_SPECTRAL)
def test_mutants_of_the_slab_solve(T, P):
    nloc, Tyl = T[2] // P, T[1] // P
    for disc in K.SYMBOLS:
        rho, hi, d, tol, top = K.spectral_reference(T, disc, K.SEED["slab_spectral"])
        for name, kw, identity in _factor_mutants(T, disc):
            if not identity:
                with np.errstate(invalid="ignore"):
                    bad = FR.slab_poisson(rho, T, P, disc, **kw)
                assert outside(bad, hi, tol), (name, disc)
        if P > 1:
            assert outside(FR.slab_poisson(rho, T, P, disc, y0_of=lambda rank, tyl: 0), hi, tol)
    for r in range(P):
        S, dS, tolS, _ = K.slab_block_reference(T, P, r)
        bad = FR.slab_spectrum_blocks(rho[r * nloc:(r + 1) * nloc], T, P, swapped=True)
        if nloc > 1 and Tyl > 1:
            assert outside(bad, S, tolS)


def test_slab_cases_cover_what_cubes_hide():
    assert any(T[1] != T[2] for T, _ in K.SLAB_SPECTRAL)
    assert any(T[2] // P > 1 and T[1] // P > 1 and T[2] // P != T[1] // P for T, P in K.SLAB_SPECTRAL)
    assert any(T[2] // P == 1 and T[1] // P == 1 for T, P in K.SLAB_SPECTRAL)
    assert any(P > 2 for _, P in K.SLAB_SPECTRAL) and any(P == 1 for _, P in K.SLAB_SPECTRAL)
    assert any(T[1] % 2 and T[2] % 2 for T, _ in K.SLAB_SPECTRAL)


def test_scale2_is_not_one_multiplication():
    """(a * 0.1) * 3.0 != a * (0.1 * 3.0) for most a: the bitwise comparison
    of pinc_hip_scale2 pins the association"""
    (a,) = K.normals((1, 4099), K.SEED["elementwise"])
    assert np.mean((a * 0.1) * 3.0 != a * (0.1 * 3.0)) > 0.25
