"""The multigrid transfer, coarse-cycle and slab kernels of k_mg.hip, each
called through the C ABI and compared with the plain numpy restatement of
tests/mg_ref.py -- bit for bit wherever the kernel's expression order is
fixed, to a stated bound where a sum's order is not.  Inputs are seeded
normals in fp64.  Every output buffer is pre-filled (NaN where the kernel
overwrites, random data where it accumulates) and sits between NaN guard
elements: everything outside the documented write range must come back
unchanged.  tests/test_mg_ref_cpu.py shows that these shapes and inputs tell
deliberate mutants of the restatement apart.
"""
import ctypes as C

import numpy as np
import pytest

import mg_cases as K
import mg_ref as MR
from gpu_buf import Buf, nans, same_bits

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


class Lvl(C.Structure):
    _fields_ = [("nd", C.c_int), ("T", C.c_int * 3)]


def lvl(shape):
    return Lvl(len(shape), (C.c_int * 3)(*(list(shape) + [1] * (3 - len(shape)))))


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available()
    from pinc_amd import _lib
    h = _lib.HIP
    vp, ci, ip = C.c_void_p, C.c_int, C.POINTER(C.c_int)
    h.pinc_hip_gs_pass.argtypes = [vp, vp, Lvl, ci, ci, vp, vp, ip, vp]
    h.pinc_hip_gs_materialize.argtypes = [vp, Lvl, ci, vp, vp, vp]
    h.pinc_hip_reduce.argtypes = [vp, ci, C.c_double, vp, vp]
    h.pinc_hip_residual.argtypes = [vp, vp, vp, Lvl, vp]
    h.pinc_hip_residual_sumsq.argtypes = [vp, vp, Lvl, vp, ip, vp]
    h.pinc_hip_restrict.argtypes = [vp, vp, Lvl, ci, vp]
    h.pinc_hip_prolong_add.argtypes = [vp, vp, Lvl, vp]
    h.pinc_hip_prolong_add3.argtypes = [vp, vp, Lvl, vp]
    h.pinc_hip_resid_restrict.argtypes = [vp, vp, vp, Lvl, ci, C.c_double, vp]
    h.pinc_hip_mg_coarse.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, ci, vp]
    h.pinc_hip_residual_slab.argtypes = [vp, vp, vp, Lvl, ci, ci, vp]
    h.pinc_hip_residual_sumsq_slab.argtypes = [vp, vp, Lvl, ci, ci, vp, ip, vp]
    h.pinc_hip_restrict_slab.argtypes = [vp, Lvl, ci, vp, Lvl, ci, vp]
    h.pinc_hip_prolong_add_own.argtypes = [vp, Lvl, ci, ci, vp, Lvl, vp]
    h.pinc_hip_prolong_add_slab.argtypes = [vp, Lvl, ci, ci, vp, Lvl, vp]
    return h


def forms(nd):
    """the 3-D operator flag: both forms in 3-D, the ND form below"""
    return (0, 1) if nd == 3 else (0,)


def reduced(hip, part, nb, div):
    """pinc_hip_reduce of the first nb block partials"""
    out = Buf(np.full(1, np.nan))
    assert 1 <= nb <= part.n
    assert hip.pinc_hip_reduce(part.ptr, nb, div, out.ptr, None) == 0
    return float(out.get()[0])


# ------------------------------------------------------------ restriction ---

@pytest.mark.parametrize("cshape", K.RESTRICT_COARSE)
def test_restrict(hip, cshape):
    """pinc_hip_restrict (k_restrict<1>, <2>, <3, false>, <3, true>)"""
    nd = len(cshape)
    (f,) = K.fields([K.fine_of(cshape)], K.SEED["restrict"])
    fine = Buf(f)
    for nd3 in forms(nd):
        coarse = Buf(nans(cshape))
        assert hip.pinc_hip_restrict(fine.ptr, coarse.ptr, lvl(cshape), nd3, None) == 0
        np.testing.assert_array_equal(coarse.get(), MR.restrict(f, nd, nd3))
    assert fine.unchanged()


# ----------------------------------------------------------- prolongation ---

@pytest.mark.parametrize("fshape", K.PROLONG_FINE)
def test_prolong_add(hip, fshape):
    """pinc_hip_prolong_add (k_prolong_add<1..3>) and, in 3-D,
    pinc_hip_prolong_add3 (k_prolong_add3c: a thread per coarse cell), each
    against fine0 + prolong(coarse), and against each other"""
    nd = len(fshape)
    cshape = K.coarse_of(fshape)
    f0, c = K.fields([fshape, cshape], K.SEED["prolong"])
    want = f0 + MR.prolong(c, nd)
    coarse = Buf(c)
    fine = Buf(f0)
    assert hip.pinc_hip_prolong_add(fine.ptr, coarse.ptr, lvl(fshape), None) == 0
    got = fine.get()
    np.testing.assert_array_equal(got, want)
    if nd == 3:
        fine3 = Buf(f0)
        assert hip.pinc_hip_prolong_add3(fine3.ptr, coarse.ptr, lvl(cshape), None) == 0
        got3 = fine3.get()
        np.testing.assert_array_equal(got3, want)
        assert same_bits(got3, got)
    assert coarse.unchanged()


def test_prolong_add3_rejects_an_unaligned_fine_grid(hip):
    fshape = (6, 10, 14)
    f0, c = K.fields([fshape, K.coarse_of(fshape)], K.SEED["prolong"])
    fine, coarse = Buf(f0, off=1), Buf(c)
    assert fine.ptr % 16 == 8
    assert hip.pinc_hip_prolong_add3(fine.ptr, coarse.ptr, lvl(K.coarse_of(fshape)), None) != 0
    assert fine.unchanged()


# --------------------------------------------------------------- residual ---

@pytest.mark.parametrize("shape,off", K.RESIDUAL)
def test_residual_and_its_sum_of_squares(hip, shape, off):
    """pinc_hip_residual (k_residual<1..3>) bit for bit, and
    pinc_hip_residual_sumsq against the long-double sum: the x-pair kernel on
    aligned 3-D levels of even x extent, the generic k_residual_sumsq<ND> on an
    odd x extent, on arrays offset by 8 bytes, and in 1-D and 2-D"""
    nd = len(shape)
    a, r = K.fields([shape, shape], K.SEED["residual"])
    phi, rho, res = Buf(a, off), Buf(r, off), Buf(nans(shape))
    assert phi.ptr % 16 == 8 * off
    assert hip.pinc_hip_residual(res.ptr, phi.ptr, rho.ptr, lvl(shape), None) == 0
    want = MR.residual(a, r, nd)
    np.testing.assert_array_equal(res.get(), want)
    part = Buf(np.full(2048, np.nan))
    nb = C.c_int()
    assert hip.pinc_hip_residual_sumsq(phi.ptr, rho.ptr, lvl(shape), part.ptr, C.byref(nb), None) == 0
    tot = reduced(hip, part, nb.value, 1.0)
    assert np.all(np.isnan(part.get()[nb.value:]))
    w = want.astype(LD)
    np.testing.assert_allclose(tot, float((w * w).sum(dtype=LD)), rtol=1e-12)
    assert phi.unchanged() and rho.unchanged()


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset8"])
@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("hw3d", [1, 0])
@pytest.mark.parametrize("fshape", K.RESID_RESTRICT_FINE)
def test_resid_restrict(hip, fshape, hw3d, scale, off):
    """pinc_hip_resid_restrict against restrict(residual) * scale of the
    restatement: the x-pair kernel on aligned arrays, k_resid_restrict3 on
    arrays offset by 8 bytes"""
    a, r = K.fields([fshape, fshape], K.SEED["resid_restrict"])
    cshape = K.coarse_of(fshape)
    phi, rho, coarse = Buf(a, off), Buf(r, off), Buf(nans(cshape))
    assert phi.ptr % 16 == 8 * off and rho.ptr % 16 == 8 * off
    assert hip.pinc_hip_resid_restrict(phi.ptr, rho.ptr, coarse.ptr, lvl(cshape), hw3d, scale, None) == 0
    np.testing.assert_array_equal(coarse.get(), MR.restrict(MR.residual(a, r, 3), 3, hw3d) * scale)
    assert phi.unchanged() and rho.unchanged()


# -------------------------------------------------- parity mode's smoother ---

@pytest.mark.parametrize("shape,nd3", [(s, f) for s in K.GS_SHAPES for f in forms(len(s))])
def test_gs_passes_with_lazy_means(hip, shape, nd3):
    """Three iterations by the host's protocol (pinc_mg.c: smooth): pass k
    reads the other colour less mu[k - 1], its block partials reduce to
    mu[k], and pinc_hip_gs_materialize applies mu[4] and mu[5].  The
    materialised grid equals, bit for bit, the colour updates with a
    subtraction of the device's own mu[k] from every point after each; and
    each mu[k] is the mean of the reference grid at that pass to 2 n eps
    mean|a| (any summation order, plus the pair add)."""
    nd = len(shape)
    a, r = K.fields([shape, shape], K.SEED["gs"])
    n = a.size
    phi, rho = Buf(a), Buf(r)
    part = Buf(np.full(2048, np.nan))
    mu = Buf(np.full(6, np.nan))
    nb = C.c_int()
    for k in range(6):
        prev = mu.ptr + 8 * (k - 1) if k else None
        assert hip.pinc_hip_gs_pass(phi.ptr, rho.ptr, lvl(shape), k & 1, nd3, prev, part.ptr, C.byref(nb), None) == 0
        assert 1 <= nb.value <= 2048
        assert hip.pinc_hip_reduce(part.ptr, nb.value, float(n), mu.ptr + 8 * k, None) == 0
    assert hip.pinc_hip_gs_materialize(phi.ptr, lvl(shape), 1, mu.ptr + 8 * 4, mu.ptr + 8 * 5, None) == 0
    mus = mu.get().copy()
    assert np.all(np.isfinite(mus))
    want, seen = MR.gs_eager(a, r, nd, nd3, mus)
    np.testing.assert_array_equal(phi.get(), want)
    for k in range(6):
        g = seen[k].astype(LD)
        mean = g.sum(dtype=LD) / n
        bound = 2 * n * EPS * float(np.abs(g).sum(dtype=LD) / n)
        assert abs(LD(mus[k]) - mean) <= bound, (k, mus[k], float(mean), bound)
    assert rho.unchanged()


@pytest.mark.parametrize("shape", [s for s in K.GS_SHAPES if len(s) < 3])
def test_gs_pass_without_means(hip, shape):
    """a red and a black pass with partial = NULL and muPrev = NULL (native
    mode), 1-D and 2-D"""
    nd = len(shape)
    a, r = K.fields([shape, shape], K.SEED["gs"])
    phi, rho = Buf(a), Buf(r)
    nb = C.c_int()
    want = a
    for colour in (0, 1):
        assert hip.pinc_hip_gs_pass(phi.ptr, rho.ptr, lvl(shape), colour, 0, None, None, C.byref(nb), None) == 0
        want = MR.gs_colour(want, r, colour, nd, 0)
        np.testing.assert_array_equal(phi.get(), want)


# ----------------------------------------------------------- coarse cycle ---

def _levels(shapes, nds=None):
    return (Lvl * len(shapes))(*[lvl(s) if nds is None else Lvl(nds[i], lvl(s).T) for i, s in enumerate(shapes)])


@pytest.mark.parametrize("case", K.COARSE, ids=[f"{'x'.join(map(str, c[0][0]))}-{len(c[0])}lv-hw{c[1]}gs{c[2]}"
                                                for c in K.COARSE])
def test_mg_coarse(hip, case):
    """pinc_hip_mg_coarse (the V-cycle of the coarse levels in one workgroup)
    against coarse_cycle.  The workgroup's neutralisation sums run in another
    order than numpy's, so the bound is measured from the restatement alone:
    d = max |cycle_f64 - cycle_longdouble|, and the kernel must be within
    max(16 d, 64 eps max|phi|) of cycle_f64 (mg_cases.coarse_reference).  The
    correction's mean must be zero to n eps max|phi|.

    Measured on an MI355X (d, the kernel's deviation, the bound; the floor
    64 eps max|phi| is what binds in every case):
      16^3 -> 2^3, hw3d = gs3d = 1   9.49e-16  4.44e-16  2.17e-14
      16^3 -> 2^3, both 0            8.77e-16  4.44e-16  2.17e-14
      16x8x4 -> 8x4x2                4.76e-16  3.33e-16  1.57e-14
      4^3 alone                      8.49e-17  1.11e-16  8.06e-15
      32x16 -> 4x2                   7.84e-16  8.88e-16  5.44e-14
      64 -> 2                        6.08e-15  7.11e-15  3.55e-13
    """
    levels, hw3d, gs3d = case
    rho0, ref, d, tol = K.coarse_reference(case)
    pre, post, nc = K.COARSE_SMOOTH
    rho, phi = Buf(rho0), Buf(nans(levels[0]))
    assert hip.pinc_hip_mg_coarse(rho.ptr, phi.ptr, len(levels), _levels(levels), pre, post, nc, hw3d, gs3d, None) == 0
    got = phi.get()
    dev = float(np.max(np.abs(got - ref)))
    top = float(np.max(np.abs(ref)))
    print(f"mg_coarse {levels[0]} x{len(levels)} hw3d={hw3d} gs3d={gs3d}: d = {d:.3e}, kernel deviation = {dev:.3e}, "
          f"bound = {tol:.3e}, max|phi| = {top:.3e}")
    assert np.all(np.isfinite(got))
    assert dev <= tol
    assert abs(float(got.astype(LD).sum(dtype=LD) / got.size)) <= got.size * EPS * top
    assert rho.unchanged()


@pytest.mark.parametrize("shapes,nds,hw3d", [
    ([(8, 8, 8), (4, 4, 2)], None, 1),        # levels that do not halve
    ([(8, 8, 8), (4, 4, 1)], [3, 2], 0),      # mixed dimensions
    ([(8, 8)], None, 1),                      # hw3d on a 2-D grid
    ([(5501,)], None, 0),                     # one point over the LDS budget
], ids=["not-halving", "mixed-nd", "hw3d-2d", "5501-points"])
def test_mg_coarse_rejects(hip, shapes, nds, hw3d):
    """the argument checks return nonzero and launch nothing"""
    (r,) = K.fields([shapes[0]], K.SEED["coarse"])
    rho, phi = Buf(r), Buf(nans(shapes[0]))
    assert hip.pinc_hip_mg_coarse(rho.ptr, phi.ptr, len(shapes), _levels(shapes, nds), 4, 4, 10, hw3d, 0, None) != 0
    assert phi.unchanged()


# ------------------------------------------------------- sharded level 0 ---

@pytest.fixture(scope="module")
def slab_problem():
    """per case of K.SLABS: the global periodic problem and its global
    results, computed once"""
    cache = {}

    def get(T):
        if T not in cache:
            phi, rho, corr = K.fields([T, T, K.coarse_of(T)], K.SEED["slab"])
            res = MR.residual(phi, rho, 3)
            for x in (phi, rho, corr, res):
                x.setflags(write=False)
            cache[T] = dict(phi=phi, rho=rho, corr=corr, res=res, pro=phi + MR.prolong(corr, 3),
                            restr=[MR.restrict(res, 3, f) * 4.0 for f in (0, 1)])
        return cache[T]
    return get


SLAB_RANKS = [(T, P, hz, rank) for T, P, hz in K.SLABS for rank in range(P)]


@pytest.mark.parametrize("T,P,hz,rank", SLAB_RANKS)
def test_slab_residual_and_restriction(hip, slab_problem, T, P, hz, rank):
    """residual_slab on planes [hz - 1, hz + nloc), as the host calls it,
    equals the global residual's planes and leaves every other plane of res
    alone; residual_sumsq_slab on the owned planes; restrict_slab(zf0 = hz)
    equals the rank's planes of restrict(residual) * 4"""
    g = slab_problem(T)
    nloc = T[2] // P
    X = (T[0], T[1], nloc + 2 * hz)
    phi = Buf(MR.extended_slab(g["phi"], rank, nloc, hz))
    rho = Buf(MR.extended_slab(g["rho"], rank, nloc, hz))
    res = Buf(nans(X))
    assert hip.pinc_hip_residual_slab(res.ptr, phi.ptr, rho.ptr, lvl(X), hz - 1, hz + nloc, None) == 0
    want = nans(X)
    want[hz - 1:hz + nloc] = g["res"][(rank * nloc + np.arange(-1, nloc)) % T[2]]
    np.testing.assert_array_equal(res.get(), want)
    part = Buf(np.full(2048, np.nan))
    nb = C.c_int()
    assert hip.pinc_hip_residual_sumsq_slab(phi.ptr, rho.ptr, lvl(X), hz, hz + nloc, part.ptr, C.byref(nb), None) == 0
    own = g["res"][rank * nloc:(rank + 1) * nloc].astype(LD)
    np.testing.assert_allclose(reduced(hip, part, nb.value, 1.0), float((own * own).sum(dtype=LD)), rtol=1e-12)
    cs = (T[0] // 2, T[1] // 2, nloc // 2)
    for nd3 in (0, 1):
        coarse = Buf(nans(cs))
        assert hip.pinc_hip_restrict_slab(res.ptr, lvl(X), hz, coarse.ptr, lvl(cs), nd3, None) == 0
        np.testing.assert_array_equal(coarse.get(), g["restr"][nd3][rank * nloc // 2:(rank + 1) * nloc // 2])
    assert phi.unchanged() and rho.unchanged()


@pytest.mark.parametrize("T,P,hz,rank", SLAB_RANKS)
def test_slab_prolongations(hip, slab_problem, T, P, hz, rank):
    """prolong_add_slab(z0 = rank nloc - hz) equals the extended slab of
    glob + prolong(coarse) on every plane; prolong_add_own, given the rank's
    coarse planes and one wrapped halo plane on each side, equals it on the
    owned planes and leaves the halo planes alone"""
    g = slab_problem(T)
    nloc = T[2] // P
    X = (T[0], T[1], nloc + 2 * hz)
    px = MR.extended_slab(g["phi"], rank, nloc, hz)
    want = MR.extended_slab(g["pro"], rank, nloc, hz)
    C1 = K.coarse_of(T)
    corr = Buf(g["corr"])
    phi = Buf(px)
    assert hip.pinc_hip_prolong_add_slab(phi.ptr, lvl(X), rank * nloc - hz, T[2], corr.ptr, lvl(C1), None) == 0
    np.testing.assert_array_equal(phi.get(), want)
    cxs = (C1[0], C1[1], nloc // 2 + 2)
    cx = Buf(MR.extended_slab(g["corr"], rank, nloc // 2, 1))
    assert cx.shape == cxs[::-1]
    phi = Buf(px)
    assert hip.pinc_hip_prolong_add_own(phi.ptr, lvl(X), hz, nloc, cx.ptr, lvl(cxs), None) == 0
    got = phi.get()
    np.testing.assert_array_equal(got[hz:hz + nloc], want[hz:hz + nloc])
    assert same_bits(got[:hz], px[:hz]) and same_bits(got[hz + nloc:], px[hz + nloc:])
    assert corr.unchanged() and cx.unchanged()


def test_slab_entry_points_reject_bad_geometry(hip):
    """one bad argument per entry point: nonzero, nothing written"""
    T, nloc, hz = (8, 4, 16), 8, 2
    X = (T[0], T[1], nloc + 2 * hz)
    C1 = K.coarse_of(T)
    a, r, c = K.fields([X, X, C1], K.SEED["slab"])
    phi, rho, res = Buf(a), Buf(r), Buf(nans(X))
    # zlo = 0: plane 0 has no lower z neighbour in the slab
    assert hip.pinc_hip_residual_slab(res.ptr, phi.ptr, rho.ptr, lvl(X), 0, hz + nloc, None) != 0
    assert res.unchanged()
    # zf0 + 2 Tc[2] > T[2]
    cs = (T[0] // 2, T[1] // 2, nloc // 2)
    coarse = Buf(nans(cs))
    assert hip.pinc_hip_restrict_slab(phi.ptr, lvl(X), X[2] - 2 * cs[2] + 1, coarse.ptr, lvl(cs), 1, None) != 0
    assert coarse.unchanged()
    # odd nloc
    cx = Buf(np.zeros((nloc // 2 + 2, C1[1], C1[0])))
    assert hip.pinc_hip_prolong_add_own(phi.ptr, lvl(X), hz, nloc - 1, cx.ptr, lvl((C1[0], C1[1], nloc // 2 + 2)),
                                        None) != 0
    # 2 Tc[2] != Tz
    corr = Buf(c)
    assert hip.pinc_hip_prolong_add_slab(phi.ptr, lvl(X), -hz, T[2] + 2, corr.ptr, lvl(C1), None) != 0
    assert phi.unchanged()
