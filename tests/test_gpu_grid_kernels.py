"""The grid glue of k_grid.hip, each entry point called through the C ABI and
compared with the plain numpy restatement of tests/field_ref.py: bit for bit
everywhere (the build has -ffp-contract=off and every expression's order is
fixed), the reductions also against long-double sums under a bound read off
the code.  Inputs are seeded normals in fp64.  Every output buffer is
pre-filled (NaN where the kernel overwrites, random data where it
accumulates) and sits between NaN guard elements (tests/gpu_buf.py):
everything outside the documented write range must come back unchanged.
tests/test_field_ref_cpu.py shows that these shapes and inputs tell
deliberate mutants of the restatement apart.
"""
import ctypes as C

import numpy as np
import pytest

import field_cases as K
import field_ref as FR
from gpu_buf import Buf, same_bits

pytestmark = pytest.mark.gpu

LD = np.longdouble


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available()
    from pinc_amd import _lib
    h, G = _lib.HIP, _lib.HipGeom
    vp, ci, cl, cd = C.c_void_p, C.c_int, C.c_long, C.c_double
    h.pinc_hip_efield.argtypes = [vp, G, vp, vp]
    h.pinc_hip_efield_scaled.argtypes = [vp, G, vp, cd, vp]
    h.pinc_hip_slab_from_global.argtypes = [vp, vp, G, ci, vp]
    h.pinc_hip_fold_self.argtypes = [vp, G, vp]
    h.pinc_hip_fold_self_values.argtypes = [vp, G, ci, vp]
    h.pinc_hip_add.argtypes = [vp, vp, cl, vp]
    h.pinc_hip_add_plane.argtypes = [vp, G, ci, vp, vp]
    h.pinc_hip_copy_plane.argtypes = [vp, vp, G, ci, ci, vp]
    h.pinc_hip_zero.argtypes = [vp, cl, vp]
    h.pinc_hip_scale.argtypes = [vp, cl, cd, vp]
    h.pinc_hip_scale2.argtypes = [vp, cl, cd, cd, vp]
    h.pinc_hip_sub_dev.argtypes = [vp, cl, vp, vp]
    h.pinc_hip_extrapolate.argtypes = [vp, vp, cl, vp]
    h.pinc_hip_lincomb.argtypes = [vp, vp, cd, vp, cd, cl, vp]
    h.pinc_hip_sum.argtypes = [vp, cl, vp, vp, vp]
    h.pinc_hip_sum_div.argtypes = [vp, cl, cd, vp, vp, vp]
    h.pinc_hip_dot.argtypes = [vp, vp, cl, vp, vp, vp]
    return h


def geom(g):
    from pinc_amd._lib import HipGeom
    T, off, nloc = g
    return HipGeom(len(T), (C.c_int * 3)(*(list(T) + [1] * (3 - len(T)))), nloc, off, 1, 0)


def assert_bits(got, want):
    assert got.shape == want.shape
    if not same_bits(got, want):
        np.testing.assert_array_equal(got, want)  # says where
        raise AssertionError("equal values, other bits (a zero's sign)")


# ----------------------------------------------------------------- efield ---

@pytest.mark.parametrize("g", K.GEOMS, ids=K.geom_id)
def test_efield(hip, g):
    """pinc_hip_efield_scaled with h = 0.5 and -0.5, and pinc_hip_efield, bit
    for bit.  k_efield_planes<ND> serves every geometry up to nloc + 2 =
    65535 planes (the 1-D case of 65533 cells is its last), k_efield<ND> (the
    grid stride) the three above: both are held to the one restatement, so
    they agree with each other through it."""
    T = g[0]
    nd = len(T)
    p = K.normals(T[::-1], K.SEED["efield"])
    phi = Buf(p)
    shape = K.slab_shape(g, nd)
    for h in K.H:
        E = Buf(np.full(shape, np.nan))
        assert hip.pinc_hip_efield_scaled(phi.ptr, geom(g), E.ptr, h, None) == 0
        assert_bits(E.get(), FR.efield_slab(p, g, h))
    E = Buf(np.full(shape, np.nan))
    assert hip.pinc_hip_efield(phi.ptr, geom(g), E.ptr, None) == 0
    assert_bits(E.get(), FR.efield_slab(p, g, 0.5))
    assert phi.unchanged()


def test_efield_rejects_another_factor(hip):
    g = ((30, 20, 12), 4, 4)
    phi = Buf(K.normals(g[0][::-1], K.SEED["efield"]))
    E = Buf(np.full(K.slab_shape(g, 3), np.nan))
    assert hip.pinc_hip_efield_scaled(phi.ptr, geom(g), E.ptr, 0.25, None) != 0
    assert b"efield" in hip.pinc_hip_error_string()
    assert E.unchanged()


# ------------------------------------------------------------ slab planes ---

@pytest.mark.parametrize("nv", K.NVALUES)
@pytest.mark.parametrize("g", K.GEOMS, ids=K.geom_id)
def test_slab_from_global(hip, g, nv):
    a = K.normals(g[0][::-1] + (nv,), K.SEED["slab"])
    glob = Buf(a)
    slab = Buf(np.full(K.slab_shape(g, nv), np.nan))
    assert hip.pinc_hip_slab_from_global(slab.ptr, glob.ptr, geom(g), nv, None) == 0
    assert_bits(slab.get(), FR.slab_from_global(a, g, nv))
    assert glob.unchanged()


@pytest.mark.parametrize("g", K.FOLD_GEOMS, ids=K.geom_id)
def test_fold_self(hip, g):
    """pinc_hip_fold_self and pinc_hip_fold_self_values (1 and 3 values per
    node): the upper ghost plane into plane 1, then the lower into plane nloc
    -- with nloc == 1 both into plane 1, (p1 + p2) + p0 -- and the ghost
    planes themselves left alone"""
    nloc = g[2]
    a = K.normals(K.slab_shape(g), K.SEED["fold"])
    slab = Buf(a)
    assert hip.pinc_hip_fold_self(slab.ptr, geom(g), None) == 0
    got = slab.get()
    assert_bits(got, FR.fold_self(a, g))
    assert same_bits(got[0], a[0]) and same_bits(got[nloc + 1], a[nloc + 1])
    for nv in K.NVALUES:
        a = K.normals(K.slab_shape(g, nv), K.SEED["fold"])
        slab = Buf(a)
        assert hip.pinc_hip_fold_self_values(slab.ptr, geom(g), nv, None) == 0
        got = slab.get()
        assert_bits(got, FR.fold_self(a, g, nv))
        assert same_bits(got[0], a[0]) and same_bits(got[nloc + 1], a[nloc + 1])
    assert hip.pinc_hip_fold_self_values(slab.ptr, geom(g), 0, None) != 0
    assert same_bits(slab.get(), got)


@pytest.mark.parametrize("g", K.FOLD_GEOMS, ids=K.geom_id)
def test_add_plane_and_copy_plane(hip, g):
    nloc = g[2]
    a = K.normals(K.slab_shape(g), K.SEED["plane"])
    inp = K.normals(a.shape[1:], K.SEED["plane"] + 1)
    src = Buf(inp)
    for plane in sorted({0, 1, nloc, nloc + 1}):
        slab = Buf(a)
        assert hip.pinc_hip_add_plane(slab.ptr, geom(g), plane, src.ptr, None) == 0
        assert_bits(slab.get(), FR.add_plane(a, plane, inp))
    assert src.unchanged()
    for nv in K.NVALUES:
        a = K.normals(K.slab_shape(g, nv), K.SEED["plane"])
        slab = Buf(a)
        for plane in sorted({0, 1, nloc, nloc + 1}):
            dst = Buf(np.full(a.shape[1:], np.nan))
            assert hip.pinc_hip_copy_plane(dst.ptr, slab.ptr, geom(g), plane, nv, None) == 0
            assert_bits(dst.get(), FR.copy_plane(a, plane))
        assert slab.unchanged()


# ------------------------------------------------------------ elementwise ---

@pytest.mark.parametrize("n", K.N_ELEMENTS)
def test_elementwise(hip, n):
    """zero, scale, scale2 ((a f1) f2, not a (f1 f2)), sub_dev (mu read from
    device memory), add, extrapolate (both outputs), lincomb with a separate
    output and in place on x and on y, as pinc_mg.c calls it"""
    a, b = K.normals((2, n), K.SEED["elementwise"])
    x = Buf(a)
    assert hip.pinc_hip_zero(x.ptr, n, None) == 0
    assert_bits(x.get(), np.zeros(n))
    x = Buf(a)
    assert hip.pinc_hip_scale(x.ptr, n, -1.7, None) == 0
    assert_bits(x.get(), a * -1.7)
    x = Buf(a)
    f1, f2 = 0.1, 3.0
    assert hip.pinc_hip_scale2(x.ptr, n, f1, f2, None) == 0
    assert_bits(x.get(), (a * f1) * f2)
    if n >= 255:
        assert np.mean((a * f1) * f2 != a * (f1 * f2)) > 0.25
    x, mu = Buf(a), Buf(np.array([0.3125 + 1e-3]))
    assert hip.pinc_hip_sub_dev(x.ptr, n, mu.ptr, None) == 0
    assert_bits(x.get(), a - (0.3125 + 1e-3))
    assert mu.unchanged()
    x, y = Buf(a), Buf(b)
    assert hip.pinc_hip_add(x.ptr, y.ptr, n, None) == 0
    assert_bits(x.get(), a + b)
    assert y.unchanged()
    phi, prev = Buf(a), Buf(b)
    assert hip.pinc_hip_extrapolate(phi.ptr, prev.ptr, n, None) == 0
    assert_bits(phi.get(), 2.0 * a - b)
    assert_bits(prev.get(), a)
    ca, cb = 0.7, -1.3
    want = ca * a + cb * b
    x, y, out = Buf(a), Buf(b), Buf(np.full(n, np.nan))
    assert hip.pinc_hip_lincomb(out.ptr, x.ptr, ca, y.ptr, cb, n, None) == 0
    assert_bits(out.get(), want)
    assert x.unchanged() and y.unchanged()
    assert hip.pinc_hip_lincomb(x.ptr, x.ptr, ca, y.ptr, cb, n, None) == 0  # out is x
    assert_bits(x.get(), want)
    assert y.unchanged()
    x = Buf(a)
    assert hip.pinc_hip_lincomb(y.ptr, x.ptr, ca, y.ptr, cb, n, None) == 0  # out is y
    assert_bits(y.get(), want)
    assert x.unchanged()


@pytest.mark.parametrize("n", [0, -5])
def test_elementwise_with_nothing_to_do(hip, n):
    """n <= 0 returns 0 and writes nothing"""
    a, b = K.normals((2, 64), K.SEED["elementwise"])
    x, y, mu = Buf(a), Buf(b), Buf(np.array([0.5]))
    assert hip.pinc_hip_zero(x.ptr, n, None) == 0
    assert hip.pinc_hip_scale(x.ptr, n, 2.0, None) == 0
    assert hip.pinc_hip_scale2(x.ptr, n, 2.0, 3.0, None) == 0
    assert hip.pinc_hip_sub_dev(x.ptr, n, mu.ptr, None) == 0
    assert hip.pinc_hip_add(x.ptr, y.ptr, n, None) == 0
    assert hip.pinc_hip_extrapolate(x.ptr, y.ptr, n, None) == 0
    assert hip.pinc_hip_lincomb(x.ptr, x.ptr, 2.0, y.ptr, 3.0, n, None) == 0
    assert x.unchanged() and y.unchanged()


# ------------------------------------------------------------- reductions ---

@pytest.mark.parametrize("n", K.N_ELEMENTS)
def test_sum_sum_div_and_dot(hip, n):
    """pinc_hip_sum, pinc_hip_sum_div and pinc_hip_dot against long-double
    sums, within D eps sum|a_i| (sum|a_i b_i| for the dot product; divided by
    |div| for sum_div).  D is the most roundings one term passes through,
    read off k_sum, k_reduce and block_sum (field_ref.tree_depth):

      k_sum     nb = min(ceil(n / 2048), 1024) blocks of 256 threads; a thread
                adds its ceil(n / (256 nb)) terms in turn, the first to 0.
                (exact): at most 9 - 1 = 8 roundings at n = 2097229
                (a product first for the dot: 1 more)
      wave_sum  6 xor-shuffle stages: 6
      block_sum thread 0 adds the 4 waves' sums in turn, the first to 0.: 3
      k_reduce  one block over the nb partials: ceil(nb / 256) - 1 <= 3,
                then 6 and 3 as above
      division  1 (sum_div)

    D = 8 + 6 + 3 + 3 + 6 + 3 = 29 for the largest n (30 for sum_div and for
    dot), 18 for n <= 2048.  Each rounding is at most eps / 2 relative, so
    D eps bounds (1 + eps/2)^D - 1 with room for the higher orders.

    The restatement (field_ref.tree_sum) reproduces that tree addition by
    addition, so value and block partials also match it bit for bit; two
    calls return identical bits; the partial buffer holds exactly
    red_blocks(n) entries between its guards.

    Measured on an MI355X at n = 2097229 (deviation from the long-double
    value, bound): sum 4.593e-13, 1.078e-08; sum_div 9.553e-20, 1.772e-15;
    dot 3.336e-14, 8.894e-09."""
    a, b = K.normals((2, n), K.SEED["reduce"])
    x, y = Buf(a), Buf(b)
    nb = min(max(-(-n // 2048), 1), 1024)
    div = 3.0 * n
    calls = [("sum", lambda p, o: hip.pinc_hip_sum(x.ptr, n, p, o, None), None, 1.0),
             ("sum_div", lambda p, o: hip.pinc_hip_sum_div(x.ptr, n, div, p, o, None), None, div),
             ("dot", lambda p, o: hip.pinc_hip_dot(x.ptr, y.ptr, n, p, o, None), b, 1.0)]
    for name, call, bb, dv in calls:
        got = []
        for _ in range(2):
            part, out = Buf(np.full(nb, np.nan)), Buf(np.full(1, np.nan))
            assert call(part.ptr, out.ptr) == 0
            got.append((out.get().copy(), part.get().copy()))
        assert same_bits(got[0][0], got[1][0]) and same_bits(got[0][1], got[1][1])
        val, partials = got[0]
        terms = a.astype(LD) * (1 if bb is None else bb.astype(LD))
        exact = terms.sum(dtype=LD) / LD(dv)
        D = FR.tree_depth(n, bb is not None, dv != 1.0)
        bound = D * K.EPS * float(np.abs(terms).sum(dtype=LD)) / dv
        print(f"{name} n = {n}: D = {D}, deviation = {abs(float(LD(val[0]) - exact)):.3e}, bound = {bound:.3e}")
        assert abs(LD(val[0]) - exact) <= bound
        want, wpart = FR.tree_sum(a, bb, dv)
        assert_bits(partials, wpart)
        assert_bits(val, np.array([want]))
    assert x.unchanged() and y.unchanged()
