"""The spectral Poisson solve of k_spectral.hip through the C ABI: the
single-plan solve (k_spectral_scale between rocFFT's transforms) and the
slab-distributed solve (k_slab_pack, k_slab_scale, k_slab_unpack) with all P
ranks emulated by P plans in this one process, the all-to-all done with
device copies.  The reference is tests/field_ref.py's dense-DFT solve in long
double; the bound comes from the references alone
(field_cases.spectral_tolerance): d = max |numpy.fft in fp64 - long double|,
tolerance max(16 d, 64 eps max|phi|), never above 1e-11 max|phi|.
tests/test_field_ref_cpu.py shows that every deliberate defect of the factor
and of the block layout lands outside that bound on these cases.
"""
import ctypes as C

import numpy as np
import pytest

import field_cases as K
from gpu_buf import Buf, nans

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available()
    from pinc_amd import _lib
    h = _lib.HIP
    vp, ci, ip, pp = C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p)
    h.pinc_hip_fft_create.argtypes = [pp, ci, ip, vp]
    h.pinc_hip_fft_set_symbol.argtypes = [vp, ci]
    h.pinc_hip_fft_poisson.argtypes = [vp, vp, vp, vp]
    h.pinc_hip_fft_destroy.argtypes = [vp]
    h.pinc_hip_fft_destroy.restype = None
    h.pinc_hip_fft_slab_create.argtypes = [pp, ip, ci, ci, ci, vp]
    h.pinc_hip_fft_slab_buffers.argtypes = [vp, pp, pp, C.POINTER(C.c_long)]
    h.pinc_hip_fft_slab_set_symbol.argtypes = [vp, ci]
    h.pinc_hip_fft_slab_forward.argtypes = [vp, vp, vp]
    h.pinc_hip_fft_slab_kspace.argtypes = [vp, vp]
    h.pinc_hip_fft_slab_backward.argtypes = [vp, vp, vp]
    h.pinc_hip_fft_slab_destroy.argtypes = [vp]
    h.pinc_hip_fft_slab_destroy.restype = None
    h.pinc_hip_d2h.argtypes = [vp, vp, C.c_ulong, vp]
    h.pinc_hip_d2d.argtypes = [vp, vp, C.c_ulong, vp]
    return h


def ints(T):
    return (C.c_int * len(T))(*T)


def solve(hip, T, discrete, rho):
    """create, set_symbol, poisson, destroy: phi between guards, rho
    untouched"""
    plan = C.c_void_p()
    assert hip.pinc_hip_fft_create(C.byref(plan), len(T), ints(T), None) == 0 and plan.value
    try:
        assert hip.pinc_hip_fft_set_symbol(plan, discrete) == 0
        src, phi = Buf(rho), Buf(nans(T))
        assert hip.pinc_hip_fft_poisson(plan, src.ptr, phi.ptr, None) == 0
        got = phi.get().copy()
        assert src.unchanged()
    finally:
        hip.pinc_hip_fft_destroy(plan)
    return got


@pytest.mark.parametrize("discrete", K.SYMBOLS, ids=["continuous", "discrete"])
@pytest.mark.parametrize("T", K.SPECTRAL, ids=K.shape_id)
def test_single_plan_solve(hip, T, discrete):
    """pinc_hip_fft_poisson against the long-double solve.

    Measured on an MI355X (d, the kernel's deviation, the tolerance):
      2         continuous  4.762e-18  4.762e-18  3.438e-16
      2         discrete    0.000e+00  0.000e+00  8.483e-16
      8         continuous  4.225e-16  4.225e-16  1.622e-14
      8         discrete    4.935e-16  2.836e-16  1.733e-14
      16        continuous  7.488e-16  9.272e-16  7.325e-14
      16        discrete    1.860e-15  2.209e-15  7.447e-14
      2x2       continuous  1.086e-17  1.086e-17  1.965e-15
      2x2       discrete    6.939e-18  4.857e-17  4.848e-15
      8x5       continuous  1.841e-16  1.722e-16  1.279e-14
      8x5       discrete    1.575e-16  2.726e-16  1.398e-14
      6x16      continuous  6.199e-16  5.251e-16  2.618e-14
      6x16      discrete    8.561e-16  6.381e-16  2.851e-14
      2x2x2     continuous  8.638e-18  1.173e-17  1.330e-15
      2x2x2     discrete    3.455e-17  8.531e-18  3.281e-15
      8x5x7     continuous  2.085e-16  2.366e-16  8.858e-15
      8x5x7     discrete    3.308e-16  3.377e-16  1.101e-14
      4x6x3     continuous  1.314e-16  8.634e-17  7.034e-15
      4x6x3     discrete    1.248e-16  1.327e-16  9.123e-15
      16x8x4    continuous  2.822e-16  4.217e-16  1.383e-14
      16x8x4    discrete    4.315e-16  5.508e-16  1.554e-14
    The floor 64 eps max|phi| is what binds in every case.
    """
    rho, ref, d, tol, top = K.spectral_reference(T, discrete)
    got = solve(hip, T, discrete, rho)
    dev = float(np.max(np.abs(got - ref)))
    print(f"fft_poisson {K.shape_id(T)} discrete={discrete}: d = {d:.3e}, kernel deviation = {dev:.3e}, "
          f"tolerance = {tol:.3e}, max|phi| = {top:.3e}")
    assert np.all(np.isfinite(got))
    assert dev <= tol


@pytest.mark.parametrize("T,P", K.SLAB_SPECTRAL, ids=[f"{K.shape_id(T)}-P{P}" for T, P in K.SLAB_SPECTRAL])
def test_slab_solve_with_every_rank_in_this_process(hip, T, P):
    """forward on each rank's planes; each rank's send buffer S against
    slab_spectrum_blocks (k_slab_pack alone); the all-to-all as device copies
    (block q of rank r's S into block r of rank q's B); kspace on each rank;
    the copies back; backward on each rank.  The assembled phi is within the
    bound of the long-double solve and of the single-plan solve.  Both
    symbols run on the same P plans (making them is most of the time).

    Measured on an MI355X (d, the kernel's deviation, the tolerance; S: the
    largest over the ranks):
      8x6x9 P=3    S           3.556e-15  3.845e-15  1.930e-13
      8x6x9 P=3    phi contin. 1.503e-16  2.400e-16  8.049e-15  (single plan: 1.665e-16)
      8x6x9 P=3    phi discr.  3.077e-16  2.522e-16  1.033e-14  (single plan: 2.220e-16)
      4x4x4 P=4    S           5.008e-16  1.247e-15  8.631e-14
      4x4x4 P=4    phi contin. 9.300e-17  9.300e-17  4.901e-15  (single plan: 1.388e-16)
      4x4x4 P=4    phi discr.  1.061e-16  1.338e-16  7.612e-15  (single plan: 2.220e-16)
      8x6x4 P=2    S           2.568e-15  2.566e-15  2.165e-13
      8x6x4 P=2    phi contin. 1.891e-16  1.891e-16  7.907e-15  (single plan: 1.665e-16)
      8x6x4 P=2    phi discr.  2.696e-16  2.391e-16  9.541e-15  (single plan: 2.220e-16)
      6x5x7 P=1    S           2.561e-15  2.168e-15  1.834e-13
      6x5x7 P=1    phi contin. 1.889e-16  2.186e-16  8.040e-15  (single plan: 3.331e-16)
      6x5x7 P=1    phi discr.  1.887e-16  2.201e-16  1.042e-14  (single plan: 2.567e-16)
      16x8x4 P=4   S           4.792e-15  4.676e-15  4.479e-13
      16x8x4 P=4   phi contin. 2.823e-16  3.896e-16  1.288e-14  (single plan: 0.000e+00)
      16x8x4 P=4   phi discr.  3.903e-16  3.868e-16  1.567e-14  (single plan: 0.000e+00)
    """
    Tx, Ty, Tz = T
    nloc, Tyl, Mx = Tz // P, Ty // P, Tx // 2 + 1
    nbytes = nloc * Tyl * Mx * 16
    rho = K.spectral_reference(T, 0, K.SEED["slab_spectral"])[0]
    plans, S, B, phis = [], [], [], {}
    try:
        for r in range(P):
            plan, s, b, bb = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_long()
            assert hip.pinc_hip_fft_slab_create(C.byref(plan), ints(T), nloc, P, r, None) == 0 and plan.value
            plans.append(plan)
            assert hip.pinc_hip_fft_slab_buffers(plan, C.byref(s), C.byref(b), C.byref(bb)) == 0
            assert bb.value == nbytes
            S.append(s.value)
            B.append(b.value)
        src = [Buf(rho[r * nloc:(r + 1) * nloc]) for r in range(P)]
        for discrete in K.SYMBOLS:
            worst = (0.0, 0.0, 0.0)
            for r in range(P):
                assert hip.pinc_hip_fft_slab_set_symbol(plans[r], discrete) == 0
                assert hip.pinc_hip_fft_slab_forward(plans[r], src[r].ptr, None) == 0
                got = np.full((P, nloc, Tyl, Mx), np.nan, np.complex128)
                assert hip.pinc_hip_d2h(got.ctypes.data, S[r], P * nbytes, None) == 0
                want, dS, tolS, _ = K.slab_block_reference(T, P, r)
                devS = float(np.max(np.abs(got - want)))
                worst = max(worst, (devS, dS, tolS))
                assert np.all(np.isfinite(got.view(np.float64)))
                assert devS <= tolS, (r, devS, tolS)
            for r in range(P):
                for q in range(P):
                    assert hip.pinc_hip_d2d(B[q] + r * nbytes, S[r] + q * nbytes, nbytes, None) == 0
            for r in range(P):
                assert hip.pinc_hip_fft_slab_kspace(plans[r], None) == 0
            for r in range(P):
                for q in range(P):
                    assert hip.pinc_hip_d2d(S[r] + q * nbytes, B[q] + r * nbytes, nbytes, None) == 0
            out = [Buf(nans((Tx, Ty, nloc))) for r in range(P)]
            for r in range(P):
                assert hip.pinc_hip_fft_slab_backward(plans[r], out[r].ptr, None) == 0
            phis[discrete] = (np.concatenate([o.get() for o in out], axis=0), worst)
        assert all(s.unchanged() for s in src)
    finally:
        for plan in plans:
            hip.pinc_hip_fft_slab_destroy(plan)
    for discrete in K.SYMBOLS:
        _, ref, d, tol, top = K.spectral_reference(T, discrete, K.SEED["slab_spectral"])
        got, worst = phis[discrete]
        dev = float(np.max(np.abs(got - ref)))
        devs = float(np.max(np.abs(got - solve(hip, T, discrete, rho))))
        print(f"fft_slab {K.shape_id(T)} P={P} discrete={discrete}: S d = {worst[1]:.3e}, deviation = {worst[0]:.3e}, "
              f"tolerance = {worst[2]:.3e}; phi d = {d:.3e}, deviation = {dev:.3e}, from the single plan = {devs:.3e}, "
              f"tolerance = {tol:.3e}, max|phi| = {top:.3e}")
        assert np.all(np.isfinite(got))
        assert dev <= tol
        assert devs <= tol


def test_rejected_creates_leave_no_plan_and_do_no_harm(hip):
    """odd Tx, nd outside 1..3, and for the slab plan Ty % P != 0,
    Tz != nloc P and a rank outside 0..P-1: nonzero, the plan pointer NULL.
    A rejected create does not count as a live plan (the count pairs
    rocfft_setup with rocfft_cleanup), and a valid plan made after it in the
    same process solves within the bound and is destroyed."""
    for nd, T in ((1, (7,)), (2, (5, 4)), (3, (9, 4, 4)), (0, (8,)), (4, (8, 8, 8, 8)), (-1, (8,))):
        plan = C.c_void_p(1)
        assert hip.pinc_hip_fft_create(C.byref(plan), nd, ints(T), None) != 0
        assert plan.value is None
    for T, nloc, P, rank in (((8, 6, 8), 2, 4, 0),    # Ty % P
                             ((8, 8, 8), 3, 4, 0),    # Tz != nloc P
                             ((8, 8, 8), 2, 4, 4),    # rank == P
                             ((8, 8, 8), 2, 4, -1),
                             ((7, 8, 8), 2, 4, 0)):   # odd Tx
        plan = C.c_void_p(1)
        assert hip.pinc_hip_fft_slab_create(C.byref(plan), ints(T), nloc, P, rank, None) != 0
        assert plan.value is None
    T = (8, 5, 7)
    rho, ref, d, tol, top = K.spectral_reference(T, 0)
    got = solve(hip, T, 0, rho)
    assert np.all(np.isfinite(got)) and float(np.max(np.abs(got - ref))) <= tol
