"""pinc_hip_init_species (k_lattice_count, k_lattice_write, the counter RNG)
called through the C ABI, against the host's serial loop restated in
tests/glue_ref.py: lin = l i, fmod and divide per dimension, the owner test
(int)(posToSub x), the cosine perturbation, the Maxwellian velocities; the
mixer and uni in integer numpy.

Global grids 24, 12 x 10 and 8 x 6 x 10; nGlobal in {1, 2047, 2048, 2049,
3 * 2048 + 5}; one rank, two slabs along the last dimension, and 2 x 1 x 2 in
3-D, each rank called on its own.  The species is species 1 of 2 at an odd
iStart; its arrays are pre-filled, and every slot outside [iStart, iStart +
count) comes back unchanged.

Without perturbation the positions are bit for bit, compared as arrays in
ascending lattice index (fmod is exact and every other operation is one IEEE
operation in a fixed order), and without Maxwellian velocities v is +0.0.

With them, the device's cos, log and sqrt need not match the host's, so the
comparison is with the long-double restatement:

    |dx| <= 16 eps amp + eps |x|          |dv| <= 32 eps vth R + eps |v|

R = sqrt(-2 log u1).  The ROCm install carries no statement of ulp bounds for
the double-precision device functions, so the constants allow for: a few
ulp per library call, the three roundings of theta = 2 pi mode p / L
(3/2 eps of at most 2 pi at mode 1: 9.5 eps), the rounding of 2 pi u2 (pi
eps), the products.  |x| is the position in the frame in which the
perturbation is added, the global one (pinc_pop.c: pToGlobalFrame, perturb,
pToLocalFrame): the add p + amp cos rounds there, and the shift to the local
frame by an integer offset is then exact (local + offset is compared, in long
double).  On a rank whose offset is 0 the two frames coincide.  Every mutant
of tests/test_glue_ref_cpu.py is more than 1e6 times outside these bounds.

Device against device, bit for bit: the ranks' particles, shifted back by
their offsets and put in lattice order by a stable sort, are the one-rank
output, positions (perturbed) and Maxwellian velocities alike.
"""
import ctypes as C

import numpy as np
import pytest

import glue_ref as G
from gpu_buf import same_bits
from push_abi import SENTINEL, Geom, Pop

pytestmark = pytest.mark.gpu

LD = G.LD
PAD = 9
DECS = {1: [(1,), (2,)], 2: [(1, 1), (1, 2)], 3: [(1, 1, 1), (1, 1, 2), (2, 1, 2)]}
CASES = [(nd, n, ns) for nd in (1, 2, 3) for n in G.INIT_NGLOBAL for ns in DECS[nd]]
case_id = lambda c: f"{c[0]}d-{c[1]}-" + "x".join(map(str, c[2]))


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available()
    from pinc_amd import _lib
    h = _lib.HIP
    vp, ci, ip, dp = C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)
    h.pinc_hip_init_species.argtypes = [Pop, ci, Geom, C.c_long, C.c_double, ip, ip, ip, dp, dp, ci, ci, C.c_double,
                                        C.c_double, C.c_ulonglong, C.POINTER(C.c_long), vp]
    return h


def run(hip, L, n_global, sub, n_sub, off, perturb, maxwell, cap):
    """(rc, nOut, x (cap + PAD + START, nd), v): species 1 of 2 with `cap`
    slots at START, every slot pre-filled with the sentinel"""
    import torch
    nd = len(L)
    total = G.START + cap + PAD
    xs = [torch.full((total,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(nd)]
    vs = [torch.full((total,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(nd)]
    ptrs = lambda ts: (C.c_void_p * 3)(*([t.data_ptr() for t in ts] + [None] * (3 - nd)))
    pop = Pop(ptrs(xs), ptrs(vs), 2, nd, (C.c_long * 9)(0, G.START, G.START + cap), (C.c_long * 8)(G.START, G.START))
    g = Geom(nd, (C.c_int * 3)(*(list(L) + [1] * (3 - nd))), L[-1] // n_sub[-1], off[-1], int(np.prod(n_sub)), 0)
    ints = lambda v: (C.c_int * nd)(*v)
    dbl = lambda v: (C.c_double * nd)(*v[:nd])
    n_out = C.c_long(-1)
    rc = hip.pinc_hip_init_species(pop, 1, g, n_global, G.lattice_step(L, n_global) if n_global else 1.0, ints(sub),
                                   ints(n_sub), ints(off), dbl(G.INIT_AMP), dbl(G.INIT_MODE), perturb, maxwell,
                                   G.INIT_DRIFT, G.INIT_VTH, G.INIT_SEED, C.byref(n_out), None)
    torch.cuda.synchronize()
    return rc, n_out.value, np.stack([t.cpu().numpy() for t in xs], 1), np.stack([t.cpu().numpy() for t in vs], 1)


def live(a, m):
    return a[G.START:G.START + m]


def rest_untouched(a, m):
    return bool(np.all(a[:G.START] == SENTINEL) and np.all(a[G.START + m:] == SENTINEL))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_lattice_positions_bit_for_bit(hip, case):
    """no perturbation, no Maxwellian: the count, the positions as arrays in
    ascending lattice index (a stable compaction), +0.0 velocities, nothing
    else written; each rank of the decomposition on its own"""
    nd, n, n_sub = case
    L = G.INIT_L[nd]
    l = G.lattice_step(L, n)
    total = 0
    for sub, off in G.decomposition(L, n_sub):
        want = G.init_species(L, n, l, sub, n_sub, off, 1, 0, 0)
        m = len(want.idx)
        rc, n_out, x, v = run(hip, L, n, sub, n_sub, off, 0, 0, cap=m)        # exactly the capacity needed
        assert rc == 0 and n_out == m
        np.testing.assert_array_equal(live(x, m), want.x)
        assert same_bits(live(x, m), want.x)
        assert same_bits(live(v, m), np.zeros((m, nd)))
        assert rest_untouched(x, m) and rest_untouched(v, m)
        total += m
    assert total == n


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_perturbed_positions_and_maxwellian_velocities(hip, case):
    """|dx| <= 16 eps amp + eps |x| (x in the frame of the perturbation) and
    |dv| <= 32 eps vth R + eps |v| against the long-double restatement; the
    ranks' outputs, shifted back and put in lattice order, are the one-rank
    output bit for bit.

    Measured on an MI355X over all cases: the largest dx is 0.475 of its
    bound, the largest dv 0.380 of its."""
    nd, n, n_sub = case
    L = G.INIT_L[nd]
    l = G.lattice_step(L, n)
    parts = []
    for sub, off in G.decomposition(L, n_sub):
        want = G.init_species(L, n, l, sub, n_sub, off, 1, 1, 1)
        m = len(want.idx)
        rc, n_out, x, v = run(hip, L, n, sub, n_sub, off, 1, 1, cap=m + 3)
        assert rc == 0 and n_out == m
        assert rest_untouched(x, m) and rest_untouched(v, m)
        glob = live(x, m).astype(LD) + np.array(off, dtype=LD)
        dx = np.abs(glob - want.glob)
        xlim = 16 * G.EPS * np.array(G.INIT_AMP[:nd], dtype=LD) + G.EPS * np.abs(want.glob)
        dv = np.abs(live(v, m).astype(LD) - want.v)
        vlim = 32 * G.EPS * G.INIT_VTH * want.R + G.EPS * np.abs(want.v)
        if m:
            print(f"{case_id(case)} rank {sub}: dx / bound {float(np.max(dx / xlim)):.3f}, "
                  f"dv / bound {float(np.max(dv / vlim)):.3f}")
        assert np.all(dx <= xlim)
        assert np.all(dv <= vlim)
        parts.append((want.idx, live(x, m) + np.array(off, dtype=np.float64), live(v, m)))
    if len(parts) > 1:
        one = G.init_species(L, n, l, (0,) * nd, (1,) * nd, (0,) * nd, 1, 1, 1)
        rc, n_out, x, v = run(hip, L, n, (0,) * nd, (1,) * nd, (0,) * nd, 1, 1, cap=n)
        assert rc == 0 and n_out == n and np.array_equal(one.idx, np.arange(n))
        order = np.argsort(np.concatenate([p[0] for p in parts]), kind="stable")
        assert same_bits(np.concatenate([p[1] for p in parts])[order], live(x, n))
        assert same_bits(np.concatenate([p[2] for p in parts])[order], live(v, n))


def test_capacity_too_small(hip):
    nd, n = 3, 2049
    L = G.INIT_L[nd]
    rc, n_out, x, v = run(hip, L, n, (0, 0, 0), (1, 1, 1), (0, 0, 0), 1, 1, cap=n - 1)
    assert rc != 0
    assert b"capacity" in hip.pinc_hip_error_string()
    assert rest_untouched(x, 0) and rest_untouched(v, 0)


def test_no_particles(hip):
    rc, n_out, x, v = run(hip, G.INIT_L[2], 0, (0, 0), (1, 1), (0, 0), 1, 1, cap=5)
    assert rc == 0 and n_out == 0
    assert rest_untouched(x, 0) and rest_untouched(v, 0)
