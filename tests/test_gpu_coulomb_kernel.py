"""pinc_hip_coulomb called directly (ctypes, tests/coulomb_abi.py) against the
long-double restatement of its rule, tests/coulomb_ref.py, on a 4 x 3 x 2-cell
geometry (tests/coulomb_cases.py holds the cases).

Checks of every launch (`check` below):
  * the counter is exactly the reference's, and the particles whose velocity
    bits changed are exactly the reference's colliders; all positions, every
    other species and every slot outside the live ranges are bit-identical to
    the input;
  * a collider's w = h v is within eps * Result.bound of the reference's, per
    component.  For a particle's first collision the bound is
        c eps (|w_p| + |w_q| + g),  c = 160,
    |w| the 1-norm.  Derivation, in unit roundoffs u = eps / 2 (the cases' h are
    powers of two, so w = h v and v = w / h are exact): g_d 1; gx gx + gy gy 4,
    g_perp 3, g 3.5; (g g) g 12.5, var 15, sqrt(var) 8.5; sqrt(-2 ln u0) 2 with a
    1-ulp log; cospi 4; dl 17; sinT = 2 dl / (1 + dl dl) 54 and
    omc = 2 dl dl / (1 + dl dl) 72 (the isotropic branch is far below both);
    sinT cphi 59; gx / g_perp 5; the three terms of a component
    (<= g, g, 2 g in size) 67, 69.5 and 74, and their two sums 8 g more: about
    293 u g = 147 eps g for D, times a mass fraction <= 1, plus the update's
    rounding eps |w| / 2: c = 160 covers it.  A particle that collides again
    (a triple's members, an unlike B-member and each of its partners) enters
    with the error e of its earlier outcome, which the rotation passes on
    magnified by at most A = 2 max(1, g / g_perp): the bound grows to
    A (e_p + e_q) + c (|w_p| + |w_q| + g) per further collision
    (coulomb_ref.coulomb), so with the number of partners;
  * per cell, sum m w is conserved within 8 P eps sum m |w| and sum m w^2 within
    4 c P eps sum m w^2, P the most collisions of one particle in the cell:
    m_p (mu / m_p) D = m_q (mu / m_q) D, so momentum moves only by the roundings
    of the two products and the two sums per component and collision (5 u
    (m_p |w_p| + m_q |w_q|) with mu |D| <= 2 mu g; 8 eps allows the 1-norms to
    grow by sqrt(3) along a particle's collisions); the
    energy by D's error (c eps g (|w_p| + |w_q| + g) mu <= 4 c eps
    (m_p w_p^2 + m_q w_q^2) per collision, since mu g^2 <= 2 (m_p w_p^2 + m_q
    w_q^2)).  Masses: m_a : m_b = fb : fa;
  * no decision may differ: the seeds are chosen so that every decision margin
    of every case is above 1e-9 and no two hash keys of a cell are equal
    (tests/test_coulomb_ref_cpu.py::test_reference_margins, in the CPU suite).

A case's later launches are compared with the restatement applied to the state
the kernel left, which is possible because pairing never reads a velocity.  The
final state of a case of several launches is also compared with the free chain
of reference steps (coulomb_cases.case: each from the float64 rounding of the one
before), at the propagated bound: the distance E of the kernel's state from the
chain's enters the next launch as coulomb_ref.coulomb's input error, and the
chain's rounding to float64 adds eps |w| / 2 per launch and component.
"""
import ctypes as C

import numpy as np
import pytest

import coulomb_cases as CC
import coulomb_ref as CR
from coulomb_abi import declare, params_t
from push_abi import SENTINEL, Pop, geom_of

pytestmark = pytest.mark.gpu
LD = np.longdouble
EPS = CR.EPS


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available()
    from pinc_amd import _lib
    h = declare(_lib.HIP)
    assert h.pinc_hip_coulomb_cell_cap() >= 65
    return h


class DevPop:
    """Two species on the device: species 0 at [start, start + n0) of SoA
    arrays, `pad` free slots, species 1 behind them and `pad` more; every slot
    outside the live ranges holds SENTINEL."""

    def __init__(self, sa, sb, start=3, pad=5):
        import torch
        (pa, va), (pb, vb) = sa, sb
        self.n = [len(pa), len(pb)]
        self.first = [start, start + self.n[0] + pad]
        self.cap = self.first[1] + self.n[1] + pad
        host = np.full((6, self.cap), SENTINEL)
        for s, (p, v) in enumerate(((pa, va), (pb, vb))):
            host[0:3, self.first[s]:self.first[s] + self.n[s]] = p.T
            host[3:6, self.first[s]:self.first[s] + self.n[s]] = v.T
        self.host0 = host
        self.t = [torch.from_numpy(host[r].copy()).cuda() for r in range(6)]
        vp3 = C.c_void_p * 3
        self.pop = Pop(vp3(*[t.data_ptr() for t in self.t[:3]]), vp3(*[t.data_ptr() for t in self.t[3:]]), 2, 3,
                       (C.c_long * 9)(self.first[0], self.first[1], self.cap),
                       (C.c_long * 8)(self.first[0] + self.n[0], self.first[1] + self.n[1]))

    def host(self):
        return np.stack([t.cpu().numpy() for t in self.t])

    def vel(self, host, s):
        return np.ascontiguousarray(host[3:6, self.first[s]:self.first[s] + self.n[s]].T)


def launch(hip, dev, a, b, par, key, counts=None, geom=None, work_ints=None):
    import torch
    if counts is None:
        counts = torch.zeros(1, dtype=torch.int64, device="cuda")
    need = hip.pinc_hip_coulomb_work(dev.n[a], 0 if a == b else dev.n[b], CC.NC)
    work = torch.full((need + 16,), -1, dtype=torch.int32, device="cuda")
    rc = hip.pinc_hip_coulomb(dev.pop, a, b, geom or geom_of(CC.T), params_t(par, key), work.data_ptr(),
                              need if work_ints is None else work_ints, counts.data_ptr(), None)
    torch.cuda.synchronize()
    assert np.all(work[need:].cpu().numpy() == -1), "scratch written past pinc_hip_coulomb_work"
    return rc, counts


def check(dev, before, after, pos, a, b, par, res, what):
    """one launch: `before` and `after` are host copies of the device arrays;
    returns the largest error in units of the bound"""
    bits = lambda x: np.ascontiguousarray(x).view(np.uint64)
    np.testing.assert_array_equal(bits(after[0:3]), bits(before[0:3]), err_msg=f"{what}: positions")
    h = np.array(par.h)
    worst = 0.0
    touched = np.zeros(dev.cap, bool)
    for side, s in enumerate((a,) if a == b else (a, b)):
        lo, hi = dev.first[s], dev.first[s] + dev.n[s]
        touched[lo:hi] = True
        v0, v1 = dev.vel(before, s), dev.vel(after, s)
        changed = np.any(bits(v0) != bits(v1), axis=1)
        np.testing.assert_array_equal(changed, res.collider[side], err_msg=f"{what}: colliders of species {s}")
        err = np.abs(v1.astype(LD) * h - res.vel[side] * h).astype(np.float64)
        bound = EPS * res.bound[side][:, None]
        assert np.all(err <= bound), (what, s, float(np.max(err[changed] / bound[changed])))
        if changed.any():
            worst = max(worst, float(np.max(err[changed] / bound[changed])))
    np.testing.assert_array_equal(bits(after[3:6][:, ~touched]), bits(before[3:6][:, ~touched]),
                                  err_msg=f"{what}: slots outside the launch's species")
    # per cell: momentum and energy
    m = [LD(par.fb), LD(par.fa)] if a != b else [LD(1), LD(1)]
    P0, P1, A1, E0, E1, A2 = (np.zeros((CC.NC, n), dtype=LD) for n in (3, 3, 3, 1, 1, 1))
    most = np.zeros(CC.NC)
    for side, s in enumerate((a,) if a == b else (a, b)):
        c = CR.cells(pos[s], CC.T)
        w0, w1 = dev.vel(before, s).astype(LD) * h, dev.vel(after, s).astype(LD) * h
        for arr, val in ((P0, m[side] * w0), (P1, m[side] * w1), (A1, m[side] * np.abs(w0)),
                         (E0, m[side] * np.sum(w0 * w0, 1, keepdims=True)),
                         (E1, m[side] * np.sum(w1 * w1, 1, keepdims=True))):
            np.add.at(arr, c, val)
        np.maximum.at(most, c, res.partners[side])
    A1 = np.sum(A1, 1, keepdims=True)
    assert np.all(np.abs(P1 - P0) <= 8 * most[:, None] * EPS * A1), (what, "momentum")
    assert np.all(np.abs(E1 - E0) <= 4 * CR.C_BOUND * most[:, None] * EPS * E0), (what, "energy")
    return worst


def run_case(hip, name, counts=None, pad=5):
    """every launch of a case; returns (largest error / bound, the Results, the DevPop)"""
    cap = hip.pinc_hip_coulomb_cell_cap()
    sa, sb, launches, cached = CC.case(name, cap)
    dev = DevPop(sa, sb, pad=pad)
    pos = (sa[0], sb[0])
    worst, total, results = 0.0, 0, []
    chain = [sa[1], sb[1]]                                   # the free chain of reference steps
    E = [np.zeros(len(sa[1])), np.zeros(len(sb[1]))]         # |kernel - chain| / eps, in w
    before = dev.host()
    np.testing.assert_array_equal(before, dev.host0)
    for n, (a, b, par, key) in enumerate(launches):
        vel = [dev.vel(before, 0), dev.vel(before, 1)]
        # the first launch's reference is the shared one; a later launch starts from the kernel's state
        res = cached[0] if n == 0 else CC.reference(pos, vel, a, b, par, key)
        for v in ("var", "gp", "g"):
            assert res.margins[v] > 1e-9, (name, n, v, res.margins)
        assert res.margins["hash_gap"] >= 1
        rc, counts = launch(hip, dev, a, b, par, key, counts)
        assert rc == 0, hip.pinc_hip_error_string()
        after = dev.host()
        total += res.count
        assert int(counts.cpu()[0]) == total, (name, n, int(counts.cpu()[0]), total)
        worst = max(worst, check(dev, before, after, pos, a, b, par, res, f"{name}, launch {n}"))
        results.append(res)
        # the same launch with the distance from the chain as input error: its bound is the new distance
        far = CC.reference(pos, vel, a, b, par, key, err0=E)
        chain = CC.advance(chain, a, b, cached[n])
        for side, s in enumerate((a,) if a == b else (a, b)):
            E[s] = far.bound[side] + np.sum(np.abs(chain[s] * np.array(par.h)), axis=1)
        before = after
    if len(launches) > 1:
        for s in range(2):
            h = np.array(launches[-1][2].h)
            err = np.abs(dev.vel(before, s).astype(LD) * h - chain[s].astype(LD) * h).astype(np.float64)
            assert np.all(err <= EPS * E[s][:, None]), (name, "chain", s, float(np.max(err / np.maximum(EPS * E[s][:, None], 1e-300))))
            if len(err):
                print(f"{name}: species {s} ends {float(np.max(err / np.maximum(EPS * E[s][:, None], 1e-300))):.3g} of the chain's bound")
    print(f"{name}: largest error {worst:.3g} of the bound")
    return worst, results, dev


def test_like_pairs_at_every_occupancy(hip):
    """0, 1, 2, 3 (the triple alone), 4, 5, 63, 64, 65, cap - 1, cap, cap + 1
    members in a cell, and more cells than a workgroup's four waves"""
    cap = hip.pinc_hip_coulomb_cell_cap()
    _, (res,), _ = run_case(hip, "occupancy")
    per_cell = np.bincount([c.cell for c in res.collisions], minlength=CC.NC)
    occ = [0, 1, 2, 3, 4, 5, 63, 64, 65, cap - 1, cap, cap + 1]
    assert per_cell[:12].tolist() == [0 if n < 2 else (n // 2 + 2 if n & 1 else n // 2) for n in occ]
    assert res.branches["small"] > 0


def test_one_cell_holds_everything(hip):
    """a list of more than twice the cap, ordered from global memory; every other cell is empty"""
    cap = hip.pinc_hip_coulomb_cell_cap()
    _, (res,), _ = run_case(hip, "one cell")
    assert {c.cell for c in res.collisions} == {7} and res.count == (2 * cap + 45) // 2 + 2


@pytest.mark.parametrize("name", ["unlike", "unlike equal mass", "unlike equal lengths"])
def test_unlike_pairs(hip, name):
    """|A| = |B|; |B| = 1 with |A| = 5; |A| = 7 with |B| = 3 (Q = 2, R = 1);
    species b the longer list; an empty list on either side; lists above the
    cap on one side and on both; 1836 : 1 and equal masses"""
    _, (res,), _ = run_case(hip, name)
    if name != "unlike equal lengths":
        per_cell = np.bincount([c.cell for c in res.collisions], minlength=CC.NC)
        cap = hip.pinc_hip_coulomb_cell_cap()
        assert per_cell[:7].tolist() == [5, 7, 7, 0, 0, cap + 3, cap + 5]
        assert {c.sp for c in res.collisions} == {0, 1}
        assert max(res.partners[1]) >= 5 and max(res.partners[0]) >= 2
    else:
        assert res.count == 5 * CC.NC and {c.sp for c in res.collisions} == {0}


def test_an_empty_species_b(hip):
    _, (res,), dev = run_case(hip, "unlike empty b")
    assert res.count == 0


def test_every_collision_isotropic_and_none_at_K0(hip):
    for name in ("isotropic", "unlike isotropic"):
        _, (res,), _ = run_case(hip, name)
        assert res.branches["small"] == 0 and res.branches["iso"] == res.count > 0
    _, (res,), _ = run_case(hip, "K0")
    assert res.count == 0 and not res.collider[0].any()


def test_second_species_at_an_odd_start(hip):
    """the like pair (1, 1) of a population whose species 1 starts at an odd slot"""
    _, (res,), dev = run_case(hip, "second species", pad=6)
    assert dev.first[1] % 2 == 1 and res.count > 0


def test_anisotropic_cells(hip):
    _, (res,), _ = run_case(hip, "h")
    assert res.count > 0


def test_cell_faces_and_the_clamped_edge(hip):
    cap = hip.pinc_hip_coulomb_cell_cap()
    sa, _, _, _ = CC.case("faces", cap)
    assert np.any(sa[0] == np.floor(sa[0])) and np.any(sa[0] < 1.0) and np.any(sa[0][:, 0] >= CC.T[0] + 1)
    _, (res,), _ = run_case(hip, "faces")
    assert res.count > 0


def test_degenerate_relative_velocities(hip):
    """g_perp == 0 (the pair differs in vz alone) and g == 0 (not counted, not written)"""
    _, results, _ = run_case(hip, "aligned")
    assert sum(r.branches["gp0"] for r in results) > 0 and sum(r.branches["g0"] for r in results) > 0


def test_two_launches_under_two_keys_into_one_counter(hip):
    _, (r0, r1), _ = run_case(hip, "two keys")
    assert [(c.jp, c.jq) for c in r0.collisions] != [(c.jp, c.jq) for c in r1.collisions]


def test_five_successive_launches(hip):
    _, results, _ = run_case(hip, "five")
    assert len(results) == 5 and all(r.count > 0 for r in results)


def test_like_then_unlike_on_one_population(hip):
    """(0, 0), (0, 1), then (1, 1), as the host operator orders them"""
    _, results, _ = run_case(hip, "like then unlike")
    assert all(r.count > 0 for r in results)


def test_key_is_the_restatement_s(hip):
    for args in ((0, 0, 0, 0, 0), (7, 3, 1, 0, 1), (2 ** 63 + 5, 2 ** 40, 5, 2, 7)):
        assert hip.pinc_hip_coulomb_key(*args) == CR.key(*args)


def test_bad_arguments_are_refused(hip):
    """every error of the header returns non-zero and writes nothing"""
    import torch
    cap = hip.pinc_hip_coulomb_cell_cap()
    sa, sb, launches, _ = CC.case("unlike equal lengths", cap)
    _, _, par, key = launches[0]
    dev = DevPop(sa, sb)
    counts = torch.zeros(1, dtype=torch.int64, device="cuda")
    P = CR.Params
    nan, inf = float("nan"), float("inf")
    bad_par = [P(K=-1.0), P(K=nan), P(K=inf), P(K=1.0, fa=0.0), P(K=1.0, fa=1.0), P(K=1.0, fb=0.0), P(K=1.0, fb=1.5),
               P(K=1.0, fa=nan), P(K=1.0, h=(1.0, 0.0, 1.0)), P(K=1.0, h=(1.0, 1.0, -2.0)), P(K=1.0, h=(nan, 1.0, 1.0))]
    for p in bad_par:
        rc, _ = launch(hip, dev, 0, 1, p, key, counts)
        assert rc != 0 and b"coulomb" in hip.pinc_hip_error_string(), p
    for a, b in ((1, 0), (-1, 0), (0, 2), (2, 2)):
        need = hip.pinc_hip_coulomb_work(dev.n[0], dev.n[1], CC.NC)
        work = torch.zeros(need, dtype=torch.int32, device="cuda")
        assert hip.pinc_hip_coulomb(dev.pop, a, b, geom_of(CC.T), params_t(par, key), work.data_ptr(), need,
                                    counts.data_ptr(), None) != 0, (a, b)
    # two dimensions: the population's, the geometry's
    rc, _ = launch(hip, dev, 0, 1, par, key, counts, geom=geom_of(CC.T[:2]))
    assert rc != 0
    flat = Pop.from_buffer_copy(dev.pop)
    flat.nd = 2
    need = hip.pinc_hip_coulomb_work(dev.n[0], dev.n[1], CC.NC)
    work = torch.zeros(need, dtype=torch.int32, device="cuda")
    call = lambda pop, w, n, cnt: hip.pinc_hip_coulomb(pop, 0, 1, geom_of(CC.T), params_t(par, key), w, n, cnt, None)
    assert call(flat, work.data_ptr(), need, counts.data_ptr()) != 0
    # a null array, scratch or counter; scratch one int short
    null = Pop.from_buffer_copy(dev.pop)
    null.v[1] = None
    assert call(null, work.data_ptr(), need, counts.data_ptr()) != 0
    null = Pop.from_buffer_copy(dev.pop)
    null.x[2] = None
    assert call(null, work.data_ptr(), need, counts.data_ptr()) != 0
    assert call(dev.pop, None, need, counts.data_ptr()) != 0
    assert call(dev.pop, work.data_ptr(), need, None) != 0
    assert call(dev.pop, work.data_ptr(), need - 1, counts.data_ptr()) != 0
    torch.cuda.synchronize()
    assert int(counts.cpu()[0]) == 0
    np.testing.assert_array_equal(dev.host(), dev.host0)
    # and the same arguments, whole, are accepted
    assert call(dev.pop, work.data_ptr(), need, counts.data_ptr()) == 0
    torch.cuda.synchronize()
    assert int(counts.cpu()[0]) == 5 * CC.NC
