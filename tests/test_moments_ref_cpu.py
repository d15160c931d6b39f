"""The velocity moments without a GPU: the numpy reference the GPU tests
compare against (tests/moments_ref.py) checked against hand-made cases and
against push_ref's deposit, pinc_amd.moments.derive, and the build (exports,
header declarations, the kernel's registers).
"""
import numpy as np
import pytest

import moments_ref as MR
import push_ref as R

LD = np.longdouble


@pytest.mark.parametrize("geom", [(8,), (6, 5), (4, 5, 3)])
def test_particle_on_a_node(geom):
    """one particle exactly on a node puts 1, v, v (x) v on that node alone"""
    nd = len(geom)
    node = np.array([[2, 3, 1][:nd]])
    pos = node.astype(np.float64)
    vel = np.array([[0.25, -0.5, 0.125][:nd]])
    ref = MR.moments_reference(pos, vel, geom)
    idx = R._corner_nodes(geom, node, 0)
    v = vel[0]
    want = [1.0] + list(v) + [v[i] * v[j] for i in range(nd) for j in range(i, nd)]
    assert len(want) == MR.n_moments(nd) == ref.M.shape[-1]
    np.testing.assert_array_equal(ref.M[idx][0], np.array(want, dtype=LD))
    rest = ref.M.copy()
    rest[idx] = 0
    assert not rest.any()
    assert ref.k[idx][0] == 1 and ref.k.sum() == 1
    np.testing.assert_array_equal(ref.A, np.abs(ref.M))


@pytest.mark.parametrize("geom", [(16,), (8, 8), (8, 4, 4)])
def test_number_is_conserved_on_a_lattice(geom):
    """sum over all stored nodes of M[0] = the particle count exactly, for
    positions on a 2^-10 lattice (every weight and partial sum is exact)"""
    rng = np.random.default_rng(5)
    n, nd = 3000, len(geom)
    hi = np.array(geom) * 1024
    pos = 0.5 + rng.integers(0, hi, size=(n, nd)) / 1024.0
    vel = rng.uniform(-1, 1, size=(n, nd))
    ref = MR.moments_reference(pos, vel, geom)
    assert ref.M[..., 0].sum() == n
    # the fold moves the ghost planes' share, nothing is lost
    assert MR.fold(ref.M, geom[-1])[..., 0].sum() == n


@pytest.mark.parametrize("geom", [(32,), (8, 8), (8, 4, 4)])
def test_number_equals_push_ref_deposit(geom):
    """M[0] of the moved particles = the deposit of push_reference without a
    kick, when no particle leaves"""
    rng = np.random.default_rng(6)
    nd = len(geom)
    pos = 1.0 + rng.random((2000, nd)) * (np.array(geom) - 1.0)
    vel = rng.uniform(-0.4, 0.4, size=(2000, nd))
    r = R.push_reference(pos, vel, None, geom, R.thresholds(geom), 0, False)
    assert np.all(r.flag == R.centre(nd))
    ref = MR.moments_reference(r.x, vel, geom)
    np.testing.assert_array_equal(ref.M[..., 0], r.rho)
    np.testing.assert_array_equal(ref.k, r.contrib)


def test_accumulation_and_fold_helpers():
    geom = (4, 4, 4)
    rng = np.random.default_rng(7)
    p1, v1 = R.uniform_particles(geom, 100, rng, 0.5)
    p2, v2 = R.uniform_particles(geom, 50, rng, 0.5)
    both = MR.moments_reference(np.concatenate([p1, p2]), np.concatenate([v1, v2]), geom)
    two = MR.add(MR.moments_reference(p1, v1, geom), MR.moments_reference(p2, v2, geom))
    assert np.max(np.abs(both.M - two.M)) <= 4 * np.finfo(LD).eps * np.max(both.A)
    np.testing.assert_array_equal(both.k, two.k)
    f = MR.folded(both, 4)
    assert f.M.shape == (4, 4, 4, 10) and f.k.sum() == both.k.sum()
    MR.check(both.M.astype(np.float64), both, "self")
    bad = both.M.astype(np.float64)
    bad[2, 1, 1, 4] *= 1 + 1e-9
    with pytest.raises(AssertionError):
        MR.check(bad, both, "perturbed")


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_derive_cold_drifting_lattice(nd):
    """a cold lattice drifting at u: derive returns n, u and zero pressure
    and temperature; empty nodes give NaN without a warning"""
    import warnings
    from pinc_amd.moments import derive, n_moments
    geom = (8, 4, 4)[:nd]
    u = np.array([0.25, -0.125, 0.5][:nd])   # dyadic: every product exact
    axes = [np.arange(1, t + 1, dtype=np.float64) for t in geom]
    pos = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, nd)
    pos = np.concatenate([pos, pos])          # two particles on every true node
    vel = np.broadcast_to(u, pos.shape).copy()
    ref = MR.moments_reference(pos, vel, geom)
    M = ref.M.astype(np.float64)
    assert M.shape[-1] == n_moments(nd) == MR.n_moments(nd)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        d = derive(M, 3.0, nd)
    true = (slice(1, geom[-1] + 1),)
    np.testing.assert_array_equal(d.n[true], 2.0)
    np.testing.assert_array_equal(d.u[true], np.broadcast_to(u, d.u[true].shape))
    np.testing.assert_array_equal(d.P[true], 0.0)
    np.testing.assert_array_equal(d.T[true], 0.0)
    assert d.P.shape == M.shape[:-1] + (nd, nd)
    # the ghost planes hold no particle
    assert np.all(d.n[0] == 0) and np.all(np.isnan(d.u[0])) and np.all(np.isnan(d.T[0])) and np.all(np.isnan(d.P[0]))
    with pytest.raises(ValueError):
        derive(M[..., :-1], 1.0, nd)


def test_derive_pressure_of_two_particles():
    from pinc_amd.moments import derive
    # one node, velocities +-a along x: n = 2, u = 0, Pxx = m 2 a^2, T = Pxx / (3 n)
    a, m = 0.5, 4.0
    pos = np.array([[2.0, 2.0, 2.0], [2.0, 2.0, 2.0]])
    vel = np.array([[a, 0.25, 0.0], [-a, 0.25, 0.0]])
    M = MR.moments_reference(pos, vel, (4, 4, 4)).M.astype(np.float64)[2, 1, 1]
    d = derive(M, m, 3)
    assert d.n == 2 and np.all(d.u == [0.0, 0.25, 0.0])
    want = np.zeros((3, 3))
    want[0, 0] = m * 2 * a * a
    np.testing.assert_array_equal(d.P, want)
    assert d.T == want[0, 0] / 6


# ------------------------------------------------------------- the build --
def test_symbols_exported_and_declared(built):
    from pathlib import Path
    from pinc_amd import _lib
    root = Path(__file__).resolve().parent.parent
    hip_names = _lib.header_symbols(root / "include" / "pinc_hip.h")
    host_names = _lib.header_symbols(root / "include" / "pinc.h")
    for n in ("pinc_hip_moments", "pinc_hip_fold_self_values"):
        assert hasattr(_lib.HIP, n), n
        assert n in hip_names, n
    for n in ("puMomentsND1", "pinc_sim_moments", "pinc_sim_moments_shape"):
        assert hasattr(_lib.HOST, n), n
        assert n in host_names, n


def test_moments_kernel_keeps_its_registers(built):
    """every instance: no spilled VGPR, at least two waves per SIMD (two
    workgroups per CU next to their LDS boxes)"""
    from pinc_amd import build
    hits = {k: v for k, v in build.kernel_resources().items() if "k_moments" in k}
    assert len(hits) == 3, sorted(hits)     # 1-D, 2-D, 3-D
    for k, v in hits.items():
        assert v.get("vgpr_spill", -1) == 0, (k, v)
        assert v.get("occupancy", 0) >= 2, (k, v)
        assert 2 * v.get("lds", 1 << 30) <= 160 * 1024, (k, v)
