"""tests/phase_ref.py, the numpy restatement of the binning rule, on hand-made
points, and pinc_amd.phase's helpers (no GPU)."""
import numpy as np
import pytest

import phase_ref as PR


def test_lower_edge_is_bin_zero_upper_edge_is_outside():
    lo, hi, nb = -0.5, 0.5, 8
    h, out = PR.histogram([np.array([lo, hi])], [nb], [lo], [hi])
    assert h.shape == (1, nb)
    np.testing.assert_array_equal(h[0], [1, 0, 0, 0, 0, 0, 0, 0])
    assert out == 1


@pytest.mark.parametrize("lo,hi,nb", [(-0.5, 0.5, 8), (0.0, 0.3, 3), (0.5, 16.5, 4096), (-0.95, 0.95, 64)])
def test_just_below_the_upper_edge_goes_where_t_says(lo, hi, nb):
    c = np.nextafter(hi, -np.inf)
    t = ((np.float64(c) + 0.0) - np.float64(lo)) * (np.float64(nb) / (np.float64(hi) - np.float64(lo)))
    h, out = PR.histogram([np.array([c])], [nb], [lo], [hi])
    if t < nb:
        assert out == 0 and h[0, int(t)] == 1 and h.sum() == 1
    else:       # the product rounded up to nbins: outside, by the rule
        assert out == 1 and h.sum() == 0


def test_nan_and_inf_are_outside():
    h, out = PR.histogram([np.array([np.nan, np.inf, -np.inf, 0.0])], [4], [-1.0], [1.0])
    assert out == 3 and h.sum() == 1 and h[0, 2] == 1


def test_negative_zero_t_is_bin_zero():
    h, out = PR.histogram([np.array([-0.0])], [4], [0.0], [1.0])
    assert out == 0 and h[0, 0] == 1


def test_one_axis_and_conservation():
    rng = np.random.default_rng(1)
    v = rng.normal(0, 0.3, 1000)
    h, out = PR.histogram([v], [16], [-0.5], [0.5])
    assert h.shape == (1, 16) and h.sum() + out == 1000 and out > 0
    ref, _ = np.histogram(v, bins=16, range=(-0.5, 0.5))
    # numpy's own histogram closes the last bin on the right and may round an
    # edge differently; away from the edges the two agree
    assert abs(int(h.sum()) - int(ref.sum())) <= 1 and np.abs(h[0] - ref).sum() <= 2


def test_two_axes_layout_shift_and_conservation():
    x = np.array([0.25, 1.75, 1.75, 3.0, 9.0])
    v = np.array([-0.9, 0.1, 0.1, 0.9, 0.0])
    # shift -1 moves x into the global frame [-0.75, 0.75, 0.75, 2, 8]
    h, out = PR.histogram([x, v], [4, 2], [-1.0, -1.0], [3.0, 1.0], shift=[-1.0, 0.0])
    assert h.shape == (2, 4)
    want = np.zeros((2, 4), dtype=np.int64)
    want[0, 0] = 1      # x -0.75, v -0.9
    want[1, 1] = 2      # x 0.75, v 0.1
    want[1, 3] = 1      # x 2, v 0.9
    np.testing.assert_array_equal(h, want)
    assert out == 1 and h.sum() + out == 5


def test_sim_histogram_picks_columns_and_offsets():
    pos = np.array([[1.5, 2.5, 3.5]])
    vel = np.array([[0.1, 0.2, 0.3]])
    h, out = PR.sim_histogram(pos, vel, [-1, -1, 7], ("z", "vy"), (16, 4), (0.0, 0.0), (16.0, 0.4))
    assert h.shape == (4, 16) and h.dtype == np.float64 and out == 0.0
    assert h[2, 10] == 1 and h.sum() == 1          # z = 3.5 + 7, vy = 0.2
    h1, _ = PR.sim_histogram(pos, vel, [-1, -1, 7], ("vx",), (4,), (0.0,), (0.4,))
    assert h1.shape == (4,) and h1[1] == 1


def test_edges_and_density():
    from pinc_amd.phase import density, edges
    e = edges((4, 2), (0.0, -1.0), (2.0, 1.0))
    np.testing.assert_array_equal(e[0], [0.0, 0.5, 1.0, 1.5, 2.0])
    np.testing.assert_array_equal(e[1], [-1.0, 0.0, 1.0])
    h = np.arange(8.0).reshape(2, 4)
    f = density(h, (4, 2), (0.0, -1.0), (2.0, 1.0))
    assert f.shape == (2, 4)
    assert abs(f.sum() * 0.5 * 1.0 - 1.0) < 1e-15
    np.testing.assert_array_equal(f, h / (0.5 * 28.0))
    f1 = density(np.array([1.0, 3.0]), 2, 0.0, 1.0)
    np.testing.assert_array_equal(f1, [0.5, 1.5])
    with pytest.raises(ValueError):
        density(h, (2, 4), (0.0, -1.0), (2.0, 1.0))
