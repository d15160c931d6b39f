"""pinc_hip_phase_hist called directly (ctypes, tests/push_abi.py) against the
numpy restatement of its binning rule, tests/phase_ref.py.  Counts are
integers: every comparison is exact, and sum(hist) + outside == n always.

Cases, the smallest at which each path exists (a chunk is 4096 particles):
  * f(vx), 64 bins, of 5000 particles in random order on 8^3: a small box
    that most of a wave hits at once (the copies of the LDS box), two
    chunks, the second partial;
  * the same as species 1 of 2 at an odd iStart, the other species' slots
    and the tail holding SENTINEL (unaligned first pair; nothing foreign
    counted: SENTINEL would show in `outside`);
  * (x, vx) at 16 * 256 x-bins x 64 on a cell-sorted population on 16x8x8
    and on the unsorted one: more bins than the LDS box has counters.  A
    chunk of the sorted population spans three tiles of 4 cells along x, so
    at 256 bins per cell its box does not fit either and it takes the global
    path as the unsorted one does (counted below, printed);
  * (z, vx) on the cell-sorted population, at as many z-bins as make the
    histogram larger than the LDS box while a chunk inside one layer of
    tiles still fits: boxes at a zero and at a non-zero origin, and one
    chunk on the global path, in one launch (checked here with numpy against
    pinc_hip_phase_lds_bins());
  * a range narrower than the data with particles exactly on lo, on hi, one
    ulp below hi, and in cells 0 and T;
  * the 2-D and 1-D populations, and a position axis >= nDims refused;
  * velocity arrays other than pop.v; two calls into one histogram; n == 0;
    bad bin counts.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import phase_ref as PR
import push_ref as R
from push_abi import SENTINEL, DevSpecies, Pop

pytestmark = pytest.mark.gpu

TW = 4
CHUNK = 4096
VR = (-R.V_MAX, R.V_MAX)


class PhaseT(C.Structure):
    """pinc_phase_t"""
    _fields_ = [("axis", C.c_int * 2), ("nbins", C.c_int * 2), ("shift", C.c_double * 2), ("lo", C.c_double * 2),
                ("scale", C.c_double * 2)]


@pytest.fixture(scope="module")
def hip(built):
    import torch
    assert torch.cuda.is_available()
    from pinc_amd import _lib
    h = _lib.HIP
    vp = C.c_void_p
    h.pinc_hip_phase_hist.argtypes = [Pop, C.c_int, C.POINTER(vp), PhaseT, vp, vp, vp]
    h.pinc_hip_phase_lds_bins.restype = C.c_long
    h.pinc_hip_error_string.restype = C.c_char_p
    return h


@functools.lru_cache(maxsize=None)
def case(name):
    """(geom, pos, vel): made once, shared, never modified"""
    rng = np.random.default_rng({"uniform3d": 21, "unsorted3d": 22, "sorted3d": 22, "2d": 24, "1d": 25}[name])
    if name == "uniform3d":
        geom = (8, 8, 8)
        pos, vel = R.uniform_particles(geom, 5000, rng, R.V_MAX)
    elif name in ("unsorted3d", "sorted3d"):
        geom = (16, 8, 8)
        pos, vel = R.uniform_particles(geom, 20000, rng, R.V_MAX)
        if name == "sorted3d":
            pos, vel = R.cell_sorted(pos, vel, geom, TW)
    elif name == "2d":
        geom = (16, 16)
        pos, vel = R.uniform_particles(geom, 6000, rng, R.V_MAX)
        pos, vel = R.cell_sorted(pos, vel, geom, 8)
    else:
        geom = (64,)
        pos, vel = R.uniform_particles(geom, 5000, rng, R.V_MAX)
    for a in (pos, vel):
        a.setflags(write=False)
    return geom, pos, vel


def spec_of(axes, bins, lo, hi, shift=None):
    na = len(axes)
    sp = PhaseT()
    sp.axis[1], sp.nbins[1], sp.scale[1] = -1, 1, 1.0
    for a in range(na):
        sp.axis[a], sp.nbins[a] = PR.AXES.index(axes[a]), bins[a]
        sp.shift[a] = 0.0 if shift is None else shift[a]
        sp.lo[a] = lo[a]
        sp.scale[a] = PR.scale_of(bins[a], lo[a], hi[a])
    return sp


def run(hip, sp, axes, bins, lo, hi, *, s=0, vs=None, hist=None, shift=None):
    """one pinc_hip_phase_hist of species s of sp.pop into hist (new, zero, if
    None: the bins and, behind them, the outside count); returns (counts
    [nb1, nb0], outside, the device tensor)"""
    import torch
    nb = int(np.prod(bins))
    if hist is None:
        hist = torch.zeros(nb + 1, dtype=torch.int64, device="cuda")
    v = sp.ptrs(vs if vs is not None else sp.vs)
    rc = hip.pinc_hip_phase_hist(sp.pop, s, v, spec_of(axes, bins, lo, hi, shift), hist.data_ptr(),
                                 hist.data_ptr() + 8 * nb, None)
    assert rc == 0, hip.pinc_hip_error_string()
    torch.cuda.synchronize()
    h = hist.cpu().numpy()
    return h[:nb].reshape(bins[1] if len(bins) > 1 else 1, bins[0]), int(h[nb]), hist


def check(got, pos, vel, axes, bins, lo, hi, what, shift=None):
    h, out, _ = got
    ref, ref_out = PR.histogram(PR.columns(pos, vel, axes), bins, lo, hi, shift)
    print(f"{what}: {int(h.sum())} inside, {out} outside of {len(pos)}; reference {int(ref.sum())}, {ref_out}")
    assert int(h.sum()) + out == len(pos), what
    assert out == ref_out, what
    np.testing.assert_array_equal(h, ref, err_msg=what)
    return ref, ref_out


def test_contended_velocity_histogram(hip):
    geom, pos, vel = case("uniform3d")
    a = (("vx",), (64,), VR[:1], VR[1:])
    ref, out = check(run(hip, DevSpecies(pos, vel), *a), pos, vel, *a, "f(vx), random order")
    assert out == 0 and ref.sum() == 5000


def test_second_species_at_an_odd_start(hip):
    geom, pos, vel = case("uniform3d")
    sp = DevSpecies(pos, vel, start=1001, pad=7)
    # species 1 of 2: species 0 is [0, 1001), live, every slot SENTINEL
    sp.pop.nSpecies = 2
    sp.pop.iStart = (C.c_long * 9)(0, sp.start, sp.cap)
    sp.pop.iStop = (C.c_long * 8)(sp.start, sp.start + sp.n)
    a = (("vx",), (64,), VR[:1], VR[1:])
    _, out = check(run(hip, sp, *a, s=1), pos, vel, *a, "f(vx), species 1")
    assert out == 0                               # no SENTINEL slot was read
    assert sp.padding_untouched(sp.xs) and sp.padding_untouched(sp.vs)


def _chunk_boxes(pos, vel, axes, bins, lo, hi):
    """per chunk of CHUNK particles (a species at iStart 0): the origin and
    the area of its bounding box in bin space"""
    cols = PR.columns(pos, vel, axes)
    b = [PR.bin_of(cols[a], 0.0, lo[a], PR.scale_of(bins[a], lo[a], hi[a]), bins[a]) for a in range(len(axes))]
    res = []
    for i in range(0, len(pos), CHUNK):
        ins = np.logical_and.reduce([ok[i:i + CHUNK] for ok, _ in b])
        lo_b = [int(k[i:i + CHUNK][ins].min()) for _, k in b]
        ext = [int(k[i:i + CHUNK][ins].max()) - l + 1 for (_, k), l in zip(b, lo_b)]
        res.append((lo_b, int(np.prod(ext))))
    return res


XV = (("x", "vx"), (16 * 256, 64), (0.5, VR[0]), (16.5, VR[1]))


def zv_spec(cap):
    """(z, vx) over the 8 cells of z at as many bins per cell as let five
    cells of z (a tile's four and a neighbour) by 64 fit an LDS box of cap"""
    return (("z", "vx"), (8 * (cap // (64 * 5)), 64), (0.5, VR[0]), (8.5, VR[1]))


def test_sorted_population_in_a_large_histogram(hip):
    geom, pos, vel = case("sorted3d")
    cap = hip.pinc_hip_phase_lds_bins()
    assert XV[1][0] * XV[1][1] > cap
    boxes = _chunk_boxes(pos, vel, *XV)
    print(f"(x, vx): LDS box {cap}, chunk boxes {[a for _, a in boxes]}")
    ref, out = check(run(hip, DevSpecies(pos, vel), *XV), pos, vel, *XV, "(x, vx), cell-sorted")
    assert out == 0 and ref.sum() == len(pos)


def test_windowed_box_at_a_nonzero_origin(hip):
    geom, pos, vel = case("sorted3d")
    cap = hip.pinc_hip_phase_lds_bins()
    ZV = zv_spec(cap)
    assert ZV[1][0] * ZV[1][1] > cap
    boxes = _chunk_boxes(pos, vel, *ZV)
    print(f"(z, vx): LDS box {cap}, chunk boxes {boxes}")
    # chunks inside one layer of tiles fit the LDS box, some of them above
    # bin 0; the chunk that straddles two layers does not fit (global path)
    assert any(a <= cap and o[0] > 0 for o, a in boxes), boxes
    assert any(a <= cap and o[0] == 0 for o, a in boxes), boxes
    assert any(a > cap for o, a in boxes), boxes
    ref, out = check(run(hip, DevSpecies(pos, vel), *ZV), pos, vel, *ZV, "(z, vx), cell-sorted")
    assert out == 0


@pytest.mark.parametrize("which", ["x-vx", "z-vx"])
def test_unsorted_population_takes_the_global_path(hip, which):
    geom, pos, vel = case("unsorted3d")
    cap = hip.pinc_hip_phase_lds_bins()
    spec = XV if which == "x-vx" else zv_spec(cap)
    assert spec[1][0] * spec[1][1] > cap
    assert all(a > cap for _, a in _chunk_boxes(pos, vel, *spec))
    check(run(hip, DevSpecies(pos, vel, start=3), *spec), pos, vel, *spec, f"{spec[0]}, unsorted")


def test_edges_and_a_range_narrower_than_the_data(hip):
    geom, pos, vel = case("sorted3d")
    lo, hi = 1.0, 16.0
    pe, ve = R.edge_particles(geom)
    mid = [t // 2 + 0.375 for t in geom]
    xs = [lo, hi, np.nextafter(hi, -np.inf), np.nextafter(lo, -np.inf), 0.25, geom[0] + 0.75]
    px = np.array([[x] + mid[1:] for x in xs])
    vx = np.zeros_like(px)
    vx[:, 0] = [-0.5, 0.5, np.nextafter(0.5, -np.inf), 0.0, 0.0, 0.0]
    pos = np.concatenate([pos[:3000], pe, px])
    vel = np.concatenate([vel[:3000], ve, vx])
    cells = pos[:, 0].astype(np.int64)
    assert cells.min() == 0 and cells.max() == geom[0]
    a = (("x", "vx"), (60, 32), (lo, -0.5), (hi, 0.5))
    ref, out = check(run(hip, DevSpecies(pos, vel, start=1), *a), pos, vel, *a, "edges")
    assert out > 0
    assert ref[0, 0] >= 1          # x == lo with vx == lo
    a1 = (("x",), (60,), (lo,), (hi,))
    ref1, out1 = check(run(hip, DevSpecies(pos, vel, start=1), *a1), pos, vel, *a1, "edges, x alone")
    assert out1 > 0 and out1 < out


def test_other_dimensions(hip):
    g2, p2, v2 = case("2d")
    a = (("y", "vx"), (17 * 4, 16), (0.0, VR[0]), (17.0, VR[1]))
    check(run(hip, DevSpecies(p2, v2, start=5), *a), p2, v2, *a, "2-D (y, vx)")
    g1, p1, v1 = case("1d")
    a = (("x", "vx"), (65, 32), (0.0, VR[0]), (65.0, VR[1]))
    check(run(hip, DevSpecies(p1, v1), *a), p1, v1, *a, "1-D (x, vx)")
    # a position (or velocity) axis >= nDims is refused
    import torch
    hist = torch.zeros(65, dtype=torch.int64, device="cuda")
    for (pos, vel), axis in (((p2, v2), "z"), ((p1, v1), "y"), ((p1, v1), "vy")):
        sp = DevSpecies(pos, vel)
        rc = hip.pinc_hip_phase_hist(sp.pop, 0, sp.ptrs(sp.vs), spec_of((axis,), (64,), (0.0,), (1.0,)),
                                     hist.data_ptr(), hist.data_ptr() + 8 * 64, None)
        assert rc != 0 and b"phase_hist" in hip.pinc_hip_error_string()
    torch.cuda.synchronize()
    assert int(hist.sum()) == 0


def test_reads_the_velocity_arrays_it_is_given(hip):
    geom, pos, vel = case("uniform3d")
    sp = DevSpecies(pos, np.full_like(vel, SENTINEL), start=5)
    other = DevSpecies(pos, vel, start=5)      # same ranges: indexed like pop.v
    a = (("vy", "vz"), (16, 16), (VR[0], VR[0]), (VR[1], VR[1]))
    _, out = check(run(hip, sp, *a, vs=other.vs), pos, vel, *a, "separate velocity arrays")
    assert out == 0
    assert np.all(sp.live(sp.vs) == SENTINEL)


def test_accumulates(hip):
    geom, p1, v1 = case("sorted3d")
    _, p2, v2 = case("unsorted3d")
    a = (("x", "vx"), (34, 16), (1.0, -0.5), (16.0, 0.5))
    _, _, hist = run(hip, DevSpecies(p1, v1), *a)
    h, out, _ = run(hip, DevSpecies(p2, v2, start=1), *a, hist=hist)
    r1, o1 = PR.histogram(PR.columns(p1, v1, a[0]), *a[1:])
    r2, o2 = PR.histogram(PR.columns(p2, v2, a[0]), *a[1:])
    np.testing.assert_array_equal(h, r1 + r2)
    assert out == o1 + o2 and o1 > 0 and int(h.sum()) + out == len(p1) + len(p2)


def test_empty_species_and_bad_bin_counts(hip):
    import torch
    geom, pos, vel = case("uniform3d")
    sp = DevSpecies(pos, vel)
    hist = torch.zeros(65, dtype=torch.int64, device="cuda")
    args = (hist.data_ptr(), hist.data_ptr() + 8 * 64, None)
    ok = spec_of(("vx",), (64,), VR[:1], VR[1:])
    sp.pop.iStop = (C.c_long * 8)(sp.start)          # n == 0
    assert hip.pinc_hip_phase_hist(sp.pop, 0, sp.ptrs(sp.vs), ok, *args) == 0
    sp.pop.iStop = (C.c_long * 8)(sp.start + sp.n)
    bad = [spec_of(("vx",), (0,), VR[:1], VR[1:]),
           spec_of(("x", "vx"), (4097, 4096), (0.0, VR[0]), (9.0, VR[1])),     # > 2^24 bins
           spec_of(("x", "vx"), (8, 0), (0.0, VR[0]), (9.0, VR[1]))]
    bad.append(spec_of(("vx",), (64,), VR[:1], VR[1:]))
    bad[-1].axis[0] = 6                                                        # no PINC_PS_*
    for b in bad:
        assert hip.pinc_hip_phase_hist(sp.pop, 0, sp.ptrs(sp.vs), b, *args) != 0
        assert b"phase_hist" in hip.pinc_hip_error_string()
    assert hip.pinc_hip_phase_hist(sp.pop, 9, sp.ptrs(sp.vs), ok, *args) != 0
    torch.cuda.synchronize()
    assert int(hist.sum()) == 0
