"""numpy restatement of pinc_hip_phase_hist's binning rule (include/pinc_hip.h),
bit for bit: the library is built without fused multiply-adds, and counts do
not depend on the order of summation, so every comparison with it is exact.

Per axis a, with c the particle's coordinate:

    t = ((c + shift[a]) - lo[a]) * scale[a]      fp64, in this order
    scale[a] = nbins[a] / (hi[a] - lo[a])        computed once

inside iff t >= 0 and t < nbins[a] on every axis (a NaN is outside); the bin
is int(t); hist[b1, b0] += 1; every other particle counts as outside.
"""
import numpy as np

AXES = ("x", "y", "z", "vx", "vy", "vz")


def scale_of(bins, lo, hi):
    return np.float64(bins) / (np.float64(hi) - np.float64(lo))


def bin_of(c, shift, lo, scale, nbins):
    """(inside, bin) of coordinates c on one axis"""
    c = np.asarray(c, dtype=np.float64)
    t = ((c + np.float64(shift)) - np.float64(lo)) * np.float64(scale)
    with np.errstate(invalid="ignore"):
        inside = (t >= 0.0) & (t < np.float64(nbins))
    return inside, np.where(inside, t, 0.0).astype(np.int64)


def histogram(cols, bins, lo, hi, shift=None):
    """cols: one or two coordinate arrays (axis 0 first).  Returns (hist,
    outside): int64 counts of shape [bins[1], bins[0]] ([1, bins[0]] for one
    axis; reshape as needed) and the number of particles outside."""
    na = len(cols)
    shift = [0.0] * na if shift is None else shift
    inside = np.ones(len(cols[0]), dtype=bool)
    b = []
    for a in range(na):
        ok, k = bin_of(cols[a], shift[a], lo[a], scale_of(bins[a], lo[a], hi[a]), bins[a])
        inside &= ok
        b.append(k)
    nb0, nb1 = int(bins[0]), int(bins[1]) if na > 1 else 1
    flat = b[0][inside] + (b[1][inside] * nb0 if na > 1 else 0)
    hist = np.bincount(flat, minlength=nb0 * nb1).reshape(nb1, nb0)
    return hist, int(len(inside) - inside.sum())


def columns(pos, vel, axes):
    """the coordinate arrays the axis names select from (n, nd) pos and vel"""
    return [(pos if AXES.index(a) < 3 else vel)[:, AXES.index(a) % 3] for a in axes]


def sim_histogram(pos, vel, offset, axes, bins, lo, hi):
    """Sim.phase_space's result for local-frame particles and the rank's
    offset: (float64 hist shaped as Sim returns it, outside)"""
    shift = [float(offset[AXES.index(a)]) if AXES.index(a) < 3 else 0.0 for a in axes]
    h, out = histogram(columns(pos, vel, axes), bins, lo, hi, shift)
    return (h if len(axes) > 1 else h[0]).astype(np.float64), float(out)
