"""Helpers for the phase-space histograms of ``Sim.phase_space``.

``Sim.phase_space(s, axes, bins, lo, hi)`` (puPhaseHist in the C library)
counts species s's particles in ``bins[a]`` equal bins over ``[lo[a], hi[a])``
per axis; the array is ``[bins[1], bins[0]]`` (axis 0 fastest), or
``[bins[0]]`` for one axis.  ``edges`` gives the bin edges per axis and
``density`` the normalised distribution function.
"""
from __future__ import annotations

import numpy as np

# axis codes of the C library (PINC_PS_*, include/pinc_hip.h)
AXES = ("x", "y", "z", "vx", "vy", "vz")


def _per_axis(bins, lo, hi):
    bins, lo, hi = (np.atleast_1d(a) for a in (bins, lo, hi))
    if not (bins.shape == lo.shape == hi.shape) or bins.size not in (1, 2):
        raise ValueError(f"one or two axes: bins {bins}, lo {lo}, hi {hi}")
    return bins.astype(np.int64), lo.astype(np.float64), hi.astype(np.float64)


def edges(bins, lo, hi) -> list[np.ndarray]:
    """per axis the bins[a] + 1 edges lo[a] + k (hi[a] - lo[a]) / bins[a]"""
    bins, lo, hi = _per_axis(bins, lo, hi)
    return [lo[a] + (hi[a] - lo[a]) * np.arange(bins[a] + 1) / bins[a] for a in range(bins.size)]


def density(hist: np.ndarray, bins, lo, hi) -> np.ndarray:
    """counts divided by the bin area (width for one axis) and by their
    total: integrates to 1 over the range (NaN for an empty histogram)"""
    bins, lo, hi = _per_axis(bins, lo, hi)
    hist = np.asarray(hist, dtype=np.float64)
    if hist.shape != tuple(int(b) for b in bins[::-1]):
        raise ValueError(f"density: histogram of shape {hist.shape} for bins {tuple(bins)}")
    area = float(np.prod((hi - lo) / bins))
    with np.errstate(divide="ignore", invalid="ignore"):
        return hist / (area * hist.sum())
