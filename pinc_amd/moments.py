"""Fluid quantities from the velocity moments of one species.

``Sim.moments(s)`` (puMomentsND1 in the C library) returns per node the
CIC-weighted sums over the species' particles

    M[0]          = sum w            number per node
    M[1 + i]      = sum w v_i        i < nd
    M[1 + nd + k] = sum w v_i v_j    i <= j, row-major upper triangle

in code units (cells, cells per step).  ``derive`` turns them into the
density, the bulk velocity, the pressure tensor and the scalar temperature.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np


def n_moments(nd: int) -> int:
    """NM(nd) = 1 + nd + nd (nd + 1) / 2: 3, 6, 10"""
    return 1 + nd + nd * (nd + 1) // 2


def second_index(nd: int) -> list[tuple[int, int]]:
    """(i, j) of each second moment in storage order"""
    return [(i, j) for i in range(nd) for j in range(i, nd)]


def derive(M: np.ndarray, mass: float, nd: int) -> SimpleNamespace:
    """M: (..., NM(nd)).  Returns
      n  (...)          density, M0
      u  (..., nd)      bulk velocity, M1 / M0
      P  (..., nd, nd)  pressure tensor, m (M2_ij - M1_i M1_j / M0), symmetric
      T  (...)          scalar temperature, tr P / (nd n)
    Nodes without particles (M0 == 0) give NaN in u, P and T, without a
    warning."""
    M = np.asarray(M, dtype=np.float64)
    if M.shape[-1] != n_moments(nd):
        raise ValueError(f"derive: last axis must hold {n_moments(nd)} moments for nd = {nd}, not {M.shape[-1]}")
    n = M[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(n == 0, np.nan, 1.0 / np.where(n == 0, 1.0, n))
        M1 = M[..., 1:1 + nd]
        u = M1 * inv[..., None]
        P = np.empty(M.shape[:-1] + (nd, nd))
        for k, (i, j) in enumerate(second_index(nd)):
            P[..., i, j] = P[..., j, i] = mass * (M[..., 1 + nd + k] - M1[..., i] * M1[..., j] * inv)
        T = np.trace(P, axis1=-2, axis2=-1) * inv / nd
    return SimpleNamespace(n=n, u=u, P=P, T=T)
