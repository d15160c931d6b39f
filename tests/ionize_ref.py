"""The ionisation rule of include/pinc_hip.h (pinc_hip_ionize) restated in
numpy: collide_ref's mix64, uni and key for the draws (the float64 values the
kernel forms), np.longdouble for everything after them.

    key(seed, step, rank, s)     pinc_hip_ionize_key
    ionize(vel, par, key)        one launch over a species' velocities

`par` is a Params; `ionize` returns a Result (below): the parents' new
velocities, the children in birth order (ascending parent index: birth k goes
to slot iStop + k of its species) and every decision's margin.
"""
from dataclasses import dataclass, field

import numpy as np

import collide_ref as CR
from collide_ref import EPS, LD, mix64, uni

TAG = 0x696F6E697365


def key(seed: int, step: int, rank: int, s: int) -> int:
    return int(mix64(np.uint64(CR.key(seed, step, rank, s)) ^ np.uint64(TAG)))


@dataclass
class Params:
    nu: float = 0.0                 # ionisation rate per step
    sig: float = 0.0                # n_n sigma per unit of path
    wth: float = 0.0                # threshold speed
    vth: float = 0.0
    drift: tuple = (0.0, 0.0, 0.0)
    h: tuple = (1.0, 1.0, 1.0)      # stepSize[d] / stepSize[0]
    target: int = 1                 # species that receives the ions


@dataclass
class Result:
    vel: np.ndarray                 # (n, nd) longdouble: v' of the parents, the input elsewhere
    hit: np.ndarray                 # (n,) bool: ionises
    parents: np.ndarray             # (births,) indices, ascending: birth k's parent
    electrons: np.ndarray           # (births, nd) longdouble: velocity of the electron of birth k
    ions: np.ndarray                # (births, nd) longdouble
    margin: np.ndarray              # (n,) min(|G - W| / max(G, W), |u0 - P|)
    scale: np.ndarray               # (n,) sum|n_d| + g
    extra: dict = field(default_factory=dict)   # n, G, rem, f, e1, e2 (tests)

    @property
    def births(self):
        return len(self.parents)


def _unit(k, j, ca, nd):
    """step 5's unit vector from the draws at counters 16 j + ca, 16 j + ca + 1"""
    two_pi = 2 * np.arctan(LD(1)) * 4
    ua = uni(k, 16 * j + np.uint64(ca)).astype(LD)
    if nd == 3:
        c = 1 - 2 * ua
        s = np.sqrt((1 - c) * (1 + c))
        phi = two_pi * uni(k, 16 * j + np.uint64(ca + 1)).astype(LD)
        return np.stack([s * np.cos(phi), s * np.sin(phi), c], 1)
    if nd == 2:
        phi = two_pi * ua
        return np.stack([np.cos(phi), np.sin(phi)], 1)
    return np.where(ua < LD(0.5), LD(1), LD(-1))[:, None]


def _neutral(k, j, par, nd):
    """step 1: pinc_hip_collide's neutral from u4..u7 of this stream (16 j + k)"""
    two_pi = 2 * np.arctan(LD(1)) * 4
    u = [uni(k, 16 * j + np.uint64(c)).astype(LD) for c in (4, 5, 6, 7)]
    R = np.sqrt(-2 * np.log(u[0]))
    N = [R * np.cos(two_pi * u[1]), R * np.sin(two_pi * u[1]), np.sqrt(-2 * np.log(u[2])) * np.cos(two_pi * u[3])]
    return np.stack([LD(par.drift[d]) + LD(par.vth) * N[d] for d in range(nd)], 1)


def ionize(vel, par: Params, k: int) -> Result:
    vel = np.asarray(vel, dtype=np.float64)
    n, nd = vel.shape
    j = np.arange(n, dtype=np.uint64)
    h = np.array(par.h[:nd], dtype=LD)
    nn = _neutral(k, j, par, nd)
    w = vel.astype(LD) * h
    G = np.sum((w - nn) ** 2, axis=1)
    g = np.sqrt(G)
    P = -np.expm1(-(LD(par.nu) + LD(par.sig) * g))
    W = LD(par.wth) * LD(par.wth)
    u0 = uni(k, 16 * j).astype(LD)
    hit = (G > W) & (u0 < P)
    rem = np.where(hit, G - W, 0)
    f = uni(k, 16 * j + np.uint64(1)).astype(LD)
    g1, g2 = np.sqrt(f * rem), np.sqrt((1 - f) * rem)
    e1, e2 = _unit(k, j, 2, nd), _unit(k, j, 8, nd)
    out = np.where(hit[:, None], (nn + g1[:, None] * e1) / h, vel.astype(LD))
    parents = np.nonzero(hit)[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        big = np.maximum(G, W)
        mG = np.where(big > 0, np.abs(G - W) / big, 0)
    margin = np.minimum(mG, np.abs(u0 - P))
    return Result(out, hit, parents, ((nn + g2[:, None] * e2) / h)[parents], (nn / h)[parents], margin,
                  np.sum(np.abs(nn), 1) + g, {"n": nn, "G": G, "rem": rem, "f": f, "e1": e1, "e2": e2, "W": W})


def min_margin(res: Result) -> float:
    return float(res.margin.min(initial=np.inf))


def min_rem_share(res: Result) -> float:
    """the smallest (G - W) / G of the ionisers: the conditioning of sqrt(G - W)"""
    G, rem = res.extra["G"][res.hit], res.extra["rem"][res.hit]
    return float((rem / G).min(initial=np.inf))


def bound(res: Result, par: Params, nd: int) -> np.ndarray:
    """(births, nd): 64 eps (sum|n_d| + g) / h_d of each birth's parent"""
    h = np.array(par.h[:nd], dtype=LD)
    return 64 * LD(EPS) * res.scale[res.parents][:, None] / h
