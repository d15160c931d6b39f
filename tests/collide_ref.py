"""The collision rule of include/pinc_hip.h (pinc_hip_collide) restated in
numpy: uint64 arithmetic for mix64, the draws u_k as the float64 values the
kernel forms, and np.longdouble for everything after the draws.

    key(seed, step, rank, s)            pinc_hip_collide_key
    collide(vel, par, key, lazy=False)  one launch over a species' velocities

`par` is a Params; `collide` returns a Result (below).  With lazy=True the
neutral's draws are evaluated for the colliders alone where the rule allows
(sig == 0 for both processes): counter-based draws, so the result is the same.
"""
from dataclasses import dataclass, field

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
MAX_SPECIES = 8
M64 = (1 << 64) - 1


def mix64(z):
    """splitmix64's finaliser on uint64 (scalars or arrays), wrapping"""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uni(key, c):
    """the kernel's uni(key, c): float64, the same two roundings"""
    x = mix64(np.uint64(key) ^ mix64(c))
    return ((x >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def key(seed: int, step: int, rank: int, s: int) -> int:
    a = mix64(np.uint64(seed & M64) ^ mix64(np.uint64(step & M64)))
    return int(mix64(a ^ mix64(np.uint64((rank * MAX_SPECIES + s) & M64))))


@dataclass
class Params:
    nu: tuple = (0.0, 0.0)          # elastic, charge exchange: rate per step
    sig: tuple = (0.0, 0.0)         # n_n sigma per unit of path
    b: float = 0.5                  # m_n / (m_s + m_n)
    vth: float = 0.0
    drift: tuple = (0.0, 0.0, 0.0)
    h: tuple = (1.0, 1.0, 1.0)      # stepSize[d] / stepSize[0]


@dataclass
class Result:
    vel: np.ndarray                 # (n, nd) longdouble: v' (the input where nothing collided)
    proc: np.ndarray                # (n,) -1 none, 0 elastic, 1 charge exchange
    m0: np.ndarray                  # |u0 - P|
    m1: np.ndarray                  # |u1 r - r_0| (colliders; inf elsewhere)
    P: np.ndarray
    r: np.ndarray
    scale: np.ndarray               # sum|w_d| + sum|n_d| + g of the colliders (0 elsewhere)
    extra: dict = field(default_factory=dict)   # w, n, g of the colliders (tests)

    @property
    def counts(self):
        return int(np.sum(self.proc == 0)), int(np.sum(self.proc == 1))


def _neutral(k, j, par, nd):
    """n_d of the particles with species-local indices j: (len(j), nd) longdouble"""
    two_pi = 2 * np.arctan(LD(1)) * 4    # (np.pi is the float64 value)
    u4, u5 = uni(k, 8 * j + np.uint64(4)).astype(LD), uni(k, 8 * j + np.uint64(5)).astype(LD)
    R = np.sqrt(-2 * np.log(u4))
    N = [R * np.cos(two_pi * u5)]
    if nd > 1:
        N.append(R * np.sin(two_pi * u5))
    if nd > 2:
        u6, u7 = uni(k, 8 * j + np.uint64(6)).astype(LD), uni(k, 8 * j + np.uint64(7)).astype(LD)
        N.append(np.sqrt(-2 * np.log(u6)) * np.cos(two_pi * u7))
    return np.stack([LD(par.drift[d]) + LD(par.vth) * N[d] for d in range(nd)], 1)


def collide(vel, par: Params, k: int, lazy: bool = False) -> Result:
    vel = np.asarray(vel, dtype=np.float64)
    n, nd = vel.shape
    two_pi = 2 * np.arctan(LD(1)) * 4
    j = np.arange(n, dtype=np.uint64)
    h = np.array(par.h[:nd], dtype=LD)
    nu0, nu1, sg0, sg1 = (LD(x) for x in (*par.nu, *par.sig))
    w = vel.astype(LD) * h
    u0 = uni(k, 8 * j).astype(LD)
    freq_only = par.sig[0] == 0 and par.sig[1] == 0
    if lazy and freq_only:
        # one draw decides; the neutral is drawn for the colliders alone
        Pc = -np.expm1(-(nu0 + nu1))
        sel = np.nonzero(u0 < Pc)[0]
    else:
        sel = np.arange(n)
    nn = np.zeros((n, nd), dtype=LD)
    g = np.zeros(n, dtype=LD)
    if len(sel):
        nn[sel] = _neutral(k, j[sel], par, nd)
        g[sel] = np.sqrt(np.sum((w[sel] - nn[sel]) ** 2, axis=1))
    r0, r1 = nu0 + sg0 * g, nu1 + sg1 * g
    r = r0 + r1
    P = -np.expm1(-r)
    hit = u0 < P
    u1 = uni(k, 8 * j + np.uint64(1)).astype(LD)
    el = hit & (u1 * r < r0)
    cx = hit & ~el
    proc = np.where(el, 0, np.where(cx, 1, -1))
    u2 = uni(k, 8 * j + np.uint64(2)).astype(LD)
    if nd == 3:
        c = 1 - 2 * u2
        s = np.sqrt((1 - c) * (1 + c))
        phi = two_pi * uni(k, 8 * j + np.uint64(3)).astype(LD)
        e = np.stack([s * np.cos(phi), s * np.sin(phi), c], 1)
    elif nd == 2:
        phi = two_pi * u2
        e = np.stack([np.cos(phi), np.sin(phi)], 1)
    else:
        e = np.where(u2 < LD(0.5), LD(1), LD(-1))[:, None]
    b = LD(par.b)
    a = 1 - b
    wel = a * w + b * nn + b * g[:, None] * e
    wout = np.where(el[:, None], wel, np.where(cx[:, None], nn, w))
    out = np.where(hit[:, None], wout / h, vel.astype(LD))
    scale = np.where(hit, np.sum(np.abs(w), 1) + np.sum(np.abs(nn), 1) + g, 0)
    m1 = np.where(hit, np.abs(u1 * r - r0), np.inf)
    return Result(out, proc, np.abs(u0 - P), m1, P, r, scale, {"w": w, "n": nn, "g": g, "hit": hit})


def min_margin(res: Result) -> float:
    """the smallest decision margin of a launch, relative to P and to r"""
    with np.errstate(divide="ignore", invalid="ignore"):
        m0 = np.where(res.P > 0, res.m0 / res.P, np.inf)
        m1 = np.where(res.proc >= 0, res.m1 / res.r, np.inf)
    return float(min(m0.min(initial=np.inf), m1.min(initial=np.inf)))


def check(got_vel, vel_in, res: Result, par: Params, what: str) -> float:
    """got_vel (n, nd) float64 against the reference: non-colliders bit-identical
    to the input, colliders per component within
        |v' - v'_ref| h_d <= 64 eps (sum|w_d| + sum|n_d| + g).
    Returns the largest ratio to that bound."""
    got_vel, vel_in = np.asarray(got_vel), np.asarray(vel_in)
    n, nd = vel_in.shape
    hit = res.proc >= 0
    changed = np.any(got_vel.view(np.uint64) != vel_in.view(np.uint64), axis=1) if n else np.zeros(0, bool)
    # (a collider may by chance keep its bits; a non-collider must)
    assert not np.any(changed & ~hit), f"{what}: {int(np.sum(changed & ~hit))} non-colliders were written"
    if not hit.any():
        return 0.0
    h = np.array(par.h[:nd], dtype=LD)
    err = np.abs(got_vel[hit].astype(LD) - res.vel[hit]) * h
    bound = 64 * LD(EPS) * res.scale[hit]
    ratio = float(np.max(err / bound[:, None]))
    print(f"{what}: {int(hit.sum())} colliders of {n}, largest error / bound = {ratio:.4f}")
    assert ratio <= 1.0, f"{what}: error {ratio:.3f} of the bound"
    return ratio
