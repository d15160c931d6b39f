"""The binary Coulomb collision rule of include/pinc_hip.h (pinc_hip_coulomb)
restated in numpy: uint64 arithmetic for mix64, the draws u_k as the float64
values the kernel forms, np.longdouble for everything after the draws, one
particle pair at a time.

    key(seed, step, rank, a, b)        pinc_hip_coulomb_key
    cells(pos, T)                      the rule's cell of every particle
    schedule(cell_a, cell_b, key, n_cells)   who collides with whom, in order
    coulomb(pos_a, vel_a, pos_b, vel_b, par, key, T)   one launch
    collide_one(wp, wq, kv, fp, fq, key_pair, j)       one collision

Pairing never reads a velocity, so `schedule` is a function of the positions
and the key alone.  `coulomb` returns a Result (below) with the margin of every
decision: var against 1, g_perp against 0, g against 0, and the smallest gap
between adjacent hash keys of a cell's list.

`relax_f64` is a float64, vectorised twin of the like-particle rule for one
cell (the physics test); tests/test_coulomb_ref_cpu.py holds it to `coulomb`.
"""
from dataclasses import dataclass, field

import numpy as np

from collide_ref import EPS, LD, M64, MAX_SPECIES, mix64, uni
from collide_ref import key as collide_key

TAG = 0x636F756C6F6D62
PI = LD("3.14159265358979323846264338327950288")
C_BOUND = 160.0     # the c of the eps-bound (derived in tests/test_gpu_coulomb_kernel.py)


def key(seed: int, step: int, rank: int, a: int, b: int) -> int:
    k = np.uint64(collide_key(seed, step, rank, a)) ^ np.uint64(TAG) ^ mix64(np.uint64(a * MAX_SPECIES + b))
    return int(mix64(k))


def subkey(k: int, t: int) -> int:
    """key_s (t = 1 for species a, 2 for b) and key_pair (t = 3, 4)"""
    return int(mix64(np.uint64(k) ^ np.uint64(t)))


@dataclass
class Params:
    K: float = 0.0
    fa: float = 0.5                 # mu / m_a
    fb: float = 0.5                 # mu / m_b
    h: tuple = (1.0, 1.0, 1.0)      # stepSize[d] / stepSize[0]


def cells(pos, T):
    """cell = c_0 + T_0 (c_1 + T_1 c_2), c_d = min(max((int)x_d, 1), T_d) - 1"""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    c = [np.clip(np.trunc(pos[:, d]).astype(np.int64), 1, T[d]) - 1 for d in range(3)]
    return c[0] + T[0] * (c[1] + T[1] * c[2])


def ordered(js, key_s):
    """the members js of a cell in the rule's order, and the smallest gap
    between adjacent hash keys (inf for fewer than two members)"""
    js = np.asarray(js, dtype=np.int64)
    hs = mix64(np.uint64(key_s) ^ mix64(js.astype(np.uint64)))
    o = np.lexsort((js, hs))
    hs = hs[o]
    gap = float(np.min((hs[1:] - hs[:-1]).astype(np.float64))) if len(js) > 1 else np.inf
    return js[o], gap


@dataclass
class Collision:
    cell: int
    sp: int      # 0: p is of species a, 1: of species b
    jp: int
    sq: int
    jq: int
    n_low: int
    f: float


def schedule(cell_a, cell_b, k, n_cells):
    """the collisions of a launch, cell by cell, in the order the rule applies
    them inside a cell; cell_b None for a like pair.  Returns (list of
    Collision, smallest hash gap over all lists that were ordered)."""
    like = cell_b is None
    out, gap = [], np.inf
    ka, kb = subkey(k, 1), subkey(k, 2)
    ia = np.argsort(cell_a, kind="stable")
    ea = np.searchsorted(cell_a[ia], np.arange(n_cells + 1))
    if not like:
        ib = np.argsort(cell_b, kind="stable")
        eb = np.searchsorted(cell_b[ib], np.arange(n_cells + 1))
    for c in range(n_cells):
        ja = ia[ea[c]:ea[c + 1]]
        if like:
            N = len(ja)
            if N < 2:
                continue
            L, g_ = ordered(ja, ka)
            gap = min(gap, g_)
            first = 0
            if N & 1:
                for p, q in ((0, 1), (1, 2), (2, 0)):
                    out.append(Collision(c, 0, int(L[p]), 0, int(L[q]), N, 0.5))
                first = 3
            for m in range(first, N, 2):
                out.append(Collision(c, 0, int(L[m]), 0, int(L[m + 1]), N, 1.0))
            continue
        jb = ib[eb[c]:eb[c + 1]]
        if len(ja) == 0 or len(jb) == 0:
            continue
        La, g1 = ordered(ja, ka)
        Lb, g2 = ordered(jb, kb)
        gap = min(gap, g1, g2)
        if len(Lb) > len(La):
            A, B, sA = Lb, La, 1
        else:
            A, B, sA = La, Lb, 0
        Q, R = divmod(len(A), len(B))
        at = 0
        for kk in range(len(B)):
            for _ in range(Q + 1 if kk < R else Q):
                out.append(Collision(c, sA, int(A[at]), 1 - sA, int(B[kk]), len(B), 1.0))
                at += 1
        assert at == len(A)
    return out, gap


def collide_one(wp, wq, kv, fp, fq, key_pair, j):
    """one collision on longdouble w_p, w_q (3,), kv = K nLow f.  Returns
    (w_p', w_q', info) or (None, None, info) if g == 0; info holds g, gp,
    var, the branch and the decision margins"""
    g3 = wp - wq
    gx, gy, gz = g3
    gp = np.sqrt(gx * gx + gy * gy)
    g = np.sqrt((gx * gx + gy * gy) + gz * gz)
    info = {"g": g, "gp": gp, "m_g": float(g) if g > 0 else np.inf, "m_gp": float(gp) if gp > 0 else np.inf,
            "m_var": np.inf, "var": LD(0)}
    if g == 0:
        return None, None, info
    var = LD(kv) / ((g * g) * g)
    info["var"], info["m_var"] = var, float(abs(var - 1))
    u0, u1, u2 = (LD(uni(key_pair, np.uint64((4 * j + t) & M64))) for t in range(3))
    pi = PI
    if var < 1:
        dl = np.sqrt(var) * np.sqrt(-2 * np.log(u0)) * np.cos(2 * pi * u1)
        sinT = 2 * dl / (1 + dl * dl)
        omc = 2 * dl * dl / (1 + dl * dl)
    else:
        c = 1 - 2 * u0
        sinT = np.sqrt((1 - c) * (1 + c))
        omc = 1 - c
    info["small"] = bool(var < 1)
    cp, sp = np.cos(2 * pi * u2), np.sin(2 * pi * u2)
    if gp > 0:
        D = np.array([(gx / gp) * gz * sinT * cp - (gy / gp) * g * sinT * sp - gx * omc,
                      (gy / gp) * gz * sinT * cp + (gx / gp) * g * sinT * sp - gy * omc,
                      -gp * sinT * cp - gz * omc], dtype=LD)
    else:
        D = np.array([gz * sinT * cp, gz * sinT * sp, -gz * omc], dtype=LD)
    return wp + LD(fp) * D, wq - LD(fq) * D, info


@dataclass
class Result:
    vel: list                        # [vel_a, vel_b] longdouble (n, 3); vel_b is vel_a for a like pair
    count: int
    collider: list                   # [mask_a, mask_b]: took part in a collision with g != 0
    bound: list                      # per particle: the eps-bound's scale, see coulomb()
    partners: list                   # per particle: collisions it took part in
    collisions: list                 # the schedule
    margins: dict = field(default_factory=dict)   # smallest var, gp, g margins and hash gap
    branches: dict = field(default_factory=dict)  # collisions per branch


def coulomb(pos_a, vel_a, pos_b, vel_b, par, k, T, err0=None):
    """One launch on species a (and b; pos_b None for a like pair), positions
    and code velocities (n, 3).  Result.bound[s][i] is what the kernel's w may
    differ by from this one's, without the factor eps: for a collision with
    input errors e_p, e_q (0 for a particle's first), both outcomes carry
        A (e_p + e_q) + C_BOUND (|w_p| + |w_q| + g),  A = 2 max(1, g / g_perp)
    (the rotation's frame turns with g / g_perp when its inputs are inexact).
    err0: [per particle of a, of b] input errors in the same unit, where the
    velocities given are themselves only close to those of interest."""
    like = pos_b is None
    h = np.array(par.h, dtype=LD)
    w = [np.asarray(vel_a, dtype=LD).reshape(-1, 3) * h]
    w.append(w[0] if like else np.asarray(vel_b, dtype=LD).reshape(-1, 3) * h)
    n_cells = T[0] * T[1] * T[2]
    ca = cells(pos_a, T)
    cb = None if like else cells(pos_b, T)
    sched, gap = schedule(ca, cb, k, n_cells) if par.K > 0 else ([], np.inf)
    kp = [subkey(k, 3), subkey(k, 4)]
    fr = [par.fa, par.fb]
    col = [np.zeros(len(w[0]), bool), np.zeros(len(w[1]), bool)]
    err = [np.zeros(len(w[0])), np.zeros(len(w[1]))]
    if err0 is not None:
        err = [np.array(err0[0], dtype=float), err[1] if like else np.array(err0[1], dtype=float)]
    part = [np.zeros(len(w[0]), int), np.zeros(len(w[1]), int)]
    if like:
        col[1], err[1], part[1] = col[0], err[0], part[0]
    m = {"var": np.inf, "gp": np.inf, "g": np.inf, "hash_gap": gap}
    br = {"small": 0, "iso": 0, "gp0": 0, "g0": 0}
    count = 0
    for c in sched:
        wp, wq = w[c.sp][c.jp], w[c.sq][c.jq]
        kv = LD(par.K) * c.n_low * LD(c.f)
        np_, nq_, info = collide_one(wp, wq, kv, fr[c.sp], fr[c.sq], kp[c.sp], c.jp)
        m["g"] = min(m["g"], info["m_g"])
        if np_ is None:
            br["g0"] += 1
            continue
        m["var"] = min(m["var"], info["m_var"])
        m["gp"] = min(m["gp"], info["m_gp"])
        br["small" if info["small"] else "iso"] += 1
        br["gp0"] += int(info["gp"] == 0)
        scale = float(np.sum(np.abs(wp)) + np.sum(np.abs(wq)) + info["g"])
        A = 2.0 * max(1.0, float(info["g"] / info["gp"])) if info["gp"] > 0 else 2.0
        e = A * (err[c.sp][c.jp] + err[c.sq][c.jq]) + C_BOUND * scale
        err[c.sp][c.jp] = err[c.sq][c.jq] = e
        w[c.sp][c.jp], w[c.sq][c.jq] = np_, nq_
        col[c.sp][c.jp] = col[c.sq][c.jq] = True
        part[c.sp][c.jp] += 1
        part[c.sq][c.jq] += 1
        count += 1
    return Result([w[0] / h, w[1] / h], count, col, err, part, sched, m, br)


def relax_f64(vel, K, k, steps):
    """The like-particle rule on one cell in float64, vectorised: all N (even)
    particles of species 0 in one cell, h = 1, `steps` launches under the keys
    k[0..steps).  Returns the velocities after every launch, (steps + 1, N, 3)."""
    w = np.array(vel, dtype=np.float64)
    N = len(w)
    assert N % 2 == 0
    out = [w.copy()]
    j = np.arange(N, dtype=np.uint64)
    for s in range(steps):
        L, _ = ordered(np.arange(N), subkey(k[s], 1))
        p, q = L[0::2], L[1::2]
        kp = subkey(k[s], 3)
        g3 = w[p] - w[q]
        gx, gy, gz = g3.T
        gp = np.sqrt(gx * gx + gy * gy)
        g = np.sqrt((gx * gx + gy * gy) + gz * gz)
        var = (K * N) / ((g * g) * g)
        u0, u1, u2 = (uni(kp, np.uint64(4) * j[p] + np.uint64(t)) for t in range(3))
        dl = np.sqrt(var) * np.sqrt(-2 * np.log(u0)) * np.cos(2 * np.pi * u1)
        small = var < 1
        c = 1 - 2 * u0
        sinT = np.where(small, 2 * dl / (1 + dl * dl), np.sqrt((1 - c) * (1 + c)))
        omc = np.where(small, 2 * dl * dl / (1 + dl * dl), 1 - c)
        cp, sp = np.cos(2 * np.pi * u2), np.sin(2 * np.pi * u2)
        assert np.all(gp > 0)
        D = np.stack([(gx / gp) * gz * sinT * cp - (gy / gp) * g * sinT * sp - gx * omc,
                      (gy / gp) * gz * sinT * cp + (gx / gp) * g * sinT * sp - gy * omc,
                      -gp * sinT * cp - gz * omc], 1)
        w[p] += 0.5 * D
        w[q] -= 0.5 * D
        out.append(w.copy())
    return np.array(out)
