"""Plain numpy restatements, and the input builders, of the kernels that the
whole-run tests reached only through energy sums: the immersed objects
(k_objects.hip), order 0 (k_deposit_ngp, k_accel_ngp), the device init
(pinc_hip_init_species: k_lattice_count, k_lattice_write, the counter RNG),
the rescaling chains (k_rho_combine, k_field_chain_all) and k_vel_assert.
No GPU.

Every restatement follows the expression order of include/pinc_hip.h in
float64, so that where the order is fixed the comparison is bit for bit (the
library is built with -ffp-contract=off, and numpy evaluates one operation
per ufunc call: no fused multiply-add on either side).  Sums whose order the
device is free to choose, and the library calls cos, log and sqrt, are
restated in np.longdouble and compared under a bound.

tests/test_glue_ref_cpu.py shows that the inputs built here tell deliberate
mutants of each restatement apart.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

import order2_ref as O
from push_abi import DevSpecies

LD = np.longdouble
EPS = np.finfo(np.float64).eps
CHUNK = 2048          # PINC_CHUNK, and the particles per block of k_accel_ngp
CENTRE3 = 13          # the flag of a particle that stays, 3-D
START = 1001          # iStart of the species under test: odd
N_PART = 2 * CHUNK + 37


def species_1_of_2(pos, vel, start=START, pad=7):
    """pos, vel (n, nd) as species 1 of 2 at an odd iStart; species 0's slots
    and the padding hold push_abi.SENTINEL"""
    sp = DevSpecies(pos, vel, start=start, pad=pad)
    sp.pop.nSpecies = 2
    sp.pop.iStart = (C.c_long * 9)(0, sp.start, sp.cap)
    sp.pop.iStop = (C.c_long * 8)(sp.start, sp.start + sp.n)
    return sp


def trunc_int(x):
    """C's (int)x for doubles well inside the int range: towards zero"""
    return np.trunc(np.asarray(x, dtype=np.float64)).astype(np.int64)


# ---------------------------------------------------------------- objects ---
OBJ_T = (16, 10, 12)
OBJ_BLOCK = ((5, 3, 4), (8, 6, 7))     # id 1: nodes lo <= p < hi, 3 x 3 x 3
OBJ_SINGLE = (10, 7, 9)                # id 2
OBJ_GHOST = (0, 0, 0)                  # id 3: ghost plane 0 of every dimension
OBJ_IDS = 3


def obj_mask():
    """(mask[z][y][x] uint8 over the padded frame, sy, sz, nNodes)"""
    Tx, Ty, Tz = OBJ_T
    m = np.zeros((Tz + 2, Ty + 2, Tx + 2), dtype=np.uint8)
    (x0, y0, z0), (x1, y1, z1) = OBJ_BLOCK
    m[z0:z1, y0:y1, x0:x1] = 1
    m[OBJ_SINGLE[::-1]] = 2
    m[OBJ_GHOST[::-1]] = 3
    sy = Tx + 2
    return m, sy, sy * (Ty + 2), m.size


def obj_ids(pos, mask, sy, sz, n_nodes, to_int=trunc_int):
    """object.c:489-494 as k_obj_flag has it: the id at node (int)x + (int)y sy
    + (int)z sz, 0 where that index is outside [0, nNodes)"""
    c = to_int(pos)
    node = c[:, 0] + c[:, 1] * sy + c[:, 2] * sz
    ok = (node >= 0) & (node < n_nodes)
    return np.where(ok, mask.ravel()[np.where(ok, node, 0)], 0).astype(np.int64)


def obj_flag(pos, mask, sy, sz, n_nodes, first=0, to_int=trunc_int):
    """(flags (n,) uint8, chunkCount per 2048 particles counted from slot
    `first` of the species, counts per id 1..OBJ_IDS)"""
    ids = obj_ids(pos, mask, sy, sz, n_nodes, to_int)
    flags = np.where(ids != 0, 0, CENTRE3).astype(np.uint8)
    n = len(pos)
    chunk = (np.arange(n) + first) // CHUNK - first // CHUNK
    nch = int(chunk[-1]) + 1 if n else 0
    cc = np.bincount(chunk[ids != 0], minlength=nch).astype(np.int32)
    return flags, cc, np.bincount(ids, minlength=OBJ_IDS + 1)[1:].astype(np.int32)


def obj_particles(seed=5):
    """(pos (N_PART, 3), planted) for obj_flag: chunk 0 all inside an object,
    chunk 1 all outside, the last 37 mixed.  `planted` names rows by what
    they are there for."""
    rng = np.random.default_rng(seed)
    mask, sy, sz, nn = obj_mask()
    Tn = np.array(OBJ_T, dtype=np.float64)
    (x0, y0, z0), (x1, y1, z1) = OBJ_BLOCK
    lo, hi = np.array([x0, y0, z0], float), np.array([x1, y1, z1], float)

    def in_block(m):
        return lo + rng.random((m, 3)) * (hi - lo)

    def outside(m):
        out = np.empty((0, 3))
        while len(out) < m:
            p = rng.random((2 * m, 3)) * (Tn + 2)
            out = np.concatenate([out, p[obj_ids(p, mask, sy, sz, nn) == 0]])
        return out[:m]

    single = np.array(OBJ_SINGLE, float)
    on = [np.array([x0, y0 + 0.5, z0 + 0.5]), np.array([x0 + 0.5, y0, z0 + 0.5]), np.array([x0 + 0.5, y0 + 0.5, z0]),
          single.copy()]
    below = []
    for d in range(3):
        b = on[d].copy()
        b[d] = np.nextafter(b[d], 0.0)
        below.append(b)
        b = single + 0.25
        b[d] = np.nextafter(single[d], 0.0)
        below.append(b)
    # (-1, 0): C truncation gives cell 0 (the id-3 node), floor gives -1
    neg = [np.array([-0.5, -0.25, -0.75]), np.array([-0.5, 0.25, 0.5]), np.array([0.5, -0.5, 0.25]),
           np.array([0.25, 0.5, -0.5])]
    # node index < 0, and >= nNodes: kept, nothing read
    far = [np.array([3.5, 2.5, -3.5]), np.array([3.5, 2.5, OBJ_T[2] + 3.5])]
    hit_planted = on + neg
    miss_planted = below + far
    a = np.concatenate([np.array(hit_planted), in_block(CHUNK - len(hit_planted) - 40),
                        single + rng.random((40, 3))])
    b = np.concatenate([np.array(miss_planted), outside(CHUNK - len(miss_planted))])
    a, b = a[rng.permutation(CHUNK)], b[rng.permutation(CHUNK)]
    c = np.concatenate([in_block(9), outside(28)])[rng.permutation(37)]
    pos = np.concatenate([a, b, c])
    assert pos.shape == (N_PART, 3)
    planted = SimpleNamespace(on=np.array(on), below=np.array(below), neg=np.array(neg), far=np.array(far))
    return pos, planted


SURFACE_N = (1, 255, 256, 257, 600)


def surface_case(n, seed=17):
    """inputs of obj_gather / obj_add / obj_correct at n surface nodes:
    distinct slab indices with about one in five -1, a matrix that is clearly
    not symmetric, and a rho whose listed nodes hold at most a quarter of the
    correction's magnitude sum (see obj_correct_ld)"""
    rng = np.random.default_rng([seed, n])
    nodes = 2 * n + 50
    idx = rng.choice(nodes, size=n, replace=False).astype(np.int64)
    drop = rng.random(n) < 0.2
    if n == 1:
        drop[:] = False
    if n >= 255:
        assert 0.1 * n < drop.sum() < 0.3 * n
    idx[drop] = -1
    M = rng.normal(size=(n, n))
    phiS = rng.normal(size=n)
    phiC = 0.37
    grid = rng.normal(size=nodes)
    rho = rng.normal(size=nodes)
    _, S = obj_correct_ld(M, phiS, phiC)
    live = idx >= 0
    rho[idx[live]] = 0.25 * S[live].astype(np.float64) * rng.uniform(-1, 1, size=int(live.sum()))
    return SimpleNamespace(n=n, nodes=nodes, idx=idx, M=M, phiS=phiS, phiC=phiC, grid=grid, rho=rho, v=-1.7)


def obj_gather(grid, idx):
    return np.where(idx >= 0, grid[np.where(idx >= 0, idx, 0)], 0.0)


def obj_add(grid, idx, v):
    out = grid.copy()
    live = idx[idx >= 0]
    out[live] = out[live] + v      # distinct indices
    return out


def obj_correction(M, phiS, phiC):
    """c_i = sum_j M[j, i] (phiC - phiS[j]), accumulated from 0.0 for j = 0..n-1"""
    c = np.zeros(M.shape[1])
    for j in range(M.shape[0]):
        c = c + M[j, :] * (phiC - phiS[j])
    return c


def obj_correct(M, phiS, phiC, idx, rho):
    out = rho.copy()
    c = obj_correction(M, phiS, phiC)
    live = idx >= 0
    out[idx[live]] = out[idx[live]] + c[live]
    return out


def obj_correct_ld(M, phiS, phiC):
    """(the correction, the sum of its terms' magnitudes), long double"""
    t = M.astype(LD) * (LD(phiC) - phiS.astype(LD))[:, None]
    return t.sum(axis=0), np.abs(t).sum(axis=0)


# ---------------------------------------------------------------- order 0 ---
# name: (global T, nloc, off, nranks)
NGP_GEOMS = {"1d": ((8,), 8, 0, 1), "2d": ((8, 6), 6, 0, 1), "3d": ((8, 6, 5), 5, 0, 1),
             "3d-slab": ((8, 6, 10), 5, 5, 2)}
NGP_BIG_T = 1021
NGP_BIG_N = 65536 * 256 + 3


def ngp_local(name):
    """the local true sizes: nloc in the slab (last) dimension"""
    T, nloc, _, _ = NGP_GEOMS[name]
    return tuple(T[:-1]) + (nloc,)


def nearest(pos, to_int=None):
    """(int)(x + 0.5), the sum rounded in float64"""
    pos = np.asarray(pos, dtype=np.float64)
    return trunc_int(pos + 0.5) if to_int is None else to_int(pos)


def ngp_planted(Tl):
    """coordinates per dimension: integers, k + 0.5 exactly (node k + 1; k
    even and odd), its lower neighbour, 0.0, and the lower neighbour of
    T + 1.5 (node T + 1: storage 0 in a periodic dimension, the ghost plane
    nloc + 1 in the slab dimension)"""
    out = []
    for t in Tl:
        v = [0.0, 1.0, float(t), float(t + 1), 0.5, 1.5, 2.5, t + 0.5, np.nextafter(0.5, 0.0), np.nextafter(1.5, 0.0),
             np.nextafter(2.5, 0.0), np.nextafter(t + 0.5, 0.0), np.nextafter(t + 1.5, 0.0)]
        out.append(np.array(v))
    return out


def ngp_particles(name, seed=23):
    """N_PART positions: uniform in [0, T + 1) per dimension ([0, nloc + 1) in
    the slab dimension), the planted coordinates in random rows"""
    Tl = ngp_local(name)
    nd = len(Tl)
    rng = np.random.default_rng([seed, nd, Tl[-1]])
    pos = rng.random((N_PART, nd)) * (np.array(Tl, dtype=np.float64) + 1)
    for d, vals in enumerate(ngp_planted(Tl)):
        rows = rng.choice(N_PART, size=len(vals), replace=False)
        pos[rows, d] = vals
    return pos


def slab_shape(Tl):
    nd = len(Tl)
    return (Tl[nd - 1] + 2,) + tuple(Tl[d] for d in range(nd - 2, -1, -1))


def ngp_offset(j, Tl):
    """flat slab offset of padded node coordinates j (n, nd): x fastest,
    periodic dimensions stored without ghosts at (p - 1) mod T"""
    off = np.zeros(len(j), dtype=np.int64)
    stride = 1
    nd = len(Tl)
    for d in range(nd):
        if d == nd - 1:
            off += j[:, d] * stride
        else:
            off += ((j[:, d] - 1) % Tl[d]) * stride
            stride *= Tl[d]
    return off


def ngp_rho0(Tl, seed=29):
    """integer-valued pre-fill of rho"""
    return np.random.default_rng(seed).integers(-50, 50, size=slab_shape(Tl)).astype(np.float64)


def ngp_deposit(pos, Tl, literal, rho0, to_int=None):
    """rho0 plus one unit (times the literal factor, a small integer) at each
    particle's nearest node: every sum is an integer below 2^53, so exact in
    any order"""
    j = nearest(pos, to_int)
    assert j.min() >= 0 and np.all(j <= np.array(Tl) + 1)
    w = O.literal_factor(j, Tl, literal).astype(np.float64)
    add = np.bincount(ngp_offset(j, Tl), weights=w, minlength=rho0.size)
    return rho0 + add.reshape(rho0.shape)


def ngp_field(Tl, seed=31):
    """E, nd values per slab node (ghost planes included), in [-0.25, 0.25]"""
    return np.random.default_rng(seed).uniform(-0.25, 0.25, size=slab_shape(Tl) + (len(Tl),))


def ngp_accelerate(pos, vel, Es, Tl, to_int=None):
    """(v' = v + E[node] in float64, per block of 2048 particles the long
    double sum of v (v + dv) and of its magnitudes)"""
    nd = len(Tl)
    j = nearest(pos, to_int)
    dv = Es.reshape(-1, nd)[ngp_offset(j, Tl)]
    v1 = vel + dv
    t = vel.astype(LD) * (vel.astype(LD) + dv.astype(LD))
    nb = -(-len(pos) // CHUNK)
    ke = np.array([t[b * CHUNK:(b + 1) * CHUNK].sum() for b in range(nb)], dtype=LD)
    mag = np.array([np.abs(t[b * CHUNK:(b + 1) * CHUNK]).sum() for b in range(nb)], dtype=LD)
    return v1, ke, mag


# ------------------------------------------------------------ device init ---
U64 = np.uint64
INIT_NGLOBAL = (1, 2047, 2048, 2049, 3 * 2048 + 5)
INIT_L = {1: (24,), 2: (12, 10), 3: (8, 6, 10)}     # global true sizes
INIT_SEED = 0x5EEDC0DE12345
INIT_AMP = (0.05, 0.03, 0.04)
INIT_MODE = (1.0, 1.0, 1.0)
INIT_DRIFT, INIT_VTH = 0.125, 0.03


def mix64(z):
    z = np.asarray(z, dtype=U64)
    with np.errstate(over="ignore"):
        z = z + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def uni(seed, c):
    x = mix64(U64(seed) ^ mix64(c))
    return ((x >> U64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def lattice_step(L, n_global):
    return (float(np.prod(L)) / n_global) ** (1.0 / len(L))


def decomposition(L, n_sub):
    """per rank (x fastest): (subdomain, offset) of global sizes L cut n_sub times per dimension"""
    nd = len(L)
    out = []
    for r in range(int(np.prod(n_sub))):
        sub, q = [], r
        for d in range(nd):
            sub.append(q % n_sub[d])
            q //= n_sub[d]
        out.append((tuple(sub), tuple(sub[d] * (L[d] // n_sub[d]) for d in range(nd))))
    return out


def lattice(L, n_global, l, sub, n_sub):
    """the serial loop (pPosLattice): lin = l i, fmod and divide per
    dimension, the owner test (int)(posToSub x) == sub.  Returns (kept
    lattice indices ascending, their global positions (m, nd))"""
    nd = len(L)
    i = np.arange(n_global, dtype=np.int64)
    lin = l * i.astype(np.float64)
    x = np.empty((n_global, nd))
    for d in range(nd):
        x[:, d] = np.fmod(lin, float(L[d]))
        lin = lin / float(L[d])
    ok = np.ones(n_global, dtype=bool)
    for d in range(nd):
        pos_to_sub = 1.0 / (L[d] // n_sub[d])
        ok &= trunc_int(pos_to_sub * x[:, d]) == sub[d]
    return i[ok], x[ok]


def init_species(L, n_global, l, sub, n_sub, off, s, perturb, maxwell, amp=INIT_AMP, mode=INIT_MODE,
                 drift=INIT_DRIFT, vth=INIT_VTH, seed=INIT_SEED, counter=None, two_pi=True):
    """What pinc_hip_init_species writes for one rank, in ascending lattice
    index.  Without perturbation the positions are float64 as the device
    computes them (bit for bit); perturbed positions and Maxwellian
    velocities are long double: cos, log and sqrt of the float64 arguments
    the device forms (theta = ((2 pi mode) p) / L in float64; u1, u2 exact).
    glob: the position in the global frame, in which the perturbation is
    added.  R = sqrt(-2 log u1).  `counter` (the lattice indices by default)
    and `two_pi` exist for the mutants of tests/test_glue_ref_cpu.py."""
    nd = len(L)
    idx, p = lattice(L, n_global, l, sub, n_sub)
    offs = np.array(off, dtype=np.float64)
    if perturb:
        theta = np.stack([2.0 * np.pi * mode[d] * p[:, d] / L[d] for d in range(nd)], 1)
        glob = p.astype(LD) + np.array(amp[:nd], dtype=LD) * np.cos(theta.astype(LD))
        x = glob - offs.astype(LD)
    else:
        glob = p
        x = p - offs
    R = np.zeros((len(idx), nd), dtype=LD)
    if maxwell:
        k = idx if counter is None else counter(idx)
        v = np.empty((len(idx), nd), dtype=LD)
        for d in range(nd):
            c = ((U64(s) << U64(40)) | k.astype(U64)) * U64(3) + U64(d)
            u1, u2 = uni(seed, U64(2) * c), uni(seed, U64(2) * c + U64(1))
            R[:, d] = np.sqrt(LD(-2.0) * np.log(u1.astype(LD)))
            ang = (2.0 * np.pi * u2) if two_pi else u2
            v[:, d] = LD(drift) + LD(vth) * (R[:, d] * np.cos(ang.astype(LD)))
    else:
        v = np.zeros((len(idx), nd))
    return SimpleNamespace(idx=idx, x=x, v=v, glob=glob, R=R)


# ------------------------------------------------------- rescaling chains ---
CHAIN_NS = (1, 2, 3, 8)
CHAIN_N_BIG = 8192 * 256 + 5          # every thread strides; at ns = 3
CHAIN_N_CAP = 8192 * 1024 + 5         # more than 8192 blocks of 4 x 256 elements: the launch cap; at ns = 3
CHAIN_N = (1, 1023)
CHARGES = (-1.3, 0.7, 2.9, -0.45, 1.9, -3.1, 0.11, 5.3)
MASSES = (1.0, 1836.2, 3.7, 0.9, 12.1, 40.3, 2.2, 7.7)
CHAIN_PRE = (1.0, 0.37)
CHAIN_CASES = [(ns, n) for ns in CHAIN_NS for n in CHAIN_N] + [(3, CHAIN_N_BIG), (3, CHAIN_N_CAP)]


def chain_id(c):
    return f"ns{c[0]}-n{c[1]}"


def chain_inputs(ns, n, seed=37):
    rng = np.random.default_rng([seed, ns, n % 1000])
    q = np.array(CHARGES[:ns])
    qm = q / np.array(MASSES[:ns])
    mq = np.array(MASSES[:ns]) / q
    return SimpleNamespace(acc=rng.normal(size=(ns, n)), q=q, qm=qm, mq=mq, E=rng.normal(size=n))


def rho_combine(acc, q):
    """gZero; per species gMul(1/q_s), add, gMul(q_s) (pusher.c:512-572)"""
    r = acc[0].copy()
    for s in range(1, len(q)):
        r = (r * q[s - 1]) * (1.0 / q[s]) + acc[s]
    return r * q[len(q) - 1]


def field_chain_all(E, qm, mq, pre):
    """(ns, n): E as it stands while species s is accelerated (pusher.c:192,212)"""
    v = E * pre
    out = [v * qm[0]]
    for s in range(1, len(qm)):
        v = (v * qm[s - 1]) * mq[s - 1]
        out.append(v * qm[s])
    return np.stack(out)


# ------------------------------------------------------- velocity assert ---
MAX_VEL = 0.8125
VEL_N = 2 * CHUNK + 37
VEL_N_STRIDE = 16384 * 256 + 3        # the grid stride
VEL_N_CAP = 16384 * 2048 + 3          # more than 16384 blocks of 8 x 256 particles: the launch cap


def vel_assert(vel, max_vel, word):
    """pVelAssertMax (population.c:342-365): signed, strict"""
    return word | int(np.any(vel > max_vel))


def vel_cases(nd, n=VEL_N, seed=41):
    """(name, vel (n, nd), offends) with every other component in
    [-maxVel, maxVel): one component planted in turn"""
    rng = np.random.default_rng([seed, nd])
    base = rng.uniform(-MAX_VEL, MAX_VEL, size=(n, nd))
    above = np.nextafter(MAX_VEL, 2.0)
    out = [("quiet", base, False)]
    for val, tag, bad in ((MAX_VEL, "equal", False), (above, "above", True), (-10 * MAX_VEL, "negative", False)):
        for slot, where in ((0, "first"), (n - 1, "last")):
            for d in range(nd):
                v = base.copy()
                v[slot, d] = val
                out.append((f"{tag}-{where}-d{d}", v, bad))
    return out
