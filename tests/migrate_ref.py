"""Plain Python/numpy reference of the migration path of libpinc_hip.so:
the serial back-fill loop of puExtractEmigrantsND (the oracle's restatement
is oracle/orc_pusher.c: emigrate/opu_extractnd) on indices only, the stable
bucketing by direction, the three small copy kernels (pack, import,
import_rec; include/pinc_hip.h) and named flag patterns that assert the
property they are named for.

Nothing here uses the closed form of DESIGN.md section 5: that is what
tests/test_gpu_migrate_kernels.py checks against this loop.
"""
import ctypes as C

import numpy as np

CHUNK = 2048          # PINC_CHUNK
NE_SINK = 27          # PINC_NE_SINK
NE_CODES = 28         # PINC_NE_CODES
REC = 7               # PINC_REC
ERR_CAPACITY = 77     # PINC_ERR_CAPACITY


class ExtractWs(C.Structure):
    """pinc_extract_ws_t (include/pinc_hip.h)."""
    _fields_ = [("chunkOffset", C.c_void_p), ("scanWork", C.c_void_p), ("tail", C.c_void_p), ("holes", C.c_void_p),
                ("order", C.c_void_p), ("blockHist", C.c_void_p), ("scratch", C.c_void_p), ("buf", C.c_void_p),
                ("bufNe", C.c_void_p), ("cap", C.c_long)]


def centre(nd: int) -> int:
    """the flag of a particle that stays"""
    return (3 ** nd - 1) // 2


def codes(nd: int) -> np.ndarray:
    """every flag an emigrant can carry: the directions but the centre, and the object sink"""
    return np.array([c for c in range(3 ** nd) if c != centre(nd)] + [NE_SINK], dtype=np.uint8)


# ------------------------------------------------------------ extraction --
def serial_backfill(flags, centre):
    """The literal loop: walk i from 0 to last; an emigrant in slot i is
    appended to the extraction list, the particle of slot last-1 is copied
    into slot i, last shrinks by one and slot i is tested again.
    Returns (slots, order): slots[k] is the original index of the particle
    that ends in slot k (k < n - E), order the original indices of the
    emigrants in extraction order."""
    flags = np.asarray(flags)
    slot = list(range(len(flags)))
    order = []
    last = len(flags)
    i = 0
    while i < last:
        if flags[slot[i]] != centre:
            order.append(slot[i])
            slot[i] = slot[last - 1]
            last -= 1
        else:
            i += 1
    return np.array(slot[:last], dtype=np.int64), np.array(order, dtype=np.int64)


def serial_backfill_sparse(flags, centre):
    """The same loop, acting only where it can: a back-fill writes the slot
    under test, never one above it, so when the loop reaches slot i that
    slot still holds particle i, and the loop does something only at the
    original emigrant positions below `last`, in ascending order.  There it
    repeats while the particle filled in is itself an emigrant.
    O(n) numpy work and O(E) Python steps."""
    flags = np.asarray(flags)
    n = len(flags)
    emig = flags != centre
    slot = np.arange(n, dtype=np.int64)
    order = []
    last = n
    for i in np.flatnonzero(emig).tolist():
        if i >= last:
            break
        while i < last and emig[slot[i]]:
            order.append(int(slot[i]))
            slot[i] = slot[last - 1]
            last -= 1
    return slot[:last], np.array(order, dtype=np.int64)


def bucket(order, flags):
    """Stable partition of the extraction order by flag value 0..27:
    (indices, their flags, neCount[28]): the content of ws.buf / ws.bufNe,
    direction-major with the extraction order inside each direction (the
    object sink, 27, after every direction)."""
    order = np.asarray(order, dtype=np.int64)
    f = np.asarray(flags)[order].astype(np.int64)
    out = [order[f == ne] for ne in range(NE_CODES)]
    idx = np.concatenate(out) if len(order) else order
    return idx, np.asarray(flags)[idx], np.array([len(o) for o in out], dtype=np.int64)


def chunk_counts(flags, centre):
    """chunkCount[b]: the flags that are not the centre in chunk b"""
    emig = np.asarray(flags) != centre
    nch = -(-len(emig) // CHUNK)
    padded = np.zeros(nch * CHUNK, dtype=np.int32)
    padded[:len(emig)] = emig
    return padded.reshape(nch, CHUNK).sum(1).astype(np.int32)


# ------------------------------------------------------ pack and import ---
def _digits(ne, nd):
    """(len(ne), nd) base-3 digits of the direction, x first"""
    ne = np.asarray(ne).astype(np.int64)
    return np.stack([(ne // 3 ** d) % 3 for d in range(nd)], 1)


def pack_ref(buf, buf_ne, first, n, nd):
    """(n, 7) records of buffer entries [first, first + n): nd positions at
    0.., nd velocities at 3.., zeros for d >= nd, the direction in [6].
    buf: (6, cap) rows x, y, z, vx, vy, vz."""
    rec = np.zeros((n, REC))
    e = slice(first, first + n)
    for d in range(nd):
        rec[:, d] = buf[d, e]
        rec[:, 3 + d] = buf[3 + d, e]
    rec[:, 6] = buf_ne[e]
    return rec


def import_ref(buf, buf_ne, first, n, nd, shift_t, shift_mask):
    """(positions, velocities), (n, nd) each, of buffer entries [first,
    first + n) as the receiver appends them: coordinate d shifted by
    (1 - digit_d(ne)) T_d where shift_mask has bit d set."""
    e = slice(first, first + n)
    dig = _digits(buf_ne[e], nd)
    x = np.stack([buf[d, e] for d in range(nd)], 1).reshape(n, nd)
    v = np.stack([buf[3 + d, e] for d in range(nd)], 1).reshape(n, nd)
    for d in range(nd):
        if (shift_mask >> d) & 1:
            x[:, d] = x[:, d] + ((1 - dig[:, d]) * int(shift_t[d])).astype(np.float64)
    return x, v


def import_rec_ref(rec, nd, shift_t):
    """(positions, velocities) of packed records, shifted in every dimension"""
    rec = np.asarray(rec).reshape(-1, REC)
    dig = _digits(rec[:, 6], nd)
    x = rec[:, :nd] + ((1 - dig) * np.asarray(shift_t[:nd], dtype=np.int64)).astype(np.float64)
    return x, rec[:, 3:3 + nd].copy()


# -------------------------------------------------------- flag patterns ---
RANDOM_P = (0.01, 0.5, 0.99)
PATTERN_NAMES = ("none", "all", "first_only", "last_only", "tail_block", "head_block", "emigrant_at_m",
                 "survivor_at_m", "alternating") + tuple(f"random_{p}" for p in RANDOM_P) + \
                ("quiet_head", "m_on_chunk_edge")


def _emigrant_mask(name, n, rng):
    """the emigrant positions of a named pattern, or None where its property cannot hold at n"""
    mask = np.zeros(n, dtype=bool)

    def scatter(count, among):
        mask[rng.choice(among, size=count, replace=False)] = True

    if name == "none":
        pass
    elif name == "all":
        mask[:] = True
    elif name == "first_only":
        mask[0] = True
    elif name == "last_only":
        mask[n - 1] = True
    elif name == "tail_block":
        mask[n - max(1, n // 3):] = True
    elif name == "head_block":
        if n < 3:
            return None
        mask[:max(1, n // 3)] = True
    elif name in ("emigrant_at_m", "survivor_at_m"):
        if n < 3:
            return None
        E = max(2, n // 4)
        m = n - E
        first = int(rng.integers(0, m))                       # a hole before m
        if name == "emigrant_at_m":
            fixed = [first, m]
        else:
            fixed = [first, int(rng.integers(m + 1, n))]      # and an emigrant behind m
        mask[fixed] = True
        scatter(E - 2, np.setdiff1d(np.arange(n), fixed + [m]))
    elif name == "alternating":
        if n < 2:
            return None
        mask[0::2] = True
    elif name.startswith("random_"):
        mask[:] = rng.random(n) < float(name[len("random_"):])
    elif name == "quiet_head":
        if n <= 2 * CHUNK:
            return None
        base = (n - 1) // CHUNK * CHUNK                       # the last chunk
        scatter((n - base + 1) // 2, np.arange(base, n))
    elif name == "m_on_chunk_edge":
        if n % CHUNK or n < 2 * CHUNK:
            return None
        scatter(n // CHUNK // 2 * CHUNK, np.arange(n))
    else:
        raise KeyError(name)
    return mask


def _assert_property(name, mask):
    n = len(mask)
    E = int(mask.sum())
    m = n - E
    if name == "none":
        assert E == 0
    elif name == "all":
        assert E == n and m == 0
    elif name == "first_only":
        assert E == 1 and mask[0]
    elif name == "last_only":
        assert E == 1 and mask[n - 1]
    elif name == "tail_block":
        assert E >= 1 and mask[n - E:].all() and not mask[:m].any() and mask[m]
    elif name == "head_block":
        assert 1 <= E < n / 2 and mask[:E].all() and not mask[m:].any()
    elif name == "emigrant_at_m":
        assert mask[m] and mask[:m].any()
    elif name == "survivor_at_m":
        assert not mask[m] and mask[:m].any() and mask[m + 1:].any()
    elif name == "alternating":
        assert np.array_equal(mask, np.arange(n) % 2 == 0)
    elif name.startswith("random_"):
        p = float(name[len("random_"):])
        assert p in RANDOM_P and abs(E - n * p) <= 6 * np.sqrt(n * p * (1 - p)) + 1
    elif name == "quiet_head":
        base = (n - 1) // CHUNK * CHUNK
        assert n > 2 * CHUNK and E >= 1 and not mask[:base].any()
        counts = chunk_counts(mask.astype(np.uint8), 0)
        assert any(counts[b] == 0 and (b + 1) * CHUNK <= m for b in range(len(counts)))
    elif name == "m_on_chunk_edge":
        assert n % CHUNK == 0 and n >= 2 * CHUNK and 0 < m < n and m % CHUNK == 0


def pattern(name, n, centre, codes, rng):
    """The flags of pattern `name` at n particles (its property asserted),
    or None where the property cannot hold at that n.  Emigrant flags are
    drawn uniformly from `codes`, so equal directions interleave."""
    mask = _emigrant_mask(name, n, rng)
    if mask is None:
        return None
    flags = np.full(n, centre, dtype=np.uint8)
    flags[mask] = rng.choice(np.asarray(codes, dtype=np.uint8), size=int(mask.sum()))
    assert centre not in codes and np.array_equal(flags != centre, mask)
    _assert_property(name, mask)
    return flags


def pattern_names(n):
    """the names whose property can hold at n"""
    rng = np.random.default_rng(0)
    return [name for name in PATTERN_NAMES if _emigrant_mask(name, n, rng) is not None]


def patterns(n, centre, codes, rng):
    """(name, flags) of every named pattern that exists at n"""
    for name in PATTERN_NAMES:
        flags = pattern(name, n, centre, codes, rng)
        if flags is not None:
            yield name, flags
