#!/usr/bin/env python3
"""Time pinc_hip_coulomb against the fused push of the same population.

Two species of a warm plasma (v_th = 0.05 cells/step per component) on a
size^3 grid, ppc particles per cell and species, each sorted by tile
(pinc_hip_sort_tiles, tile width 4).  Two states, each in a process of its own
under a time limit (a state that fails or runs out of time ends the probe):
    fresh     right after the tile sort
    decayed   after `--decay` fused pushes (kick with E = 0, drift, periodic
              wrap in place, deposit) without a sort
In each: the like launch (0, 0), the unlike launch (0, 1) (K = 1e-6, equal
masses for the like pair, 1 : 1836 for the unlike one) and the fused push of
species 0 (pinc_hip_push, kick = 1 with E = 0, in place), as the median of
`--launches` launches after `--warmup` warm-ups on the library's events; every
collision launch gets a new key.  The push moves the particles, so its launches
come last.

Bytes of a collision launch by the rule's own count, per particle of each
species of the launch: 24 B positions read, the cell 4 B written and 4 B read,
the index 4 B written and 4 B read, and per collider 24 B of velocity gathered
and 24 B scattered; 12 B per cell and species for counts, cursors and offsets.
The push: 96 B per particle + 32 B per node.

    python tools/coulomb_probe.py --out profiles/coulomb.json
"""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

PEAK_BW = 8.0e12        # B/s
COPY_CEILING = 6.35e12  # B/s, DESIGN.md (profiles/r05e_copy_ceiling.json)


def child(args) -> int:
    import numpy as np
    import torch
    import push_ref as R
    from coulomb_abi import CoulombT, declare
    from push_abi import Geom, Pop, PushArgs, geom_of
    from pinc_amd import _lib
    hip = declare(_lib.HIP)
    vp = C.c_void_p
    hip.pinc_hip_push.argtypes = [Pop, C.c_int, Geom, C.POINTER(PushArgs), C.POINTER(C.c_int), vp]
    hip.pinc_hip_push_chunk.restype = C.c_long
    hip.pinc_hip_sort_tiles.argtypes = [Pop, Pop, C.c_int, Geom, C.c_int, vp, C.c_long, C.POINTER(C.c_long), vp]
    hip.pinc_hip_tile_keys.argtypes = [Geom, C.c_int]
    hip.pinc_hip_tile_keys.restype = C.c_long
    hip.pinc_hip_event_create.argtypes = [C.POINTER(vp)]
    hip.pinc_hip_event_record.argtypes = [vp, vp]
    hip.pinc_hip_event_sync.argtypes = [vp]
    hip.pinc_hip_event_elapsed.argtypes = [C.POINTER(C.c_float), vp, vp]

    S, tw = args.size, 4
    T = (S, S, S)
    n = S ** 3 * args.ppc
    geom = geom_of(T)
    gen = torch.Generator(device="cuda").manual_seed(1)
    f64 = dict(dtype=torch.float64, device="cuda")
    # both species in one set of arrays: [0, n) and [n, 2 n)
    xs = [torch.clamp(1.0 + S * torch.rand(2 * n, generator=gen, **f64), max=S + 1 - 1e-9) for _ in range(3)]
    vs = [0.05 * torch.randn(2 * n, generator=gen, **f64) for _ in range(3)]

    def pop_of(x, v):
        return Pop((vp * 3)(*[t.data_ptr() for t in x]), (vp * 3)(*[t.data_ptr() for t in v]), 2, 3,
                   (C.c_long * 9)(0, n, 2 * n), (C.c_long * 8)(n, 2 * n))

    ox, ov = [torch.empty_like(t) for t in xs], [torch.empty_like(t) for t in vs]
    K = hip.pinc_hip_tile_keys(geom, tw)
    cap = 2 * (K + 1) + 2 * (K // 4096 + 1) + 1
    work = torch.zeros(cap, dtype=torch.int32, device="cuda")
    nk = C.c_long()
    for s in range(2):
        rc = hip.pinc_hip_sort_tiles(pop_of(xs, vs), pop_of(ox, ov), s, geom, tw, work.data_ptr(), cap, C.byref(nk), None)
        assert rc == 0, hip.pinc_hip_error_string()
    torch.cuda.synchronize()
    del xs, vs, work
    xs, vs = ox, ov
    pop = pop_of(xs, vs)

    # the fused push of species s, in place, E = 0
    chunk = hip.pinc_hip_push_chunk()
    nblk, nch = (n + chunk - 1) // chunk, (n + R.PINC_CHUNK - 1) // R.PINC_CHUNK
    slab = int(np.prod(R.slab_shape(T)))
    Es = torch.zeros(3 * slab, **f64)
    rho = torch.zeros(slab, **f64)
    flags = torch.full((2 * n,), R.centre(3), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(2 * nch + 4, dtype=torch.int32, device="cuda")
    err = torch.zeros(16, dtype=torch.int32, device="cuda")
    ke = torch.zeros(2 * nblk + 4, **f64)
    thr = (C.c_double * 9)(*R.thresholds(T))
    a = PushArgs()
    a.xout, a.vout = pop.x, pop.v
    a.kick, a.Es, a.rhoS, a.thr = 1, Es.data_ptr(), rho.data_ptr(), C.cast(thr, vp)
    a.flags, a.chunkCount, a.maxVel, a.errFlag = flags.data_ptr(), cnt.data_ptr(), 1.0, err.data_ptr()
    a.wrapMask, a.kePartial, a.tileWidth, a.flagsSparse = 7, ke.data_ptr(), tw, 0
    nb = C.c_int()

    def push(s):
        cnt.zero_()
        return hip.pinc_hip_push(pop, s, geom, C.byref(a), C.byref(nb), None)

    if args.child == "decayed":
        for _ in range(args.decay):
            for s in range(2):
                assert push(s) == 0, hip.pinc_hip_error_string()
        torch.cuda.synchronize()
        assert int(err[0]) == 0

    ev = [vp(), vp()]
    for e in ev:
        assert hip.pinc_hip_event_create(C.byref(e)) == 0

    def timed(launch):
        ms = []
        for i in range(args.warmup + args.launches):
            hip.pinc_hip_event_record(ev[0], None)
            assert launch() == 0, hip.pinc_hip_error_string()
            hip.pinc_hip_event_record(ev[1], None)
            hip.pinc_hip_event_sync(ev[1])
            t = C.c_float()
            hip.pinc_hip_event_elapsed(C.byref(t), ev[0], ev[1])
            if i >= args.warmup:
                ms.append(t.value)
        return statistics.median(ms), ms

    nc = S ** 3
    counts = torch.zeros(1, dtype=torch.int64, device="cuda")
    need = hip.pinc_hip_coulomb_work(n, n, nc)
    cwork = torch.zeros(need, dtype=torch.int32, device="cuda")
    step = [0]

    def coulomb(sa, sb, fa, fb):
        def go():
            par = CoulombT(1e-6, fa, fb, (C.c_double * 3)(1, 1, 1), hip.pinc_hip_coulomb_key(9, step[0], 0, sa, sb))
            step[0] += 1
            return hip.pinc_hip_coulomb(pop, sa, sb, geom, par, cwork.data_ptr(), need, counts.data_ptr(), None)
        return go

    rows = []
    for name, sa, sb, fa, fb in (("like (0, 0)", 0, 0, 0.5, 0.5), ("unlike (0, 1)", 0, 1, 1836.0 / 1837.0, 1.0 / 1837.0)):
        counts.zero_()
        ms, every = timed(coulomb(sa, sb, fa, fb))
        torch.cuda.synchronize()
        per_launch = int(counts.item()) / (args.warmup + args.launches)
        species = 1 if sa == sb else 2
        colliders = 2.0 * per_launch if sa == sb else 2.0 * n     # unlike: every A-member and (nearly) every B-member
        bytes_ = species * (40.0 * n + 12.0 * nc) + 48.0 * colliders
        rows.append({"launch": name, "ms": ms, "ms_all": every, "collisions_per_launch": per_launch,
                     "algorithmic_bytes": bytes_, "bytes_per_particle": bytes_ / (species * n),
                     "fraction_of_8TBps": bytes_ / (ms * 1e-3) / PEAK_BW,
                     "fraction_of_copy_ceiling": bytes_ / (ms * 1e-3) / COPY_CEILING})
    p_ms, p_all = timed(lambda: push(0))
    torch.cuda.synchronize()
    assert int(err[0]) == 0
    p_bytes = 96.0 * n + 32.0 * slab
    res = {"state": "fresh from the sort" if args.child == "fresh" else f"{args.decay} pushes after the sort",
           "launches": rows, "push_ms": p_ms, "push_ms_all": p_all,
           "push_fraction_of_copy_ceiling": p_bytes / (p_ms * 1e-3) / COPY_CEILING,
           "coulomb_step_over_push": {r["launch"]: r["ms"] / p_ms for r in rows},
           "device": torch.cuda.get_device_name(0)}
    Path(args.child_out).write_text(json.dumps(res))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--ppc", type=int, default=32)
    ap.add_argument("--decay", type=int, default=20)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=240, help="seconds allowed to each state's process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=["fresh", "decayed"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    from pinc_amd import build
    states = []
    with tempfile.TemporaryDirectory() as tmp:
        for state in ("fresh", "decayed"):
            part = Path(tmp) / f"{state}.json"
            cmd = [sys.executable, __file__, "--child", state, "--child-out", str(part)]
            for k in ("size", "ppc", "decay", "launches", "warmup"):
                cmd += [f"--{k}", str(getattr(args, k))]
            try:
                r = subprocess.run(cmd, timeout=args.timeout)
            except subprocess.TimeoutExpired:
                print(f"coulomb_probe: state {state} ran out of its {args.timeout} s; nothing more is started", file=sys.stderr)
                return 1
            if r.returncode != 0:
                print(f"coulomb_probe: state {state} ended with {r.returncode}; nothing more is started", file=sys.stderr)
                return 1
            states.append(json.loads(part.read_text()))
    res = {"tool": "tools/coulomb_probe.py", "size": args.size, "ppc": args.ppc, "particles_per_species": args.size ** 3 * args.ppc,
           "tile_width": 4, "launches": args.launches, "warmup": args.warmup, "copy_ceiling_Bps": COPY_CEILING,
           "kernel_resources": {k: v for k, v in build.kernel_resources().items() if "k_cou_" in k}, "states": states}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
