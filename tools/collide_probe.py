#!/usr/bin/env python3
"""Time pinc_hip_collide against a plain read of the same velocity arrays.

One species of a warm plasma (v_th = 0.05 cells/step per component) on a
size^3 grid, ppc particles per cell, sorted by tile (pinc_hip_sort_tiles,
tile width 4).  Three cases:
    frequency   nu = (0.005, 0.005), sig = 0: one draw per particle, no
                velocity read; the ~1 % that collide are listed per workgroup
                and processed densely
    sigma       sig = (0.1, 0.1): the neutral sampled for every particle
    two in three  nu = (0.5, 0.5): P = 1 - 1/e, 63 % collide and are stored
    everyone    nu = (20, 20): every particle collides
each measured fresh from the sort and after `--decay` steps (x += v, periodic,
one collision step of the case per step: the kernel never reads positions, so
the two states differ by the velocities only).  Next to them the plain read:
pinc_hip_vel_assert over the same three arrays (24 B per particle, nothing
written).  All on the library's events in this process: the median of
`--launches` launches after `--warmup` warm-ups; every launch gets a new key.
Algorithmic bytes of a collision launch as reported: 24 B read per particle
plus 48 B per collider (the sectors around a stored component are not
counted); with rates alone the kernel reads the colliders' velocities only,
so its time there is the draws', not the bytes'.

    python tools/collide_probe.py --out profiles/collisions.json
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

PEAK_BW = 8.0e12  # B/s


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--ppc", type=int, default=64)
    ap.add_argument("--decay", type=int, default=8)
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--label", default="", help="a note kept in the output (the store form of a variant build)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from pinc_amd import _lib, build
    from push_abi import Geom, Pop, geom_of
    from collide_abi import CollideT
    hip = _lib.HIP
    vp = C.c_void_p
    hip.pinc_hip_collide.argtypes = [Pop, C.c_int, C.POINTER(vp), CollideT, vp, vp]
    hip.pinc_hip_collide_key.restype = C.c_ulonglong
    hip.pinc_hip_collide_key.argtypes = [C.c_ulonglong, C.c_ulonglong, C.c_int, C.c_int]
    hip.pinc_hip_vel_assert.argtypes = [Pop, C.c_int, C.c_double, vp, vp]
    hip.pinc_hip_sort_tiles.argtypes = [Pop, Pop, C.c_int, Geom, C.c_int, vp, C.c_long, C.POINTER(C.c_long), vp]
    hip.pinc_hip_tile_keys.argtypes = [Geom, C.c_int]
    hip.pinc_hip_tile_keys.restype = C.c_long
    hip.pinc_hip_event_create.argtypes = [C.POINTER(vp)]
    hip.pinc_hip_event_record.argtypes = [vp, vp]
    hip.pinc_hip_event_sync.argtypes = [vp]
    hip.pinc_hip_event_elapsed.argtypes = [C.POINTER(C.c_float), vp, vp]

    S, nd, tw = args.size, 3, 4
    n = S ** 3 * args.ppc
    geom = geom_of((S, S, S))
    gen = torch.Generator(device="cuda").manual_seed(1)
    xs = [0.5 + S * torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) for _ in range(nd)]
    xs = [torch.clamp(x, max=S + 0.5 - 1e-9) for x in xs]
    vs = [0.05 * torch.randn(n, dtype=torch.float64, device="cuda", generator=gen) for _ in range(nd)]

    def pop_of(x, v):
        return Pop((vp * 3)(*[t.data_ptr() for t in x]), (vp * 3)(*[t.data_ptr() for t in v]), 1, nd,
                   (C.c_long * 9)(0, n), (C.c_long * 8)(n))

    ox = [torch.empty_like(t) for t in xs]
    ov = [torch.empty_like(t) for t in vs]
    K = hip.pinc_hip_tile_keys(geom, tw)
    cap = 2 * (K + 1) + 2 * (K // 4096 + 1) + 1
    work = torch.zeros(cap, dtype=torch.int32, device="cuda")
    nk = C.c_long()
    rc = hip.pinc_hip_sort_tiles(pop_of(xs, vs), pop_of(ox, ov), 0, geom, tw, work.data_ptr(), cap, C.byref(nk), None)
    assert rc == 0, hip.pinc_hip_error_string()
    torch.cuda.synchronize()
    del xs, vs, work
    xs, v_sorted = ox, ov

    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    err = torch.zeros(16, dtype=torch.int32, device="cuda")
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

    cases = {"frequency": ((0.005, 0.005), (0.0, 0.0)), "sigma": ((0.0, 0.0), (0.1, 0.1)),
             "two in three": ((0.5, 0.5), (0.0, 0.0)), "everyone": ((20.0, 20.0), (0.0, 0.0))}
    rows = []
    for name, (nu, sig) in cases.items():
        vs = [t.clone() for t in v_sorted]
        x = [t.clone() for t in xs]
        pop = pop_of(x, vs)
        vptr = (vp * 3)(*[t.data_ptr() for t in vs])
        step = [0]

        def collide():
            par = CollideT((C.c_double * 2)(*nu), (C.c_double * 2)(*sig), 0.5, 0.05, (C.c_double * 3)(0, 0, 0),
                           (C.c_double * 3)(1, 1, 1), hip.pinc_hip_collide_key(9, step[0], 0, 0))
            step[0] += 1
            return hip.pinc_hip_collide(pop, 0, vptr, par, counts.data_ptr(), None)

        def read():
            return hip.pinc_hip_vel_assert(pop, 0, 1e300, err.data_ptr(), None)

        def measure(label):
            counts.zero_()
            c_ms, c_all = timed(collide)
            torch.cuda.synchronize()
            hit = int(counts.sum().item()) / (n * (args.warmup + args.launches))
            r_ms, r_all = timed(read)
            bytes_ = 24.0 * n + 48.0 * n * hit
            return {"case": name, "nu": nu, "sig": sig, "state": label, "collide_ms": c_ms, "read_ms": r_ms,
                    "read_over_collide": r_ms / c_ms, "collided_fraction": hit, "collide_ms_all": c_all,
                    "read_ms_all": r_all, "algorithmic_bytes": bytes_,
                    "fraction_of_8TBps": bytes_ / (c_ms * 1e-3) / PEAK_BW,
                    "read_fraction_of_8TBps": 24.0 * n / (r_ms * 1e-3) / PEAK_BW}

        rows.append(measure("fresh from the sort"))
        for _ in range(args.decay):
            for xx, v in zip(x, vs):
                xx += v
                xx -= S * (xx >= S + 0.5)
                xx += S * (xx < 0.5)
            assert collide() == 0
        torch.cuda.synchronize()
        rows.append(measure(f"{args.decay} steps after the sort"))
        del vs, x

    res = {"tool": "tools/collide_probe.py", "label": args.label, "size": S, "ppc": args.ppc, "particles": n,
           "tile_width": tw, "launches": args.launches, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0),
           "kernel_resources": {k: v for k, v in build.kernel_resources().items() if "k_collide" in k}, "runs": rows}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
