#!/usr/bin/env python3
"""Time the order-2 kernels against the order-1 ones on the same particles:
pinc_hip_deposit_tsc against pinc_hip_deposit (k_deposit_tiled) and
pinc_hip_accelerate_tsc against pinc_hip_accelerate (k_accel).

One species of a warm plasma (v_th = 0.05 cells/step per component) on a
size^3 grid, ppc particles per cell, sorted by tile (pinc_hip_sort_tiles,
tile width 4): once fresh from the sort and once after `--decay` steps of
free streaming without a sort (x += v, periodic in [0.5, T + 0.5)).  All four
kernels run in this process on the library's events: the median of
`--launches` launches after `--warmup` warm-ups.  The accelerations kick with
a zero field, so the velocities (and the decay) are the same for every launch.

    python tools/order2_probe.py --out profiles/order2.json
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--ppc", type=int, default=64)
    ap.add_argument("--decay", type=int, default=8)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from pinc_amd import _lib
    hip = _lib.HIP
    vp = C.c_void_p
    # one mirror of the structs for every call: pinc_amd._lib's, as its prototypes of the order-2 pair use
    Geom, Pop = _lib.HipGeom, _lib.HipPop
    hip.pinc_hip_deposit.argtypes = [Pop, C.c_int, Geom, vp, vp]
    hip.pinc_hip_accelerate.argtypes = [Pop, C.c_int, Geom, vp, vp, C.POINTER(C.c_int), vp]
    hip.pinc_hip_sort_tiles.argtypes = [Pop, Pop, C.c_int, Geom, C.c_int, vp, C.c_long, C.POINTER(C.c_long), vp]
    hip.pinc_hip_tile_keys.argtypes = [Geom, C.c_int]
    hip.pinc_hip_tile_keys.restype = C.c_long
    hip.pinc_hip_event_create.argtypes = [C.POINTER(vp)]
    hip.pinc_hip_event_record.argtypes = [vp, vp]
    hip.pinc_hip_event_sync.argtypes = [vp]
    hip.pinc_hip_event_elapsed.argtypes = [C.POINTER(C.c_float), vp, vp]

    S, nd, tw = args.size, 3, 4
    n = S ** 3 * args.ppc
    geom = Geom(nd, (C.c_int * 3)(S, S, S), S, 0, 1, 0)
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
    del xs, vs
    xs, vs = ox, ov

    nodes = (S + 2) * S * S
    rho = torch.zeros(nodes, dtype=torch.float64, device="cuda")
    Es = torch.zeros(nodes * nd, dtype=torch.float64, device="cuda")
    ke = torch.zeros(n // 2048 + 2, dtype=torch.float64, device="cuda")
    nb = C.c_int()
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

    def measure(label):
        pop = pop_of(xs, vs)
        row = {"state": label}
        for key, fn in (("deposit_tsc", hip.pinc_hip_deposit_tsc), ("deposit_tiled", hip.pinc_hip_deposit)):
            row[key + "_ms"], row[key + "_ms_all"] = timed(lambda: fn(pop, 0, geom, rho.data_ptr(), None))
        for key, fn in (("accel_tsc", hip.pinc_hip_accelerate_tsc), ("accel", hip.pinc_hip_accelerate)):
            row[key + "_ms"], row[key + "_ms_all"] = timed(
                lambda: fn(pop, 0, geom, Es.data_ptr(), ke.data_ptr(), C.byref(nb), None))
        row["deposit_ratio"] = row["deposit_tsc_ms"] / row["deposit_tiled_ms"]
        row["accel_ratio"] = row["accel_tsc_ms"] / row["accel_ms"]
        return row

    rows = [measure("fresh from the sort")]
    for _ in range(args.decay):
        for x, v in zip(xs, vs):
            x += v
            x -= S * (x >= S + 0.5)
            x += S * (x < 0.5)
    torch.cuda.synchronize()
    rows.append(measure(f"{args.decay} steps after the sort"))
    res = {"tool": "tools/order2_probe.py", "size": S, "ppc": args.ppc, "particles": n, "tile_width": tw,
           "launches": args.launches, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "runs": rows}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
