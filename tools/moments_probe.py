#!/usr/bin/env python3
"""Time pinc_hip_moments against pinc_hip_deposit on the same particles.

One species of a warm plasma (v_th = 0.05 cells/step per component) on a
size^3 grid, ppc particles per cell, sorted by tile (pinc_hip_sort_tiles,
tile width 4): once fresh from the sort and once after `--decay` steps of
free streaming without a sort (x += v, periodic; at this temperature the
field's kick does not change how the order decays).  Both kernels run in this
process on the library's events: the median of `--launches` launches after
`--warmup` warm-ups.  Algorithmic bytes of the moments: 48 B per particle
plus 8 NM B per node.

    python tools/moments_probe.py --out profiles/moments.json
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
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from pinc_amd import _lib
    from push_abi import Geom, Pop, geom_of
    hip = _lib.HIP
    vp = C.c_void_p
    hip.pinc_hip_moments.argtypes = [Pop, C.c_int, Geom, C.POINTER(vp), vp, vp]
    hip.pinc_hip_deposit.argtypes = [Pop, C.c_int, Geom, vp, vp]
    hip.pinc_hip_sort_tiles.argtypes = [Pop, Pop, C.c_int, Geom, C.c_int, vp, C.c_long, C.POINTER(C.c_long), vp]
    hip.pinc_hip_tile_keys.argtypes = [Geom, C.c_int]
    hip.pinc_hip_tile_keys.restype = C.c_long
    hip.pinc_hip_event_create.argtypes = [C.POINTER(vp)]
    hip.pinc_hip_event_record.argtypes = [vp, vp]
    hip.pinc_hip_event_sync.argtypes = [vp]
    hip.pinc_hip_event_elapsed.argtypes = [C.POINTER(C.c_float), vp, vp]

    S, nd, nm, tw = args.size, 3, 10, 4
    n = S ** 3 * args.ppc
    geom = geom_of((S, S, S))
    gen = torch.Generator(device="cuda").manual_seed(1)
    xs = [0.5 + S * torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) for _ in range(nd)]
    xs = [torch.clamp(x, max=S + 0.5 - 1e-9) for x in xs]
    vs = [0.05 * torch.randn(n, dtype=torch.float64, device="cuda", generator=gen) for _ in range(nd)]

    def pop_of(x, v):
        return Pop((vp * 3)(*[t.data_ptr() for t in x]), (vp * 3)(*[t.data_ptr() for t in v]), 1, nd,
                   (C.c_long * 9)(0, n), (C.c_long * 8)(n))

    # sort by tile into a second set of arrays
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
    mom = torch.zeros(nodes * nm, dtype=torch.float64, device="cuda")
    rho = torch.zeros(nodes, dtype=torch.float64, device="cuda")
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
        vptr = (vp * 3)(*[t.data_ptr() for t in vs])
        m_ms, m_all = timed(lambda: hip.pinc_hip_moments(pop, 0, geom, vptr, mom.data_ptr(), None))
        d_ms, d_all = timed(lambda: hip.pinc_hip_deposit(pop, 0, geom, rho.data_ptr(), None))
        bytes_ = 48.0 * n + 8.0 * nm * nodes
        return {"state": label, "moments_ms": m_ms, "deposit_ms": d_ms, "ratio": m_ms / d_ms,
                "moments_ms_all": m_all, "deposit_ms_all": d_all, "algorithmic_bytes": bytes_,
                "fraction_of_8TBps": bytes_ / (m_ms * 1e-3) / PEAK_BW}

    rows = [measure("fresh from the sort")]
    for _ in range(args.decay):
        for x, v in zip(xs, vs):
            x += v
            x -= S * (x >= S + 0.5)
            x += S * (x < 0.5)
    torch.cuda.synchronize()
    rows.append(measure(f"{args.decay} steps after the sort"))
    res = {"tool": "tools/moments_probe.py", "size": S, "ppc": args.ppc, "particles": n, "tile_width": tw,
           "launches": args.launches, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "runs": rows}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
