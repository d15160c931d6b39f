#!/usr/bin/env python3
"""Time pinc_hip_phase_hist against a plain read of the same arrays and
against pinc_hip_deposit on the same particles.

One species of a warm plasma (v_th = 0.05 cells/step per component) on a
size^3 grid, ppc particles per cell, sorted by tile (pinc_hip_sort_tiles,
tile width 4): once fresh from the sort and once after `--decay` steps of
free streaming without a sort (x += v, periodic).  Three histograms:

    f(vx)    128 bins over +-0.3             a small box most of a wave hits
    (x, vx)  128 x 128                       a position axis: a small box inside
    (x, y)   1024 x 1024                     8 bins per cell: a box that stops
                                             fitting the LDS as the order decays

All kernels run in this process on the library's events: the median of
`--launches` launches after `--warmup` warm-ups.  `read_ms` is the time to
read the arrays the histogram names once (torch.sum of each): the roofline
of 8 B per particle and axis.  Algorithmic bytes of the histogram: 8 B per
particle and axis plus 8 B per touched bin.

    python tools/phase_probe.py --out profiles/phase_space.json
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


class PhaseT(C.Structure):
    """pinc_phase_t"""
    _fields_ = [("axis", C.c_int * 2), ("nbins", C.c_int * 2), ("shift", C.c_double * 2), ("lo", C.c_double * 2),
                ("scale", C.c_double * 2)]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--ppc", type=int, default=64)
    ap.add_argument("--decay", type=int, default=8)
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from pinc_amd import _lib
    from push_abi import Geom, Pop, geom_of
    hip = _lib.HIP
    vp = C.c_void_p
    hip.pinc_hip_phase_hist.argtypes = [Pop, C.c_int, C.POINTER(vp), PhaseT, vp, vp, vp]
    hip.pinc_hip_phase_lds_bins.restype = C.c_long
    hip.pinc_hip_deposit.argtypes = [Pop, C.c_int, Geom, vp, vp]
    hip.pinc_hip_sort_tiles.argtypes = [Pop, Pop, C.c_int, Geom, C.c_int, vp, C.c_long, C.POINTER(C.c_long), vp]
    hip.pinc_hip_tile_keys.argtypes = [Geom, C.c_int]
    hip.pinc_hip_tile_keys.restype = C.c_long
    hip.pinc_hip_event_create.argtypes = [C.POINTER(vp)]
    hip.pinc_hip_event_record.argtypes = [vp, vp]
    hip.pinc_hip_event_sync.argtypes = [vp]
    hip.pinc_hip_event_elapsed.argtypes = [C.POINTER(C.c_float), vp, vp]
    hip.pinc_hip_error_string.restype = C.c_char_p

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

    lo_x, hi_x = 0.5, S + 0.5
    shapes = [("f(vx)", (3,), (128,), (-0.3,), (0.3,)),
              ("(x, vx)", (0, 3), (128, 128), (lo_x, -0.3), (hi_x, 0.3)),
              ("(x, y)", (0, 1), (1024, 1024), (lo_x, lo_x), (hi_x, hi_x))]

    def spec_of(axes, bins, lo, hi):
        sp = PhaseT()
        sp.axis[1], sp.nbins[1], sp.scale[1] = -1, 1, 1.0
        for a in range(len(axes)):
            sp.axis[a], sp.nbins[a], sp.lo[a] = axes[a], bins[a], lo[a]
            sp.scale[a] = bins[a] / (hi[a] - lo[a])
        return sp

    rho = torch.zeros((S + 2) * S * S, dtype=torch.float64, device="cuda")
    ev = [vp(), vp()]
    for e in ev:
        assert hip.pinc_hip_event_create(C.byref(e)) == 0

    def timed(launch):
        ms = []
        for i in range(args.warmup + args.launches):
            hip.pinc_hip_event_record(ev[0], None)
            launch()
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
        arrays = xs + vs

        def deposit():
            assert hip.pinc_hip_deposit(pop, 0, geom, rho.data_ptr(), None) == 0, hip.pinc_hip_error_string()
        d_ms, d_all = timed(deposit)
        rows = []
        for name, axes, bins, lo, hi in shapes:
            nb = bins[0] * (bins[1] if len(bins) > 1 else 1)
            hist = torch.zeros(nb + 1, dtype=torch.int64, device="cuda")
            sp = spec_of(axes, bins, lo, hi)

            def phase():
                rc = hip.pinc_hip_phase_hist(pop, 0, vptr, sp, hist.data_ptr(), hist.data_ptr() + 8 * nb, None)
                assert rc == 0, hip.pinc_hip_error_string()

            def read():
                for a in axes:
                    arrays[a].sum()
            p_ms, p_all = timed(phase)
            r_ms, r_all = timed(read)
            h = hist.cpu()
            runs = args.warmup + args.launches
            assert int(h.sum()) == runs * n, (name, int(h.sum()), runs * n)
            bytes_ = 8.0 * n * len(axes) + 8.0 * int((h[:nb] > 0).sum())
            rows.append({"shape": name, "bins": list(bins), "phase_ms": p_ms, "read_ms": r_ms, "phase_over_read": p_ms / r_ms,
                         "phase_over_deposit": p_ms / d_ms, "outside_fraction": int(h[nb]) / (runs * n),
                         "phase_ms_all": p_all, "read_ms_all": r_all, "algorithmic_bytes": bytes_,
                         "fraction_of_8TBps": bytes_ / (p_ms * 1e-3) / PEAK_BW})
        return {"state": label, "deposit_ms": d_ms, "deposit_ms_all": d_all, "histograms": rows}

    runs = [measure("fresh from the sort")]
    for _ in range(args.decay):
        for x, v in zip(xs, vs):
            x += v
            x -= S * (x >= S + 0.5)
            x += S * (x < 0.5)
    torch.cuda.synchronize()
    runs.append(measure(f"{args.decay} steps after the sort"))
    res = {"tool": "tools/phase_probe.py", "label": args.label, "lds_bins": hip.pinc_hip_phase_lds_bins(), "size": S,
           "ppc": args.ppc, "particles": n, "tile_width": tw, "launches": args.launches, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "runs": runs}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
