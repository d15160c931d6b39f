"""The multigrid host driver's decisions as pure functions (pinc_mg.c), no GPU.

* pinc_mg_smooth_form: which smoother a native level gets (colour passes,
  single fused sweeps, double fused sweeps).
* pinc_mg_smooth_next: the launch schedule of one smoothing, which
  smooth_native walks step by step.
* pinc_mg_stop: the one stop rule of every solve.
"""
import ctypes as C
import math

import pytest

PASSES, SINGLE, DOUBLE = 0, 1, 2
CONTINUE, CONVERGED, STOP_CAP, STOP_NONFINITE, ERROR = range(5)
FUSED_MIN = 1 << 23


class _Lvl(C.Structure):
    _fields_ = [("nd", C.c_int), ("T", C.c_int * 3)]


@pytest.fixture(scope="module")
def host(built):
    from pinc_amd import _lib
    h = _lib.HOST
    h.pinc_mg_smooth_form.restype = C.c_int
    h.pinc_mg_smooth_form.argtypes = [_Lvl, C.c_long, C.c_int, C.c_int, C.c_long, C.c_int]
    h.pinc_mg_smooth_next.restype = C.c_int
    h.pinc_mg_smooth_next.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    h.pinc_mg_stop.restype = C.c_int
    h.pinc_mg_stop.argtypes = [C.c_double, C.c_long, C.c_long, C.c_int]
    return h


def _form(h, T, fused_min=FUSED_MIN, nd3=1, shard0=0, aligned=1):
    nd = len(T)
    T = tuple(T) + (1,) * (3 - nd)
    return h.pinc_mg_smooth_form(_Lvl(nd, (C.c_int * 3)(*T)), T[0] * T[1] * T[2], nd3, shard0, fused_min, aligned)


# (extents, fusedMin, sharded level 0, form) with nd3 = 1 and aligned buffers
FORMS = [
    ((256, 256, 256), FUSED_MIN, 0, DOUBLE),
    ((128, 128, 128), FUSED_MIN, 0, PASSES),
    ((128, 128, 128), 1, 0, DOUBLE),
    ((16, 16, 16), 1, 0, SINGLE),
    ((48, 48, 48), 1, 0, SINGLE),
    ((32, 8, 16), 1, 0, PASSES),       # y is not a multiple of 16
    ((24, 16, 16), 1, 0, PASSES),
    ((256, 256, 80), FUSED_MIN, 1, DOUBLE),  # 5.2 M points >= 2^23 / 4
    ((256, 256, 80), FUSED_MIN, 0, PASSES),
    ((256, 256), 1, 0, PASSES),        # a 2-D level
]


@pytest.mark.parametrize("T,fused_min,shard0,form", FORMS)
def test_smooth_form_table(host, T, fused_min, shard0, form):
    assert _form(host, T, fused_min, shard0=shard0) == form
    # the N-D smoother of this phase: colour passes whatever the level
    assert _form(host, T, fused_min, nd3=0, shard0=shard0) == PASSES
    # a misaligned buffer costs a double-capable level its x-pair fetches only
    assert _form(host, T, fused_min, shard0=shard0, aligned=0) == (SINGLE if form == DOUBLE else form)


def _schedule(h, form, shard0, n_iter, pre_done=False):
    """smooth_native's walk: D/S a double/single sweep phi -> res, then the
    pointer swap (>) or the launch back (=); P a red and a black pass."""
    out, k, it = [], 2 if pre_done else 0, C.c_int()
    while k < n_iter:
        kind = h.pinc_mg_smooth_next(form, shard0, n_iter - k, C.byref(it))
        back = shard0 or kind != DOUBLE
        out.append("P" if kind == PASSES else "DS"[kind == SINGLE] + "=>"[not back])
        assert it.value == {"P": 1, "S=": 2, "D>": 2, "D=": 4}[out[-1]]
        k += it.value
    return out


@pytest.mark.parametrize("form,shard0,n_iter,pre_done,seq", [
    (DOUBLE, 0, 10, False, ["D>"] * 5),
    (DOUBLE, 0, 3, False, ["D>", "P"]),
    (DOUBLE, 0, 10, True, ["D>"] * 4),   # the queued sweep counts as the first two iterations
    (DOUBLE, 0, 1, False, ["P"]),
    (DOUBLE, 1, 4, False, ["D="]),
    (DOUBLE, 1, 6, False, ["D=", "S="]),
    (DOUBLE, 1, 5, False, ["D=", "P"]),
    (SINGLE, 0, 5, False, ["S=", "S=", "P"]),
    (SINGLE, 1, 5, False, ["S=", "S=", "P"]),
    (PASSES, 0, 7, False, ["P"] * 7),
    (PASSES, 1, 4, False, ["P"] * 4),
])
def test_smooth_schedule_table(host, form, shard0, n_iter, pre_done, seq):
    assert _schedule(host, form, shard0, n_iter, pre_done) == seq


@pytest.mark.parametrize("res,cycles,cap,diagnostic,want", [
    (1e-11, 3, 0, 0, CONVERGED),
    (1e-3, 3, 40, 1, CONTINUE),
    (1e-3, 3, 0, 0, CONTINUE),
    (1e-3, 40, 40, 1, STOP_CAP),
    (math.nan, 3, 40, 1, STOP_NONFINITE),
    (math.inf, 3, 40, 1, STOP_NONFINITE),
    (math.nan, 3, 0, 0, ERROR),
    (math.inf, 3, 0, 0, ERROR),
    (math.inf, 3, 40, 0, ERROR),          # a PINC_MG_MAX_CYCLES cap is no diagnostic limit
    (1e-3, 1000000, 0, 0, CONTINUE),
    (1e-3, 1000001, 0, 0, ERROR),
])
def test_stop_rule(host, res, cycles, cap, diagnostic, want):
    assert host.pinc_mg_stop(res, cycles, cap, diagnostic) == want
