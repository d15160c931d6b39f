"""ctypes mirror of the particle part of include/pinc_hip.h, shared by the
GPU tests that call libpinc_hip.so's C ABI directly, and helpers that put a
species on the device (torch memory).
"""
import ctypes as C

import numpy as np


class Geom(C.Structure):
    """pinc_geom_t"""
    _fields_ = [("nd", C.c_int), ("T", C.c_int * 3), ("nloc", C.c_int), ("off", C.c_int), ("nranks", C.c_int),
                ("literal", C.c_int)]


class Pop(C.Structure):
    """pinc_pop_t"""
    _fields_ = [("x", C.c_void_p * 3), ("v", C.c_void_p * 3), ("nSpecies", C.c_int), ("nd", C.c_int),
                ("iStart", C.c_long * 9), ("iStop", C.c_long * 8)]


class PushArgs(C.Structure):
    """pinc_push_t"""
    _fields_ = [("xout", C.c_void_p * 3), ("vout", C.c_void_p * 3), ("kick", C.c_int), ("Es", C.c_void_p),
                ("rhoS", C.c_void_p), ("thr", C.c_void_p), ("flags", C.c_void_p), ("chunkCount", C.c_void_p),
                ("maxVel", C.c_double), ("errFlag", C.c_void_p), ("wrapMask", C.c_int), ("kePartial", C.c_void_p),
                ("tileWidth", C.c_int), ("cursor", C.c_void_p), ("cntNext", C.c_void_p), ("moved", C.c_void_p),
                ("spread", C.c_void_p), ("tstamp", C.c_void_p), ("diag", C.c_void_p), ("objInside", C.c_void_p),
                ("objSy", C.c_long), ("objSz", C.c_long), ("objNodes", C.c_long), ("objCount", C.c_void_p),
                ("objLo", C.c_int * 3), ("objHi", C.c_int * 3), ("emigTotal", C.c_void_p),
                ("flagsSparse", C.c_int)]


def geom_of(T) -> Geom:
    """one rank's geometry of true sizes T (x first, 1 to 3 entries)"""
    nd = len(T)
    full = tuple(T) + (1,) * (3 - nd)
    return Geom(nd, (C.c_int * 3)(*full), T[nd - 1], 0, 1, 0)


SENTINEL = -7.25   # fills every slot outside a species' live range


class DevSpecies:
    """Species 0 of an nd-dimensional population at [start, start + n) of
    SoA device arrays (torch memory) with `pad` more slots behind it; every
    slot outside the live range holds `fill`.  Keeps the tensors alive."""

    def __init__(self, pos: np.ndarray, vel: np.ndarray, start: int = 0, pad: int = 7, fill: float = SENTINEL):
        self.n, self.nd = pos.shape
        self.start, self.cap, self.fill = start, start + self.n + pad, fill
        self.xs = [self._put(pos[:, d]) for d in range(self.nd)]
        self.vs = [self._put(vel[:, d]) for d in range(self.nd)]
        self.pop = Pop(self.ptrs(self.xs), self.ptrs(self.vs), 1, self.nd, (C.c_long * 9)(start, self.cap),
                       (C.c_long * 8)(start + self.n))

    def _put(self, col):
        import torch
        a = np.full(self.cap, self.fill)
        a[self.start:self.start + self.n] = col
        return torch.from_numpy(a).cuda()

    @classmethod
    def blank(cls, n: int, nd: int, start: int = 0, pad: int = 7):
        z = np.full((n, nd), SENTINEL)
        return cls(z, z, start, pad)

    def live(self, ts) -> np.ndarray:
        """(n, nd) host copy of the live range of tensors ts"""
        return np.stack([t.cpu().numpy()[self.start:self.start + self.n] for t in ts], 1)

    def padding_untouched(self, ts) -> bool:
        for t in ts:
            a = t.cpu().numpy()
            if not (np.all(a[:self.start] == self.fill) and np.all(a[self.start + self.n:] == self.fill)):
                return False
        return True

    def ptrs(self, ts):
        return (C.c_void_p * 3)(*([t.data_ptr() for t in ts] + [None] * (3 - self.nd)))


def device_pop(pos: np.ndarray, vel: np.ndarray, start: int = 0):
    """(pop, position tensors, velocity tensors) of a DevSpecies with zero padding"""
    d = DevSpecies(pos, vel, start, pad=5, fill=0.0)
    return d.pop, d.xs, d.vs
