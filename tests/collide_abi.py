"""ctypes mirror of pinc_collide_t (include/pinc_hip.h), shared by the tests
that call pinc_hip_collide directly and by tools/collide_probe.py."""
import ctypes as C


class CollideT(C.Structure):
    """pinc_collide_t"""
    _fields_ = [("nu", C.c_double * 2), ("sig", C.c_double * 2), ("b", C.c_double), ("vth", C.c_double),
                ("drift", C.c_double * 3), ("h", C.c_double * 3), ("key", C.c_ulonglong)]


def params_t(par, key: int) -> CollideT:
    """a collide_ref.Params and a key as the kernel's argument"""
    return CollideT((C.c_double * 2)(*par.nu), (C.c_double * 2)(*par.sig), par.b, par.vth, (C.c_double * 3)(*par.drift),
                    (C.c_double * 3)(*par.h), key)
