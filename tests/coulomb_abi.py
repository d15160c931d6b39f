"""ctypes mirror of pinc_coulomb_t (include/pinc_hip.h), shared by the tests
that call pinc_hip_coulomb directly and by tools/coulomb_probe.py (the timing probe)."""
import ctypes as C


class CoulombT(C.Structure):
    """pinc_coulomb_t"""
    _fields_ = [("K", C.c_double), ("fa", C.c_double), ("fb", C.c_double), ("h", C.c_double * 3),
                ("key", C.c_ulonglong)]


def params_t(par, key: int) -> CoulombT:
    """a coulomb_ref.Params and a key as the kernel's argument"""
    return CoulombT(par.K, par.fa, par.fb, (C.c_double * 3)(*par.h), key)


def declare(hip):
    """argument and result types of the pinc_hip_coulomb entry points"""
    from push_abi import Geom, Pop
    vp = C.c_void_p
    hip.pinc_hip_coulomb.argtypes = [Pop, C.c_int, C.c_int, Geom, CoulombT, vp, C.c_long, vp, vp]
    hip.pinc_hip_coulomb_work.argtypes = [C.c_long, C.c_long, C.c_long]
    hip.pinc_hip_coulomb_work.restype = C.c_long
    hip.pinc_hip_coulomb_cell_cap.restype = C.c_long
    hip.pinc_hip_coulomb_key.argtypes = [C.c_ulonglong, C.c_ulonglong, C.c_int, C.c_int, C.c_int]
    hip.pinc_hip_coulomb_key.restype = C.c_ulonglong
    hip.pinc_hip_error_string.restype = C.c_char_p
    return hip
