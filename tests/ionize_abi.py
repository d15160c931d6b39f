"""ctypes mirror of pinc_ionize_t and of pinc_hip_ionize's entry points
(include/pinc_hip.h), shared by the tests that call them directly."""
import ctypes as C

from push_abi import Pop


class IonizeT(C.Structure):
    """pinc_ionize_t"""
    _fields_ = [("nu", C.c_double), ("sig", C.c_double), ("wth", C.c_double), ("vth", C.c_double),
                ("drift", C.c_double * 3), ("h", C.c_double * 3), ("target", C.c_int), ("key", C.c_ulonglong)]


def params_t(par, key: int) -> IonizeT:
    """an ionize_ref.Params and a key as the kernel's argument"""
    return IonizeT(par.nu, par.sig, par.wth, par.vth, (C.c_double * 3)(*par.drift), (C.c_double * 3)(*par.h),
                   par.target, key)


def bind(hip):
    """argument and result types of the ionisation entry points of libpinc_hip.so"""
    vp = C.c_void_p
    hip.pinc_hip_ionize.argtypes = [Pop, C.c_int, IonizeT, vp, C.c_long, vp, vp]
    hip.pinc_hip_ionize.restype = C.c_int
    hip.pinc_hip_ionize_work.argtypes = [C.c_long]
    hip.pinc_hip_ionize_work.restype = C.c_long
    hip.pinc_hip_ionize_chunk.restype = C.c_long
    hip.pinc_hip_ionize_key.argtypes = [C.c_ulonglong, C.c_ulonglong, C.c_int, C.c_int]
    hip.pinc_hip_ionize_key.restype = C.c_ulonglong
    hip.pinc_hip_error_string.restype = C.c_char_p
    return hip
