"""The order-2 (quadratic spline) operators in the build: their symbols are
exported and declared, and the kernels keep their registers (no GPU)."""
from pathlib import Path


def test_symbols_exported_and_declared(built):
    from pinc_amd import _lib
    root = Path(__file__).resolve().parent.parent
    hip_names = _lib.header_symbols(root / "include" / "pinc_hip.h")
    host_names = _lib.header_symbols(root / "include" / "pinc.h")
    for n in ("pinc_hip_deposit_tsc", "pinc_hip_accelerate_tsc"):
        assert hasattr(_lib.HIP, n), n
        assert n in hip_names, n
    for n in ("puAccND2_set", "puAccND2KE_set", "puDistrND2_set", "puAccND2KE", "puDistrND2"):
        assert hasattr(_lib.HOST, n), n
        assert n in host_names, n


def test_order2_kernels_keep_their_registers(built):
    """the 1-, 2- and 3-D instances of both kernels: no spilled register, and
    two workgroups per CU next to their LDS"""
    from pinc_amd import build
    res = build.kernel_resources()
    for name in ("k_deposit_tsc", "k_accel_tsc"):
        hits = {k: v for k, v in res.items() if name in k}
        assert len(hits) == 3, (name, sorted(hits))
        for k, v in hits.items():
            assert v.get("vgpr_spill", -1) == 0, (k, v)
            assert v.get("sgpr_spill", -1) == 0, (k, v)
            assert v.get("occupancy", 0) >= 2, (k, v)
            assert 2 * v.get("lds", 1 << 30) <= 160 * 1024, (k, v)
