"""The ionisation operator in the build: its symbols are exported and
declared, and the kernels keep their registers (no GPU)."""
from pathlib import Path


def test_symbols_exported_and_declared(built):
    from pinc_amd import _lib
    root = Path(__file__).resolve().parent.parent
    hip_names = _lib.header_symbols(root / "include" / "pinc_hip.h")
    host_names = _lib.header_symbols(root / "include" / "pinc.h")
    for n in ("pinc_hip_ionize", "pinc_hip_ionize_work", "pinc_hip_ionize_chunk", "pinc_hip_ionize_key"):
        assert hasattr(_lib.HIP, n), n
        assert n in hip_names, n
    for n in ("mccIonize", "mccIonizations", "pinc_sim_ionizations"):
        assert hasattr(_lib.HOST, n), n
        assert n in host_names, n


def test_ionize_kernels_keep_their_registers(built):
    """the twelve instances (1-D, 2-D, 3-D; a cross section or the rate alone;
    the counting and the writing pass): no spilled register, and k_collide's
    bar of four waves per SIMD"""
    from pinc_amd import build
    hits = {k: v for k, v in build.kernel_resources().items() if "k_ionize" in k}
    assert len(hits) == 12, sorted(hits)
    for k, v in hits.items():
        assert v.get("vgpr_spill", -1) == 0, (k, v)
        assert v.get("sgpr_spill", -1) == 0, (k, v)
        assert v.get("occupancy", 0) >= 4, (k, v)
