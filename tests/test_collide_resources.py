"""The collision operator in the build: its symbols are exported and
declared, and the kernel keeps its registers (no GPU)."""
from pathlib import Path


def test_symbols_exported_and_declared(built):
    from pinc_amd import _lib
    root = Path(__file__).resolve().parent.parent
    hip_names = _lib.header_symbols(root / "include" / "pinc_hip.h")
    host_names = _lib.header_symbols(root / "include" / "pinc.h")
    for n in ("pinc_hip_collide", "pinc_hip_collide_key", "pinc_hip_collide_chunk"):
        assert hasattr(_lib.HIP, n), n
        assert n in hip_names, n
    for n in ("mccAlloc", "mccCollide", "mccFree", "mccCounts", "pinc_sim_collisions"):
        assert hasattr(_lib.HOST, n), n
        assert n in host_names, n


def test_collide_kernel_keeps_its_registers(built):
    """the six instances (1-D, 2-D, 3-D; cross sections or rates alone): no
    spilled register"""
    from pinc_amd import build
    hits = {k: v for k, v in build.kernel_resources().items() if "k_collide" in k}
    assert len(hits) == 6, sorted(hits)
    for k, v in hits.items():
        assert v.get("vgpr_spill", -1) == 0, (k, v)
        assert v.get("sgpr_spill", -1) == 0, (k, v)
        assert v.get("occupancy", 0) >= 4, (k, v)
