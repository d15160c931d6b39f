"""The phase-space histogram in the build: its symbols are exported and
declared, and the kernel keeps its registers (no GPU)."""
from pathlib import Path


def test_symbols_exported_and_declared(built):
    from pinc_amd import _lib
    root = Path(__file__).resolve().parent.parent
    hip_names = _lib.header_symbols(root / "include" / "pinc_hip.h")
    host_names = _lib.header_symbols(root / "include" / "pinc.h")
    for n in ("pinc_hip_phase_hist", "pinc_hip_phase_lds_bins"):
        assert hasattr(_lib.HIP, n), n
        assert n in hip_names, n
    for n in ("puPhaseHist", "pinc_sim_phase_hist", "pinc_sim_offset", "psOpenH5", "psWriteH5", "psCloseH5"):
        assert hasattr(_lib.HOST, n), n
        assert n in host_names, n


def test_phase_kernel_keeps_its_registers(built):
    """both instances (one axis, two axes): no spilled register, and two
    workgroups per CU next to their LDS boxes"""
    from pinc_amd import build
    hits = {k: v for k, v in build.kernel_resources().items() if "k_phase_hist" in k}
    assert len(hits) == 2, sorted(hits)
    for k, v in hits.items():
        assert v.get("vgpr_spill", -1) == 0, (k, v)
        assert v.get("sgpr_spill", -1) == 0, (k, v)
        assert v.get("occupancy", 0) >= 2, (k, v)
        assert 2 * v.get("lds", 1 << 30) <= 160 * 1024, (k, v)
