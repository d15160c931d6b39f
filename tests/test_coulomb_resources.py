"""The Coulomb collision operator in the build: its symbols are exported and
declared, the kernels keep their registers, and the pairing kernel's LDS is
what pinc_hip_coulomb_cell_cap() says (no GPU)."""
import ctypes as C
from pathlib import Path


def test_symbols_exported_and_declared(built):
    from pinc_amd import _lib
    root = Path(__file__).resolve().parent.parent
    hip_names = _lib.header_symbols(root / "include" / "pinc_hip.h")
    host_names = _lib.header_symbols(root / "include" / "pinc.h")
    for n in ("pinc_hip_coulomb", "pinc_hip_coulomb_key", "pinc_hip_coulomb_work", "pinc_hip_coulomb_cell_cap"):
        assert hasattr(_lib.HIP, n), n
        assert n in hip_names, n
    for n in ("mccCoulomb", "mccCoulombActive", "mccCoulombCoef", "mccCoulombCounts", "pinc_sim_coulomb_count",
              "pinc_sim_coulomb_coef"):
        assert hasattr(_lib.HOST, n), n
        assert n in host_names, n


def test_coulomb_kernels_spill_nothing_and_lds_matches_the_cap(built):
    """count, scatter and the two pairing instances: no spilled register.  A
    pairing workgroup is four waves; each orders up to cap members per species
    of the launch with an 8-byte hash key, the index and the ordered index
    (16 bytes per member), next to one copy of the parameters (below 512 B)."""
    from pinc_amd import _lib, build
    f = _lib.HIP.pinc_hip_coulomb_cell_cap
    f.restype = C.c_long
    cap = int(f())
    assert cap >= 65
    hits = {k: v for k, v in build.kernel_resources().items() if "k_cou_" in k}
    assert len(hits) == 4, sorted(hits)
    for k, v in hits.items():
        assert v["source"] == "k_coulomb.hip"
        assert v.get("vgpr_spill", -1) == 0, (k, v)
        assert v.get("sgpr_spill", -1) == 0, (k, v)
    pair = {k: v for k, v in hits.items() if "k_cou_pair" in k}
    assert len(pair) == 2
    for k, v in pair.items():
        species = 2 if "ILb1E" in k else 1
        lists = 4 * species * cap * 16
        assert lists <= v["lds"] < lists + 512, (k, v, lists)
