"""pinc_amd.build refuses any target but gfx950 before it starts a compiler
(the kernels use gfx950-only lane swaps unconditionally)."""
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_other_arch_is_rejected_before_any_compile(tmp_path):
    lib = tmp_path / "lib_gfx942"
    env = dict(os.environ, PINC_ARCH="gfx942", PINC_LIBDIR=str(lib))
    env.pop("PINC_HIP_DEFINES", None)
    r = subprocess.run([sys.executable, "-m", "pinc_amd.build"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode != 0
    lines = [ln for ln in (r.stdout + r.stderr).splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    assert "gfx950" in lines[0] and "gfx942" in lines[0]
    # neither the library directory nor its object directory was created
    assert not lib.exists()
    assert not (ROOT / "build" / ("obj_" + lib.name)).exists()
