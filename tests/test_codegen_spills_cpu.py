"""Register-spill guard of the raycast kernels (no GPU: hipcc cross-compiles gfx950).  The class-table march is a chain of
dependent instructions, and every scalar register the allocator parks in a VGPR lane comes back with a v_readlane on that
chain: no k_raycast_* kernel may use scratch, spill VGPRs or spill more SGPRs than it used to, and the LDS-mode class kernels
stay at the numbers scripts/check_raycast_spills.py pins."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_raycast_kernels_keep_their_spill_limits():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_raycast_spills.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert ", 0 over their spill limits, 0 pinned kernels missing" in out.stdout and "k_raycast_sdf_classes<RayF32,0>" in out.stdout
