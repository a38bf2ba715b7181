"""roo::BrickPack / roo::BrickUnpack from C++ (include/kangaroo/VolumeBricks.h over include/kfx_bricks.h): BoundedVolume<SDF_t>, <SDF_h>
and <float> packed on the device against a loop on the host, reset and unpacked again (apps/roo_bricks_test)."""
import os
import subprocess

import pytest

import kfx_testlib as T

APPS = os.path.join(T.ROOT, "apps")
pytestmark = pytest.mark.gpu


def test_cpp_roo_bricks_test():
    subprocess.check_call(["make", "-C", APPS, "roo_bricks_test"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(APPS, "roo_bricks_test")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "passed" in out.stdout, out.stdout + out.stderr
