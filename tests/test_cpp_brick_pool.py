"""The brick pool from C++ (roo::BrickPool* of include/kangaroo/VolumeBricks.h over include/kfx_brick_pool.h): a sub-view of a
BoundedVolume<SDF_t>, <SDF_h> and <float> spilled into a pool, the pool read as a map against a loop on the host, the volume overwritten
and restored (apps/roo_brick_pool_test)."""
import os
import subprocess

import pytest

import kfx_testlib as T

APPS = os.path.join(T.ROOT, "apps")
pytestmark = pytest.mark.gpu


def test_cpp_roo_brick_pool_test():
    subprocess.check_call(["make", "-C", APPS, "roo_brick_pool_test"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(APPS, "roo_brick_pool_test")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "passed" in out.stdout, out.stdout + out.stderr
