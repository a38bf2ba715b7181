"""roo::VolumeShift from C++ (include/kangaroo/VolumeShift.h over include/kfx_shift.h): BoundedVolume<SDF_t>, <SDF_h> and <float>
shifted on the device against a loop on the host, and the bbox moved with them (apps/roo_shift_test)."""
import os
import subprocess

import pytest

import kfx_testlib as T

APPS = os.path.join(T.ROOT, "apps")
pytestmark = pytest.mark.gpu


def test_cpp_roo_shift_test():
    subprocess.check_call(["make", "-C", APPS, "roo_shift_test"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(APPS, "roo_shift_test")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "passed" in out.stdout, out.stdout + out.stderr
