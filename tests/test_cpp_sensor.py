"""roo::DepthInput and roo::BilateralFilterDepth from C++ (include/kangaroo/DepthInput.h over include/kfx_sensor.h): a stream of
16-bit frames through the upload ring against ElementwiseScaleBias<float, unsigned short, float> + BilateralFilter<float, float>
(apps/roo_sensor_test)."""
import os
import subprocess

import pytest

import kfx_testlib as T

APPS = os.path.join(T.ROOT, "apps")
pytestmark = pytest.mark.gpu


def test_cpp_roo_sensor_test():
    subprocess.check_call(["make", "-C", APPS, "roo_sensor_test"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(APPS, "roo_sensor_test")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "passed" in out.stdout, out.stdout + out.stderr
