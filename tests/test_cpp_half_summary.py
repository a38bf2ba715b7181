"""apps/roo_half_summary_test: the C++ overloads of include/kangaroo/SdfSummary.h on BoundedVolume<SDF_h> (config C5) -- tracked
SdfReset / SdfFuse / RaycastSdf / RaycastSdfLevels give the volume and the images of the plain SDF_h calls, bit for bit."""
import os
import subprocess

import pytest

import kfx_testlib as T

APPS = os.path.join(T.ROOT, "apps")


@pytest.mark.gpu
def test_cpp_half_summary_overloads_match_the_plain_calls():
    subprocess.check_call(["make", "-C", APPS, "roo_half_summary_test"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(APPS, "roo_half_summary_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "passed" in out.stdout, out.stdout + out.stderr
