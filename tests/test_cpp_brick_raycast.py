"""roo::RaycastBricksPlan / RaycastSdfBricks from C++ (include/kangaroo/VolumeBricks.h over include/kfx_raycast_bricks.h): a small volume
is packed, its bricks are rendered, the volume is rendered, and the images are compared bit for bit (apps/roo_brick_raycast_test).  The
driver compiles against the headers without a device; running it needs one."""
import os
import subprocess

import pytest

import kfx_testlib as T

APPS = os.path.join(T.ROOT, "apps")


def test_cpp_roo_brick_raycast_test_compiles(tmp_path):
    """host code only: the headers' overloads resolve and the driver links against libkfx.so"""
    exe = str(tmp_path / "roo_brick_raycast_test")
    rocm = os.environ.get("ROCM", "/opt/rocm")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(T.ROOT, "include"),
                           "-I" + os.path.join(rocm, "include"), "-Wall", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-maybe-uninitialized",
                           os.path.join(APPS, "roo_brick_raycast_test.cpp"), "-o", exe, "-L" + os.path.join(T.ROOT, "kangaroo_amd"), "-lkfx",
                           "-Wl,-rpath," + os.path.join(T.ROOT, "kangaroo_amd")])
    assert os.path.getsize(exe) > 0


@pytest.mark.gpu
def test_cpp_roo_brick_raycast_test():
    subprocess.check_call(["make", "-C", APPS, "roo_brick_raycast_test"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(APPS, "roo_brick_raycast_test")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "passed" in out.stdout, out.stdout + out.stderr
