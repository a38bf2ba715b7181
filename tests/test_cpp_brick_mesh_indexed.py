"""roo::MeshBricksIndexPlan / MeshBricksEmitIndexed / SaveMeshBricksIndexed from C++ (include/kangaroo/VolumeBricks.h over
include/kfx_mesh_bricks_index.h): a small ragged volume is packed, its bricks are meshed as a soup and as an indexed mesh, and the
indexed mesh is compared with a host-side weld of the soup (apps/roo_brick_mesh_indexed_test)."""
import os
import subprocess

import pytest

import kfx_testlib as T

APPS = os.path.join(T.ROOT, "apps")
pytestmark = pytest.mark.gpu


def test_cpp_roo_brick_mesh_indexed_test():
    subprocess.check_call(["make", "-C", APPS, "roo_brick_mesh_indexed_test"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(APPS, "roo_brick_mesh_indexed_test")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "passed" in out.stdout, out.stdout + out.stderr
