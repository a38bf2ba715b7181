"""SaveMeshIndexed from C++ (include/kangaroo/MarchingCubes.h, SlabVolume.h over include/kfx_mesh_index.h): the overloads and
SlabVolume::SaveMeshIndexed against the plain calls and SaveMesh's files (apps/roo_mesh_indexed_test), and the headless
application's --save-mesh P --mesh-indexed: the PLY holds the triangle and vertex counts it prints."""
import os
import re
import subprocess

import numpy as np
import pytest

import kfx_testlib as T

APPS = os.path.join(T.ROOT, "apps")
pytestmark = pytest.mark.gpu


def _make(target):
    subprocess.check_call(["make", "-C", APPS, target], stdout=subprocess.DEVNULL)


def test_cpp_roo_mesh_indexed_test():
    _make("roo_mesh_indexed_test")
    out = subprocess.run([os.path.join(APPS, "roo_mesh_indexed_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "passed" in out.stdout, out.stdout + out.stderr


def test_cpp_headless_save_mesh_indexed(tmp_path):
    _make("kinectfusion_headless")
    prefix = str(tmp_path / "model")
    out = subprocess.run([os.path.join(APPS, "kinectfusion_headless"), "--res", "96", "--frames", "3", "--width", "160", "--height", "120",
                          "--save-mesh", prefix, "--mesh-indexed"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"mesh: (\d+) triangles, (\d+) vertices written to (\S+)\.ply", out.stdout)
    assert m and m.group(3) == prefix, out.stdout
    nt, nv = int(m.group(1)), int(m.group(2))
    raw = open(prefix + ".ply", "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert int(re.search(rb"element vertex (\d+)", head).group(1)) == nv and int(re.search(rb"element face (\d+)", head).group(1)) == nt
    assert nt > 1000 and nv < nt and len(body) == 24 * nv + 13 * nt
    rows = np.frombuffer(body, np.dtype([("k", "u1"), ("i", "<u4", 3)]), nt, 24 * nv)
    assert (rows["k"] == 3).all() and rows["i"].max() == nv - 1 and len(np.unique(rows["i"])) == nv
    assert np.isfinite(np.frombuffer(body, "<f4", 6 * nv)).all()
