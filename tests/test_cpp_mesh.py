"""SaveMesh from C++ (include/kangaroo/MarchingCubes.h, SlabVolume.h over include/kfx_mesh.h): the half-cell overloads and
SlabVolume::SaveMesh against the plain calls (apps/roo_mesh_test), and the applications' --save-mesh: the slab application's
per-rank PLYs hold the one-rank run's triangles, the headless application's PLY the face count it prints."""
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


def ply_triangles(path):
    """(faces, 18) uint32: x y z nx ny nz of a triangle's three vertices, from a binary PLY this library wrote (no colour)."""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    nv = int(re.search(rb"element vertex (\d+)", head).group(1))
    nf = int(re.search(rb"element face (\d+)", head).group(1))
    assert nv == 3 * nf and b"property float alpha" not in head
    return np.frombuffer(body[:nv * 24], dtype="<u4").reshape(nf, 18), nf


def test_cpp_roo_mesh_test():
    _make("roo_mesh_test")
    out = subprocess.run([os.path.join(APPS, "roo_mesh_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "passed" in out.stdout, out.stdout + out.stderr


def test_cpp_slabs_save_mesh_ranks_partition_the_one_rank_mesh(tmp_path):
    _make("kinectfusion_slabs")
    common = ["--res", "96", "--frames", "3", "--width", "160", "--height", "120", "--halo", "exchange"]
    for ranks in (1, 4):
        out = subprocess.run([os.path.join(APPS, "kinectfusion_slabs"), "--ranks", str(ranks), "--save-mesh", str(tmp_path / ("m%d" % ranks))] + common,
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "mesh: " in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    one, n1 = ply_triangles(str(tmp_path / "m1.r0.ply"))
    parts = [ply_triangles(str(tmp_path / ("m4.r%d.ply" % r))) for r in range(4)]
    four = np.concatenate([p for p, _ in parts])
    assert n1 > 1000 and min(n for _, n in parts) > 0
    key = lambda a: a[np.lexsort(a.T[::-1])]
    assert four.shape == one.shape and np.array_equal(key(four), key(one))


def test_cpp_headless_save_mesh(tmp_path):
    _make("kinectfusion_headless")
    prefix = str(tmp_path / "model")
    out = subprocess.run([os.path.join(APPS, "kinectfusion_headless"), "--res", "96", "--frames", "3", "--width", "160", "--height", "120",
                          "--save-mesh", prefix], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"mesh: (\d+) triangles written to (\S+)\.ply", out.stdout)
    assert m and m.group(2) == prefix, out.stdout
    tris, nf = ply_triangles(prefix + ".ply")
    assert nf == int(m.group(1)) > 1000 and np.isfinite(tris.view(np.float32)).all()
