"""The mesh smoothing from C++ (include/kangaroo/MarchingCubes.h, VolumeBricks.h over include/kfx_mesh_smooth.h): roo::MeshAdjacency,
MeshSmooth, MeshVertexNormals and SaveMeshIndexed(min_faces, largest, nvert, cell, smooth_iterations) on the three-sphere volume
(apps/roo_mesh_smooth_test), and the applications' --mesh-smooth: the PLY holds the counts it prints and is the oracle's smoothing of the
plain file; the flag is refused without --mesh-indexed, and by kinectfusion_slabs with more than one rank."""
import os
import re
import subprocess

import numpy as np
import pytest

import kfx_testlib as T

import mesh_components as MC
import mesh_simplify as MS
import mesh_smooth as SM

APPS = os.path.join(T.ROOT, "apps")
pytestmark = pytest.mark.gpu


def _make(target):
    subprocess.check_call(["make", "-C", APPS, target], stdout=subprocess.DEVNULL)


def test_cpp_roo_mesh_smooth_test():
    _make("roo_mesh_smooth_test")
    out = subprocess.run([os.path.join(APPS, "roo_mesh_smooth_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "roo_mesh_smooth_test: ok" in out.stdout, out.stdout + out.stderr


def _ply(prefix):
    raw = open(prefix + ".ply", "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    nv, nt = int(re.search(rb"element vertex (\d+)", head).group(1)), int(re.search(rb"element face (\d+)", head).group(1))
    assert len(body) == 24 * nv + 13 * nt
    table = np.frombuffer(body, "<f4", 6 * nv).reshape(nv, 6)
    rows = np.frombuffer(body, np.dtype([("k", "u1"), ("i", "<u4", 3)]), nt, 24 * nv)
    return table, rows["i"]


def smoothed(verts, faces, iterations):
    """the oracle's (verts, norms, faces) after --mesh-smooth N: Taubin's defaults, the boundary pinned, the normals recomputed"""
    adj = SM.adjacency(len(verts), faces)
    out = SM.smooth(verts, faces, iterations=iterations, pin_mask=SM.BOUNDARY, adj=adj)
    return out, SM.vertex_normals(out, faces, adj=adj), faces


def _same_file(prefix, want):
    table, faces = _ply(prefix)
    assert np.array_equal(faces, want[2])
    assert np.array_equal(np.ascontiguousarray(table[:, :3]).view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(np.ascontiguousarray(table[:, 3:]).view(np.uint32), want[1].view(np.uint32))


CELL = "0.0625"   # metres; exactly a float


def test_cpp_headless_mesh_smooth_flag(tmp_path):
    _make("kinectfusion_headless")
    exe = os.path.join(APPS, "kinectfusion_headless")
    base = [exe, "--res", "96", "--frames", "3", "--width", "160", "--height", "120"]
    plain, smooth, all3 = str(tmp_path / "plain"), str(tmp_path / "smooth"), str(tmp_path / "all3")
    out = subprocess.run(base + ["--save-mesh", plain, "--mesh-indexed"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    table, faces = _ply(plain)
    out = subprocess.run(base + ["--save-mesh", smooth, "--mesh-indexed", "--mesh-smooth", "3"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"mesh: (\d+) triangles, (\d+) vertices written to (\S+)\.ply", out.stdout)
    assert m and m.group(3) == smooth and "mesh smoothing: 3" in out.stdout and "mesh clean-up" not in out.stdout, out.stdout
    assert (int(m.group(1)), int(m.group(2))) == (len(faces), len(table))
    want = smoothed(np.ascontiguousarray(table[:, :3]), faces, 3)
    assert (want[0] != table[:, :3]).any()
    _same_file(smooth, want)
    # with the filter and the cell: smoothing goes last
    out = subprocess.run(base + ["--save-mesh", all3, "--mesh-indexed", "--mesh-largest", "--mesh-min-faces", "10", "--mesh-cell", CELL, "--mesh-smooth", "2"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mesh clean-up" in out.stdout and "mesh simplification" in out.stdout and "mesh smoothing" in out.stdout, \
        out.stdout[-2000:] + out.stderr[-2000:]
    kept = MC.filter_mesh(table[:, :3], table[:, 3:], None, faces, min_faces=10, largest=True)
    coarse = MS.simplify(*kept, float(CELL))
    _same_file(all3, smoothed(coarse[0], coarse[3], 2))
    # the flag smooths the indexed mesh: refused without --mesh-indexed, and when it is no count, before any frame runs
    for flags in (["--mesh-smooth", "3"], ["--mesh-indexed", "--mesh-smooth", "-1"]):
        out = subprocess.run(base + ["--save-mesh", str(tmp_path / "no")] + flags, capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "--mesh-indexed" in out.stderr and not os.path.exists(str(tmp_path / "no.ply"))


def test_cpp_slabs_mesh_smooth_flag_only_with_one_rank(tmp_path):
    """kinectfusion_slabs: with one rank the slab is the whole volume and the smoothing applies; with more a rank's mesh is welded within
    the rank and the flag is refused with a message that says so"""
    _make("kinectfusion_slabs")
    exe = os.path.join(APPS, "kinectfusion_slabs")
    base = [exe, "--res", "96", "--frames", "3", "--width", "160", "--height", "120", "--raycast", "exact"]
    plain, smooth = str(tmp_path / "plain"), str(tmp_path / "smooth")
    for prefix, flags in ((plain, []), (smooth, ["--mesh-smooth", "3"])):
        out = subprocess.run(base + ["--ranks", "1", "--save-mesh", prefix, "--mesh-indexed"] + flags, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and re.search(r"mesh: (\d+) triangles, (\d+) vertices", out.stdout), out.stdout[-2000:] + out.stderr[-2000:]
    table, faces = _ply(plain + ".r0")
    _same_file(smooth + ".r0", smoothed(np.ascontiguousarray(table[:, :3]), faces, 3))
    out = subprocess.run(base + ["--ranks", "2", "--save-mesh", str(tmp_path / "two"), "--mesh-indexed", "--mesh-smooth", "3"], capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 2 and "slab boundaries" in out.stderr and not os.path.exists(str(tmp_path / "two.r0.ply"))
    out = subprocess.run(base + ["--ranks", "1", "--save-mesh", str(tmp_path / "no"), "--mesh-smooth", "3"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--mesh-indexed" in out.stderr
