"""The mesh simplification from C++ (include/kangaroo/MarchingCubes.h, VolumeBricks.h over include/kfx_mesh_simplify.h):
roo::MeshSimplify and SaveMeshIndexed(min_faces, largest, nvert, cell) on the three-sphere volume (apps/roo_mesh_simplify_test), and the
applications' --mesh-cell: the PLY holds the counts it prints and is the oracle's simplification of the plain file; the flag is
refused without --mesh-indexed, and by kinectfusion_slabs with more than one rank."""
import os
import re
import subprocess

import numpy as np
import pytest

import kfx_testlib as T

import mesh_components as MC
import mesh_simplify as MS

APPS = os.path.join(T.ROOT, "apps")
pytestmark = pytest.mark.gpu


def _make(target):
    subprocess.check_call(["make", "-C", APPS, target], stdout=subprocess.DEVNULL)


def test_cpp_roo_mesh_simplify_test():
    _make("roo_mesh_simplify_test")
    out = subprocess.run([os.path.join(APPS, "roo_mesh_simplify_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "roo_mesh_simplify_test: ok" in out.stdout, out.stdout + out.stderr


def _ply(prefix):
    raw = open(prefix + ".ply", "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    nv, nt = int(re.search(rb"element vertex (\d+)", head).group(1)), int(re.search(rb"element face (\d+)", head).group(1))
    assert len(body) == 24 * nv + 13 * nt
    table = np.frombuffer(body, "<f4", 6 * nv).reshape(nv, 6)
    rows = np.frombuffer(body, np.dtype([("k", "u1"), ("i", "<u4", 3)]), nt, 24 * nv)
    return table, rows["i"]


def _same_file(prefix, want):
    table, faces = _ply(prefix)
    assert np.array_equal(faces, want[3]) and T.nan_equal(table[:, :3], want[0]) and T.nan_equal(table[:, 3:], want[1])


CELL = "0.0625"   # metres; exactly a float


def test_cpp_headless_mesh_cell_flag(tmp_path):
    _make("kinectfusion_headless")
    exe = os.path.join(APPS, "kinectfusion_headless")
    base = [exe, "--res", "96", "--frames", "3", "--width", "160", "--height", "120"]
    plain, coarse, both = str(tmp_path / "plain"), str(tmp_path / "coarse"), str(tmp_path / "both")
    out = subprocess.run(base + ["--save-mesh", plain, "--mesh-indexed"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    table, faces = _ply(plain)
    out = subprocess.run(base + ["--save-mesh", coarse, "--mesh-indexed", "--mesh-cell", CELL], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"mesh: (\d+) triangles, (\d+) vertices written to (\S+)\.ply", out.stdout)
    assert m and m.group(3) == coarse and "mesh simplification" in out.stdout and "mesh clean-up" not in out.stdout, out.stdout
    want = MS.simplify(table[:, :3], table[:, 3:], None, faces, float(CELL))
    assert 0 < len(want[3]) < len(faces) and (int(m.group(1)), int(m.group(2))) == (len(want[3]), len(want[0]))
    _same_file(coarse, want)
    # with the filter: floaters go first
    out = subprocess.run(base + ["--save-mesh", both, "--mesh-indexed", "--mesh-largest", "--mesh-min-faces", "10", "--mesh-cell", CELL],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mesh clean-up" in out.stdout and "mesh simplification" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    kept = MC.filter_mesh(table[:, :3], table[:, 3:], None, faces, min_faces=10, largest=True)
    _same_file(both, MS.simplify(*kept, float(CELL)))
    # the flag simplifies the indexed mesh: refused without --mesh-indexed, and when it is no length, before any frame runs
    for flags in (["--mesh-cell", CELL], ["--mesh-indexed", "--mesh-cell", "-1"], ["--mesh-indexed", "--mesh-cell", "nan"]):
        out = subprocess.run(base + ["--save-mesh", str(tmp_path / "no")] + flags, capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "--mesh-indexed" in out.stderr and not os.path.exists(str(tmp_path / "no.ply"))


def test_cpp_slabs_mesh_cell_flag_only_with_one_rank(tmp_path):
    """kinectfusion_slabs: with one rank the slab is the whole volume and the cell applies; with more a rank's mesh is welded within the
    rank and the flag is refused with a message that says so"""
    _make("kinectfusion_slabs")
    exe = os.path.join(APPS, "kinectfusion_slabs")
    base = [exe, "--res", "96", "--frames", "3", "--width", "160", "--height", "120", "--raycast", "exact"]
    plain, coarse = str(tmp_path / "plain"), str(tmp_path / "coarse")
    for prefix, flags in ((plain, []), (coarse, ["--mesh-cell", CELL])):
        out = subprocess.run(base + ["--ranks", "1", "--save-mesh", prefix, "--mesh-indexed"] + flags, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and re.search(r"mesh: (\d+) triangles, (\d+) vertices", out.stdout), out.stdout[-2000:] + out.stderr[-2000:]
    table, faces = _ply(plain + ".r0")
    want = MS.simplify(table[:, :3], table[:, 3:], None, faces, float(CELL))
    assert 0 < len(want[3]) < len(faces)
    _same_file(coarse + ".r0", want)
    out = subprocess.run(base + ["--ranks", "2", "--save-mesh", str(tmp_path / "two"), "--mesh-indexed", "--mesh-cell", CELL], capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 2 and "slab boundaries" in out.stderr and not os.path.exists(str(tmp_path / "two.r0.ply"))
    out = subprocess.run(base + ["--ranks", "1", "--save-mesh", str(tmp_path / "no"), "--mesh-cell", CELL], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--mesh-indexed" in out.stderr
