"""The mesh clean-up from C++ (include/kangaroo/MarchingCubes.h, VolumeBricks.h, SlabVolume.h over include/kfx_mesh_clean.h):
roo::MeshComponents, roo::MeshFilter and SaveMeshIndexed(min_faces, largest) on the three-sphere volume (apps/roo_mesh_clean_test), and
the headless application's --mesh-min-faces / --mesh-largest: the PLY holds the counts it prints, fewer than the unfiltered file's, and
the flags are refused without --mesh-indexed."""
import os
import re
import subprocess

import numpy as np
import pytest

import kfx_testlib as T

import mesh_components as MC

APPS = os.path.join(T.ROOT, "apps")
pytestmark = pytest.mark.gpu


def _make(target):
    subprocess.check_call(["make", "-C", APPS, target], stdout=subprocess.DEVNULL)


def test_cpp_roo_mesh_clean_test():
    _make("roo_mesh_clean_test")
    out = subprocess.run([os.path.join(APPS, "roo_mesh_clean_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "roo_mesh_clean_test: ok" in out.stdout, out.stdout + out.stderr


def _ply(prefix):
    raw = open(prefix + ".ply", "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    nv, nt = int(re.search(rb"element vertex (\d+)", head).group(1)), int(re.search(rb"element face (\d+)", head).group(1))
    assert len(body) == 24 * nv + 13 * nt
    table = np.frombuffer(body, "<f4", 6 * nv).reshape(nv, 6)
    rows = np.frombuffer(body, np.dtype([("k", "u1"), ("i", "<u4", 3)]), nt, 24 * nv)
    return table, rows["i"]


def test_cpp_headless_mesh_clean_flags(tmp_path):
    _make("kinectfusion_headless")
    exe = os.path.join(APPS, "kinectfusion_headless")
    base = [exe, "--res", "96", "--frames", "3", "--width", "160", "--height", "120"]
    plain, largest = str(tmp_path / "plain"), str(tmp_path / "largest")
    out = subprocess.run(base + ["--save-mesh", plain, "--mesh-indexed"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    table, faces = _ply(plain)
    out = subprocess.run(base + ["--save-mesh", largest, "--mesh-indexed", "--mesh-largest", "--mesh-min-faces", "10"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"mesh: (\d+) triangles, (\d+) vertices written to (\S+)\.ply", out.stdout)
    assert m and m.group(3) == largest and "mesh clean-up" in out.stdout, out.stdout
    got_table, got_faces = _ply(largest)
    assert (int(m.group(1)), int(m.group(2))) == (len(got_faces), len(got_table))
    # the oracle's filter of the unfiltered file is the filtered file
    wv, wn, _, wf = MC.filter_mesh(table[:, :3], table[:, 3:], None, faces, min_faces=10, largest=True)
    assert 0 < len(wf) <= len(faces) and np.array_equal(got_faces, wf)
    assert T.nan_equal(got_table[:, :3], wv) and T.nan_equal(got_table[:, 3:], wn)
    # the flags filter the indexed mesh: refused without --mesh-indexed, before any frame runs
    for flags in (["--mesh-largest"], ["--mesh-min-faces", "10"]):
        out = subprocess.run(base + ["--save-mesh", str(tmp_path / "no")] + flags, capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "--mesh-indexed" in out.stderr and not os.path.exists(str(tmp_path / "no.ply"))


def test_cpp_slabs_mesh_clean_flags_only_with_one_rank(tmp_path):
    """kinectfusion_slabs: with one rank the slab is the whole volume and the filter applies; with more a rank's mesh is welded within
    the rank, its components are cut at the slab boundaries, and the flags are refused with a message that says so"""
    _make("kinectfusion_slabs")
    exe = os.path.join(APPS, "kinectfusion_slabs")
    base = [exe, "--res", "96", "--frames", "3", "--width", "160", "--height", "120", "--raycast", "exact"]
    plain, largest = str(tmp_path / "plain"), str(tmp_path / "largest")
    for prefix, flags in ((plain, []), (largest, ["--mesh-largest", "--mesh-min-faces", "10"])):
        out = subprocess.run(base + ["--ranks", "1", "--save-mesh", prefix, "--mesh-indexed"] + flags, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and re.search(r"mesh: (\d+) triangles, (\d+) vertices", out.stdout), out.stdout[-2000:] + out.stderr[-2000:]
    table, faces = _ply(plain + ".r0")
    got_table, got_faces = _ply(largest + ".r0")
    wv, wn, _, wf = MC.filter_mesh(table[:, :3], table[:, 3:], None, faces, min_faces=10, largest=True)
    assert 0 < len(wf) <= len(faces) and np.array_equal(got_faces, wf)
    assert T.nan_equal(got_table[:, :3], wv) and T.nan_equal(got_table[:, 3:], wn)
    out = subprocess.run(base + ["--ranks", "2", "--save-mesh", str(tmp_path / "two"), "--mesh-indexed", "--mesh-largest"], capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 2 and "slab boundaries" in out.stderr and not os.path.exists(str(tmp_path / "two.r0.ply"))
    out = subprocess.run(base + ["--ranks", "1", "--save-mesh", str(tmp_path / "no"), "--mesh-largest"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--mesh-indexed" in out.stderr
