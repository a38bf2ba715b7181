"""The oracle of the mesh clean-up (tests/mesh_components.py) on hand-made meshes with known answers and on the two volumes the GPU
tests use, against the figures worked out for them; and the host-check program (scripts/mesh_clean_host_check.cpp), which builds with a
plain host compiler, plainly and under the address and undefined-behaviour sanitizers, as a stand-alone executable, and passes."""
import os
import subprocess

import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import oracle

import mesh_components as MC
import mesh_weld as W
import test_mesh_cpu as TM


def welded(ovol):
    return W.weld(ovol, *oracle.marching_cubes(ovol, None, *TM.tables()))


@pytest.mark.parametrize("name", sorted(MC.HAND_MADE))
def test_oracle_on_hand_made_meshes(name):
    faces, n, want_vc, want_cf = MC.HAND_MADE[name]
    vc, cf = MC.components(faces, n)
    assert vc.dtype == np.uint32 and cf.dtype == np.uint32
    assert vc.tolist() == want_vc and cf.tolist() == want_cf
    # any order of the faces and any rotation of a face gives the same answer
    f = np.asarray(faces)[::-1, [1, 2, 0]]
    vc2, cf2 = MC.components(f, n)
    assert vc2.tolist() == want_vc and cf2.tolist() == want_cf


def test_oracle_on_strips_and_the_fan():
    for faces, n in (MC.permuted_strip(), MC.descending_strip(), MC.fan()):
        vc, cf = MC.components(faces, n)
        assert not vc.any() and cf.tolist() == [len(faces)]
    # two strips and a fan side by side, ids interleaved: three components in the order of their smallest ids
    a, na = MC.permuted_strip(300, seed=5)
    b, nb = MC.descending_strip(200)
    c, nc = MC.fan(64, hub=9)
    faces = np.concatenate([3 * c.astype(np.int64) + 1, 3 * a.astype(np.int64), 3 * b.astype(np.int64) + 2])
    n = 3 * max(na, nb, nc)
    vc, cf = MC.components(faces, n)
    used = np.zeros(n, bool)
    used[faces.reshape(-1)] = True
    assert cf[:3].tolist() == [300, 64, 200] and not cf[3:].any() and len(cf) == 3 + int((~used).sum())
    assert set(vc[np.arange(0, 3 * na, 3)]) == {0} and set(vc[np.arange(1, 3 * nc, 3)]) == {1} and set(vc[np.arange(2, 3 * nb, 3)]) == {2}


def test_oracle_filter_rules():
    faces, n = np.array([[0, 1, 2], [1, 2, 3], [5, 6, 7], [8, 9, 10], [9, 10, 11], [4, 4, 4]]), 13
    verts = np.arange(3 * n, dtype=np.float32).reshape(n, 3)
    verts[6, 1] = np.nan
    vc, cf = MC.components(faces, n)
    assert cf.tolist() == [2, 1, 1, 2, 0]
    # the identity
    v, nr, c, f = MC.filter_mesh(verts, None, None, faces)
    assert T.nan_equal(v, verts) and nr is None and c is None and np.array_equal(f, faces)
    # min_faces = 1 drops the isolated vertex 12 alone
    v, _, _, f = MC.filter_mesh(verts, None, None, faces, min_faces=1)
    assert T.nan_equal(v, verts[:12]) and np.array_equal(f, faces)
    # min_faces = 2 keeps the two pairs; vertices 8 .. 11 become 4 .. 7
    v, _, _, f = MC.filter_mesh(verts, None, None, faces, min_faces=2)
    assert T.nan_equal(v, verts[[0, 1, 2, 3, 8, 9, 10, 11]]) and f.tolist() == [[0, 1, 2], [1, 2, 3], [4, 5, 6], [5, 6, 7]]
    # largest: a tie goes to the smaller component id; min_faces still applies on top
    v, _, _, f = MC.filter_mesh(verts, None, None, faces, largest=True)
    assert T.nan_equal(v, verts[:4]) and f.tolist() == [[0, 1, 2], [1, 2, 3]]
    v, _, _, f = MC.filter_mesh(verts, None, None, faces, min_faces=3, largest=True)
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_oracle_on_the_three_sphere_volume():
    """48^3, box [-1, 1]^3: V = 2480, T = 4948, three closed components of 132, 2260 and 2556 faces"""
    wv, wn, _, wf = welded(MC.three_spheres(oracle))
    assert (len(wv), len(wf)) == (2480, 4948)
    vc, cf = MC.components(wf, len(wv))
    assert sorted(cf.tolist()) == [132, 2260, 2556]
    parts = MC.split_parts(wf, len(wv))
    assert len(parts) == 3
    for f, nv in parts:
        assert nv == len(f) // 2 + 2 and W.closed_with_euler_2(f, nv)
    v, n, _, f = MC.filter_mesh(wv, wn, None, wf, min_faces=1000)
    assert (len(v), len(f)) == (2412, 4816) and len(n) == 2412
    assert all(W.closed_with_euler_2(pf, pv) for pf, pv in MC.split_parts(f, len(v))) and len(MC.split_parts(f, len(v))) == 2
    v, _, _, f = MC.filter_mesh(wv, wn, None, wf, largest=True)
    assert len(f) == 2556 and len(v) == 2556 // 2 + 2 and W.closed_with_euler_2(f, len(v))
    v, n, _, f = MC.filter_mesh(wv, wn, None, wf)
    assert T.nan_equal(v, wv) and T.nan_equal(n, wn) and np.array_equal(f, wf)


def test_oracle_on_the_ragged_unobserved_volume():
    """21 x 13 x 34 with the NaN lattice: V = 828, T = 983, 13 components of 1 to 227 faces"""
    import test_gpu_mesh_indexed as TI
    ovol, _, _ = TI.f32_case("ragged_unobserved")
    wv, _, _, wf = welded(ovol)
    assert (len(wv), len(wf)) == (828, 983)
    vc, cf = MC.components(wf, len(wv))
    assert len(cf) == 13 and int(cf.min()) == 1 and int(cf.max()) == 227 and int(cf.sum()) == 983
    assert len(MC.filter_mesh(wv, None, None, wf, min_faces=228)[3]) == 0
    for m in (2, 13):
        v, _, _, f = MC.filter_mesh(wv, None, None, wf, min_faces=m)
        assert 0 < len(f) <= 983 and len(f) == int(cf[cf >= m].sum())


def build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + [os.path.join(T.ROOT, "scripts", "mesh_clean_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "mesh_clean_host_check: ok" in out.stdout, out.stdout + out.stderr


def test_the_host_check_program_builds_plainly_and_passes(tmp_path):
    build_and_run(tmp_path, "mesh_clean_host_check", ["-O1"])


def test_the_host_check_program_builds_and_passes_under_the_host_sanitizers(tmp_path):
    build_and_run(tmp_path, "mesh_clean_host_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
