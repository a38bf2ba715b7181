"""The numpy oracle of the mesh smoothing (tests/mesh_smooth.py, the contract of include/kfx_mesh_smooth.h) on hand-made cases with the
answers written out; the host-check program (scripts/mesh_smooth_host_check.cpp), which runs the templates of mesh_smooth_host.h on plain
arrays, plainly and under the address and undefined-behaviour sanitizers; and properties of the oracle alone on a sphere's indexed mesh,
stated as comparisons.  No GPU, nothing of the library."""
import os
import subprocess

import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import oracle

import mesh_smooth as SM
import mesh_weld as W
import test_mesh_cpu as TM

CENTRE, RADIUS = (0.05, -0.02, 0.03), 0.7   # of TM.sphere_volume


@pytest.mark.parametrize("name", sorted(SM.HAND_MADE))
def test_oracle_gives_the_written_answer(name):
    verts, faces, case = SM.hand_made(name)
    start, inc, flags = SM.adjacency(len(verts), faces)
    assert start.dtype == inc.dtype == flags.dtype == np.uint32
    assert start.tolist() == case["inc_start"] and inc.tolist() == case["inc"] and flags.tolist() == case["flags"]
    got = SM.smooth(verts, faces, iterations=1, lam=0.5, mu=0.0, pin_mask=0)
    want = np.asarray(case["smooth"], np.float32)
    assert got.dtype == np.float32 and T.nan_equal(got, want), (got, want)
    normals = SM.vertex_normals(verts, faces)
    assert normals.dtype == np.float32 and not np.isnan(normals).any()
    for v, n in case["normals"].items():
        assert np.array_equal(normals[v], np.asarray(n, np.float32)), (v, normals[v])
    # no flagged vertex moves when every flag pins, and nothing with no iteration; a row that stays is the input's words
    pinned = SM.smooth(verts, faces, iterations=3, pin_mask=0xf)
    assert np.array_equal(pinned[flags != 0].view(np.uint32), verts[flags != 0].view(np.uint32))
    assert np.array_equal(SM.smooth(verts, faces, iterations=0).view(np.uint32), verts.view(np.uint32))


def test_a_nan_does_not_travel():
    verts, faces, case = SM.hand_made("nan_vertex")
    out = SM.smooth(verts, faces, iterations=4)
    assert np.array_equal(out.view(np.uint32), verts.view(np.uint32))
    # ... and a vertex that does not read it moves as if it were not there
    more = np.concatenate([verts, [[2, 0, 0], [2, 1, 0], [3, 1, 0]]]).astype(np.float32)
    faces = np.concatenate([faces, [[4, 5, 6]]]).astype(np.uint32)
    out = SM.smooth(more, faces, iterations=1, mu=0.0)
    assert np.array_equal(out[:4].view(np.uint32), verts.view(np.uint32)) and not np.isnan(out[4:]).any() and (out[4:] != more[4:]).any()


def test_random_meshes_sum_in_the_order_of_the_lists():
    """the vectorised rank-by-rank sum against a plain loop over every vertex's entries"""
    verts, faces = SM.random_mesh(257, 400, 11)
    start, inc, flags = SM.adjacency(257, faces)
    f = faces.astype(np.int64)
    assert np.array_equal(np.sort(inc), np.arange(1200)) and start[0] == 0 and start[-1] == 1200
    got = SM.smooth(verts, faces, iterations=1, lam=0.5, mu=0.0)
    for v in range(257):
        seg = inc[start[v]:start[v + 1]].astype(np.int64)
        assert (np.diff(seg) > 0).all() and (f.reshape(-1)[seg] == v).all()
        if len(seg) == 0:
            assert flags[v] == SM.ISOLATED and np.array_equal(got[v], verts[v])
            continue
        acc = np.zeros(3, np.float32)
        for s in seg:
            face, c = s // 3, s % 3
            acc = acc + verts[f[face, (c + 1) % 3]]
            acc = acc + verts[f[face, (c + 2) % 3]]
        want = verts[v] + np.float32(0.5) * (acc / np.float32(2 * len(seg)) - verts[v])
        assert want.dtype == np.float32 and np.array_equal(got[v], want), v


def build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags
                          + [os.path.join(T.ROOT, "scripts", "mesh_smooth_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "mesh_smooth_host_check: ok" in out.stdout, out.stdout + out.stderr


def test_the_host_check_program_builds_plainly_and_passes(tmp_path):
    build_and_run(tmp_path, "mesh_smooth_host_check", ["-O1"])


def test_the_host_check_program_builds_and_passes_under_the_host_sanitizers(tmp_path):
    build_and_run(tmp_path, "mesh_smooth_host_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


@pytest.fixture(scope="module")
def sphere():
    """the oracle's indexed mesh of a single SdfSphere volume at 32^3: (verts, norms, faces)"""
    ovol = TM.sphere_volume(32, RADIUS)
    v, n, c, f = W.weld(ovol, *oracle.marching_cubes(ovol, None, *TM.tables()))
    assert c is None and len(f) > 1000
    return v, n, f


def radius(verts):
    d = verts.astype(np.float64) - np.asarray(CENTRE)
    return np.sqrt((d * d).sum(axis=1))


def test_every_recomputed_normal_of_the_sphere_agrees_with_the_extractions(sphere):
    """the sign the header states, e1 x e2: every vertex of this sphere's mesh, without exception"""
    v, n, f = sphere
    got = SM.vertex_normals(v, f)
    assert ((got * n).sum(axis=1) > 0).all()
    assert ((got * (v - np.asarray(CENTRE, np.float32))).sum(axis=1) > 0).all()   # outwards


def test_smoothing_lowers_the_noise_with_each_iteration_count(sphere):
    v, n, f = sphere
    noisy = (v + np.random.RandomState(5).normal(0, 0.01, v.shape)).astype(np.float32)
    adj = SM.adjacency(len(v), f)
    assert not adj[2].any()   # closed and manifold
    spread = [radius(noisy).std()] + [radius(SM.smooth(noisy, f, iterations=k, adj=adj)).std() for k in (1, 5, 10)]
    assert spread[0] > spread[1] > spread[2] > spread[3]
    # Taubin's second pass holds the volume: the mean radius moves less than under plain Laplacian smoothing of equal lambda and count
    r0 = radius(noisy).mean()
    taubin = abs(radius(SM.smooth(noisy, f, iterations=10, lam=0.5, mu=-0.53, adj=adj)).mean() - r0)
    laplace = abs(radius(SM.smooth(noisy, f, iterations=10, lam=0.5, mu=0.0, adj=adj)).mean() - r0)
    assert taubin < laplace


def test_pinned_boundary_vertices_of_an_open_cap_keep_their_bits(sphere):
    v, n, f = sphere
    noisy = (v + np.random.RandomState(6).normal(0, 0.01, v.shape)).astype(np.float32)
    cap = f[(v[f.astype(np.int64)][:, :, 2] > 0.3).all(axis=1)]   # the faces above z = 0.3; the vertices below become isolated
    start, inc, flags = SM.adjacency(len(v), cap)
    rim = (flags & SM.BOUNDARY) != 0
    inner = flags == 0
    assert rim.sum() > 20 and inner.sum() > 100 and ((flags & SM.ISOLATED) != 0).sum() > 100
    out = SM.smooth(noisy, cap, iterations=5, pin_mask=SM.BOUNDARY)
    assert np.array_equal(out[rim].view(np.uint32), noisy[rim].view(np.uint32))
    assert (out[inner] != noisy[inner]).any(axis=1).all()
    free = SM.smooth(noisy, cap, iterations=5, pin_mask=0)
    assert (free[rim] != noisy[rim]).any(axis=1).all()
