"""Indexed mesh extraction (include/kfx_mesh_index.h: kfx_mesh_index_plan / kfx_mesh_emit_indexed) against the weld of the ORACLE's
soup by lattice edge (tests/mesh_weld.py) -- never against the library's own soup: vertices, normals, colours and faces bit for bit
on fp32 and half cells, whole volumes and Z-slab views, grey and colour; the SlabPipeline's ranks; the PLY file; and 2048^3 half
cells (cube indices beyond 2^32) checked on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import oracle, scenes

import mesh_weld as W
import test_gpu_mesh_volumes as TV
import test_mesh_cpu as TM

pytestmark = pytest.mark.gpu


def upload(roo, ovol, kind="f32", pitch=None):
    vol = roo.BoundedVolume(ovol.w, ovol.h, ovol.d, ovol.boxmin, ovol.boxmax, pitch=pitch, kind=kind)
    vol.MemcpyFromHost(ovol.data)
    return vol


def expected(ovol, ocvol=None, z_range=None, soup=None):
    soup = soup or oracle.marching_cubes(ovol, ocvol, *TM.tables())
    return W.weld(ovol, *soup, z_range=z_range)


def check(got, want, what=""):
    v, n, c, f = got
    wv, wn, wc, wf = want
    assert len(wf) > 100 and len(wv) < 3 * len(wf)
    assert tuple(f.shape) == wf.shape and np.array_equal(f.cpu().numpy().view(np.uint32), wf), what
    assert T.nan_equal(v.cpu().numpy(), wv) and T.nan_equal(n.cpu().numpy(), wn), what
    assert (c is None) == (wc is None), what
    if wc is not None:
        assert T.nan_equal(c.cpu().numpy(), wc), what


def f32_case(case):
    """the oracle volumes of test_gpu_mesh_volumes.volume_case"""
    import test_color_cpu as TC
    ocvol, pitch = None, None
    if case == "sphere":
        ovol = TM.sphere_volume(48, 0.7)
    elif case == "fused_room_colour":
        ovol, ocvol, K, Kimg, tr, near, far, inputs = TC.color_setup(0, 160, 120, 160, 120, dims=(64, 64, 64))
        for fr in inputs:
            oracle.sdf_fuse_color(ovol, ocvol, fr["f"], fr["nrm"], fr["T_cw"], K, fr["rgb"], fr["T_iw"], Kimg, tr, 1000.0, 0.1, nthreads=0)
    else:
        pitch = 21 * 8 + 40
        ovol = oracle.Volume(21, 13, 34, (-1, -0.5, -1), (1, 0.7, 1.5), pitch_bytes=pitch)
        oracle.sdf_sphere(ovol, (0.1, 0.0, 0.2), 0.45)
        ovol.data[:, :, :, 0][(np.add.outer(np.add.outer(np.arange(34), np.arange(13)), np.arange(21)) % 7) == 0] = np.nan
    return ovol, ocvol, pitch


@pytest.mark.parametrize("case", ["sphere", "ragged_unobserved", "fused_room_colour"])
def test_gpu_indexed_mesh_f32_equals_the_welded_oracle_soup(roo, case):
    """a) sphere 48^3; b) 21x13x34 with the NaN lattice and a padded pitch: ragged extents, skipped cubes, ownership passing to a later
    cube; c) the fused room with colour at 64^3."""
    from kangaroo_amd import mesh
    ovol, ocvol, pitch = f32_case(case)
    vol = upload(roo, ovol, pitch=pitch)
    cvol = upload(roo, ocvol, kind="c32") if ocvol is not None else None
    want = expected(ovol, ocvol)
    got = mesh.ExtractMesh(vol, cvol, indexed=True)
    check(got, want, case)
    if case == "sphere":
        assert len(want[0]) == len(want[3]) // 2 + 2 and W.closed_with_euler_2(want[3], len(want[0]))
    # the soup path is untouched by the indexed call
    sv, sn, sc = mesh.ExtractMesh(vol, cvol)
    ov, on, oc = oracle.marching_cubes(ovol, ocvol, *TM.tables())
    assert T.nan_equal(sv.cpu().numpy(), ov) and T.nan_equal(sn.cpu().numpy(), on)


def test_gpu_indexed_mesh_half_cells_equal_the_welded_oracle_soup_of_the_widened_volume(roo):
    """d) half cells, room, 80x64x72 with the %11 NaN lattice and pitch 80*4 + 52: columns span two 64-cube segments (d = 72), rows two
    64-lane groups (w = 80)."""
    from kangaroo_amd import mesh
    dims, pitch = (80, 64, 72), 80 * 4 + 52
    bmin, bmax, near, far = scenes.SCENES["room"]
    w, h = 160, 120
    K = scenes.intrinsics(w, h)
    tr = scenes.trunc_dist(bmin, bmax, dims)
    ovh = oracle.VolumeH(*dims, bmin, bmax, pitch_bytes=pitch)
    oracle.sdf_reset(ovh, float("nan"))
    for i in range(3):
        T_wc = scenes.orbit_pose(i, 8)
        f, vbo, nrm = T.preprocess_oracle(scenes.render_depth("room", w, h, T_wc, K), K)
        oracle.sdf_fuse(ovh, f, nrm, scenes.se3_inverse(T_wc), K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, nthreads=0)
    ovh.data[:, :, :, 0][(np.add.outer(np.add.outer(np.arange(dims[2]), np.arange(dims[1])), np.arange(dims[0])) % 11) == 0] = np.nan
    vol = upload(roo, ovh, kind="f16", pitch=pitch)
    assert T.nan_equal(vol.MemcpyToHost(), ovh.data)
    want = expected(TV.widened(ovh))
    assert len(want[3]) > 1000
    check(mesh.ExtractMesh(vol, indexed=True), want)


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_gpu_indexed_mesh_slab_views_weld_each_ranks_part(roo, kind):
    """e) 70x60x88 sphere with the %13 NaN lattice, worlds 2 and 3, ghost 2: every rank's indexed mesh is the weld of that rank's part
    of the whole volume's oracle soup; a ghost of 1 is refused with KFX_E_RANGE before any launch."""
    from kangaroo_amd import _lib, mesh
    D = 88
    bmin, bmax = (-1.0, -0.8, -1.1), (1.0, 0.9, 1.2)
    vol = roo.BoundedVolume(70, 60, D, bmin, bmax, kind=kind)
    roo.SdfSphere(vol, (0.1, -0.05, 0.15), 0.8)
    t = vol.tensor()
    t[..., 0][(TV.torch_arange3(t.shape[:3]) % 13) == 0] = float("nan")
    ovol = oracle.Volume(70, 60, D, bmin, bmax)
    ovol.data[...] = vol.MemcpyToHost().astype(np.float32)
    soup = oracle.marching_cubes(ovol, None, *TM.tables())
    seen = 0
    for world in (2, 3):
        for z0, z1, s0, s1 in TV.slab_bounds(D, world, 2):
            want = expected(ovol, z_range=(z0, min(z1, D - 1)), soup=soup)
            got = mesh.ExtractMesh(vol.ZSlab(s0, s1), slab=(D, s0, bmin[2], bmax[2], z0, z1), indexed=True)
            check(got, want, (world, z0, z1))
            seen += len(want[3])
    assert seen == 2 * len(soup[0]) // 3
    z0, z1, s0, s1 = list(TV.slab_bounds(D, 3, 1))[1]
    with pytest.raises(_lib.KfxError) as e:
        mesh.ExtractMesh(vol.ZSlab(s0, s1), slab=(D, s0, bmin[2], bmax[2], z0, z1), indexed=True)
    assert e.value.code == -4


def test_gpu_slab_pipeline_rank_meshes_indexed(tmp_path):
    """SlabPipeline.ExtractMesh / SaveMesh(indexed=True) on three ranks: each rank's indexed mesh is the weld of its own soup."""
    world = 3
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(TV._free_port()), os.path.join(T.ROOT, "tests", "mp_slab_mesh_indexed_gpu.py"), str(tmp_path / "m")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=T.ROOT)
    assert out.returncode == 0 and out.stdout.count("MESH_OK") == world, out.stdout[-3000:] + out.stderr[-3000:]


def test_gpu_indexed_mesh_refuses_totals_that_are_not_the_plans(roo):
    """kfx_mesh_index_plan reads the plan's totals back from the scratch, kfx_mesh_emit_indexed the index plan's totals and vertex
    count: others are refused with KFX_E_RANGE, and nothing is written."""
    import ctypes as C
    import torch
    from kangaroo_amd import _lib
    L = _lib.load()
    vol = upload(roo, TM.sphere_volume(24, 0.7))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    nbytes = L.kfx_mesh_scratch_bytes(vol.ref(), 0, None, 0, 0)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    totals = (C.c_ulonglong * 2)()
    _lib.check(L.kfx_mesh_plan(vol.ref(), 0, None, 0, 0, ptr(scratch), nbytes, totals, None))
    na, nt = int(totals[0]), int(totals[1])
    xbytes = L.kfx_mesh_index_scratch_bytes(vol.ref(), 0, None, 0, 0, totals)
    xscratch = torch.empty(xbytes, dtype=torch.uint8, device="cuda")
    nv = C.c_ulonglong(0)
    for wrong in ((na - 1, nt), (na, nt - 1)):
        bad = (C.c_ulonglong * 2)(*wrong)
        assert L.kfx_mesh_index_plan(vol.ref(), 0, None, 0, 0, ptr(scratch), nbytes, bad, ptr(xscratch), xbytes, C.byref(nv), None) == -4
    _lib.check(L.kfx_mesh_index_plan(vol.ref(), 0, None, 0, 0, ptr(scratch), nbytes, totals, ptr(xscratch), xbytes, C.byref(nv), None))
    V = int(nv.value)
    assert 0 < V < 3 * nt
    out = torch.full((3 * nt, 3), -7.0, dtype=torch.float32, device="cuda")
    faces = torch.full((nt, 3), -7, dtype=torch.int32, device="cuda")
    emit = lambda tot, n: L.kfx_mesh_emit_indexed(vol.ref(), 0, None, 0, 0, None, ptr(xscratch), xbytes, tot, n, ptr(out), ptr(out), None, ptr(faces), None)
    assert emit(totals, V - 1) == -4 and emit(totals, V + 1) == -4
    assert emit((C.c_ulonglong * 2)(na, nt - 1), V) == -4
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((faces == -7).all())
    assert emit(totals, V) == 0
    torch.cuda.synchronize()
    assert int(faces.max()) == V - 1 and int(faces.min()) == 0


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_gpu_mesh_colours_are_written_only_when_asked_for(roo, kind):
    """kfx_mesh_emit and kfx_mesh_emit_indexed with a `colors` buffer but no colour volume to sample -- colorvol null, or (whole
    volume) one that is not IsValid(), 24 x 20 x 7 -- on a 24 x 20 x 28 sphere, whole and as the upper of two slab views with a ghost of
    two planes (there a colour slab must have the SDF slab's dimensions, so only the null one cannot be sampled): the buffer keeps its
    sentinel in every element, and every other array is that of the call with `colors` null, bit for bit."""
    import ctypes as C
    import torch
    from kangaroo_amd import _lib, mesh
    L = _lib.load()
    D, cell = 28, mesh.CELL[kind]
    bmin, bmax = (-1.0, -0.8, -1.1), (1.0, 0.9, 1.2)
    vol = roo.BoundedVolume(24, 20, D, bmin, bmax, kind=kind)
    roo.SdfSphere(vol, (0.1, -0.05, 0.15), 0.7)
    small = roo.BoundedVolume(24, 20, 7, bmin, bmax, kind="c32")
    assert not small.IsValid()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ref = lambda v: None if v is None else v.ref()
    z0, z1, s0, s1 = list(TV.slab_bounds(D, 2, 2))[1]
    views = [(vol, None, 0, 0, (None, small)), (vol.ZSlab(s0, s1), C.byref(_lib.KfxSlab(D, s0, bmin[2], bmax[2])), z0, z1, (None,))]
    for view, sl, lo, hi, colour_volumes in views:
        nbytes = L.kfx_mesh_scratch_bytes(view.ref(), cell, sl, lo, hi)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        totals = (C.c_ulonglong * 2)()
        _lib.check(L.kfx_mesh_plan(view.ref(), cell, sl, lo, hi, ptr(scratch), nbytes, totals, None))
        na, nt = int(totals[0]), int(totals[1])
        xbytes = L.kfx_mesh_index_scratch_bytes(view.ref(), cell, sl, lo, hi, totals)
        xscratch = torch.empty(xbytes, dtype=torch.uint8, device="cuda")
        nvert = C.c_ulonglong(0)
        _lib.check(L.kfx_mesh_index_plan(view.ref(), cell, sl, lo, hi, ptr(scratch), nbytes, totals, ptr(xscratch), xbytes, C.byref(nvert), None))
        V = int(nvert.value)
        assert na > 100 and nt > 200 and 0 < V < 3 * nt

        def run(cvol, colors, xcolors):
            full = lambda shape, dt: torch.full(shape, -7, dtype=dt, device="cuda")
            ci, to, f = full((na,), torch.int64), full((na,), torch.int32), full((nt, 3), torch.int32)
            v, n, xv, xn = (full((rows, 3), torch.float32) for rows in (3 * nt, 3 * nt, V, V))
            _lib.check(L.kfx_mesh_emit(view.ref(), cell, sl, lo, hi, ref(cvol), ptr(scratch), nbytes, totals, ptr(ci), ptr(to), ptr(v), ptr(n),
                                       ptr(colors), None))
            _lib.check(L.kfx_mesh_emit_indexed(view.ref(), cell, sl, lo, hi, ref(cvol), ptr(xscratch), xbytes, totals, V, ptr(xv), ptr(xn),
                                               ptr(xcolors), ptr(f), None))
            torch.cuda.synchronize()
            return ci.view(torch.int32), to, v, n, xv, xn, f

        plain = run(None, None, None)
        assert not any(bool((a == -7).any()) for a in plain)   # every element of every array is written
        for cvol in colour_volumes:
            colors = torch.full((3 * nt, 4), -7.0, dtype=torch.float32, device="cuda")
            xcolors = torch.full((V, 4), -7.0, dtype=torch.float32, device="cuda")
            got = run(cvol, colors, xcolors)
            assert bool((colors == -7.0).all()) and bool((xcolors == -7.0).all()), (sl is not None, cvol is not None)
            assert all(TV.bits_equal(a, b) for a, b in zip(got, plain)), (sl is not None, cvol is not None)


def read_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode().split("\n")
    nv = int([l for l in head if l.startswith("element vertex")][0].split()[2])
    nf = int([l for l in head if l.startswith("element face")][0].split()[2])
    nprop = sum(l.startswith("property float") for l in head)
    table = np.frombuffer(raw, "<f4", nv * nprop, end).reshape(nv, nprop)
    rows = np.frombuffer(raw, np.dtype([("k", "u1"), ("i", "<u4", 3)]), nf, end + 4 * nv * nprop)
    return len(raw), end, nv, nf, table, rows


def test_gpu_indexed_mesh_file(roo, tmp_path):
    """f) SaveMesh(indexed=True) of the 48^3 sphere: element vertex V, element face T, len(header) + 24 V + 13 T bytes, the body decodes
    to the arrays; the default call still writes the 3T-vertex file of its size (header + 72 T + 13 T)."""
    from kangaroo_amd import mesh
    ovol = TM.sphere_volume(48, 0.7)
    vol = upload(roo, ovol)
    wv, wn, _, wf = expected(ovol)
    V, Tn = len(wv), len(wf)
    assert mesh.SaveMesh(str(tmp_path / "i"), vol, indexed=True) == Tn
    size, head, nv, nf, table, rows = read_ply(str(tmp_path / "i.ply"))
    assert (nv, nf) == (V, Tn) and size == head + 24 * V + 13 * Tn
    assert T.nan_equal(table[:, :3], wv) and T.nan_equal(table[:, 3:], wn)
    assert (rows["k"] == 3).all() and np.array_equal(rows["i"], wf)
    assert mesh.SaveMesh(str(tmp_path / "s"), vol) == Tn
    size, head, nv, nf, table, rows = read_ply(str(tmp_path / "s.ply"))
    assert (nv, nf) == (3 * Tn, Tn) and size == head + 72 * Tn + 13 * Tn
    sv, sn, _ = oracle.marching_cubes(ovol, None, *TM.tables())
    assert T.nan_equal(table[:, :3], sv) and T.nan_equal(table[:, 3:], sn)
    assert np.array_equal(rows["i"], np.arange(3 * Tn, dtype=np.uint32).reshape(-1, 3))
    assert (72 + 13) * Tn / (24 * V + 13 * Tn) > 3.0   # the file: 85 T against ~25 T


def test_gpu_indexed_mesh_2048_half_cells_beyond_32_bit_cube_indices(roo):
    """g) the sphere of test_gpu_mesh_2048_half_cells_beyond_32_bit_cube_indices, every cube index >= 2^32, checked on the device:
    closed (V = T/2 + 2), every id < V and every vertex referenced, verts[faces] within 4 ulp of M = 1 of the soup
    (measured: T = 6 318 332, V = 3 159 168, copies within 1.19e-7 = 1 ulp)."""
    import torch
    from kangaroo_amd import mesh
    N = 2048
    vol = roo.BoundedVolume(N, N, N, (-1, -1, -1), (1, 1, 1), kind="f16")
    roo.SdfSphere(vol, (0.45, 0.0, 0.0), 0.4)
    v, n, _, f = mesh.ExtractMesh(vol, indexed=True)
    V, Tn = len(v), len(f)
    assert Tn > 1_000_000 and V == Tn // 2 + 2 and Tn % 2 == 0
    ids = f.reshape(-1).to(torch.int64) & 0xffffffff
    assert int(ids.max()) == V - 1 and int(ids.min()) == 0
    assert int(torch.bincount(ids, minlength=V).min()) >= 1
    sv, sn, _ = mesh.ExtractMesh(vol)
    assert len(sv) == 3 * Tn
    err = float((v[ids].double() - sv.double()).abs().max())
    print("2048^3 half: T = %d, V = %d, copies within %.3g = %.2f ulp of M = 1" % (Tn, V, err, err / W.ulp(1.0)))
    assert err <= 4 * W.ulp(1.0)
    del vol, v, n, f, ids, sv, sn
    torch.cuda.empty_cache()
