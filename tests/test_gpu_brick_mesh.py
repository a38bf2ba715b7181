"""Marching cubes straight from packed bricks (include/kfx_mesh_bricks.h, mesh.ExtractBrickMesh) against its definition: the existing
ExtractMesh(D, C, with_index=True) on the dense volume D that is NaN everywhere and then gets the same bricks unpacked (C: 0.5, then
the colour bricks).  The same cubes and, cube by cube, the same triangles bit for bit; only the order is the bricks'."""
import ctypes as C

import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import oracle, scenes

pytestmark = pytest.mark.gpu

NAN = float("nan")
E_RANGE = -4
GUARD = 0xA5


def _np(t):
    return None if t is None else t.cpu().numpy()


def dense_volume(roo, dims, bmin, bmax, kind, ids, cells):
    """the definition's D (kind f32 / f16: NaN, then the bricks) or C (kind c32: 0.5, then the bricks)"""
    D = roo.BoundedVolume(*[int(d) for d in dims], bmin, bmax, kind=kind)
    if kind == "c32":
        roo.ColorReset(D)
    else:
        roo.SdfReset(D, NAN)
    if len(ids):
        roo.BrickUnpack(D, ids, cells)
    return D


def by_cube(out):
    """(cube_index, triangles per cube, verts / norms / colors as int32 bits gathered in ascending cube order)"""
    v, n, c, ci, to = [_np(a) for a in out]
    ntri = len(v) // 3
    to = to.view(np.uint32).astype(np.int64)
    cnt = np.diff(np.append(to, ntri))
    assert np.all(cnt > 0) and (len(to) == 0 or to[0] == 0)          # the list is packed: every cube's triangles follow the one before
    order = np.argsort(ci, kind="stable")
    tri = np.concatenate([np.arange(to[k], to[k] + cnt[k]) for k in order]) if len(order) else np.zeros(0, np.int64)
    pick = lambda a, k: None if a is None else a.reshape(ntri, 3, k)[tri].view(np.int32)
    return ci[order], cnt[order], pick(v, 3), pick(n, 3), pick(c, 4)


def assert_brick_order(ci, dims, ids):
    """cubes brick by brick in ascending brick id, within a brick by ascending dense index"""
    w, h, d = [int(v) for v in dims]
    z, y, x = ci % (d - 1), (ci // (d - 1)) % (h - 1), ci // ((d - 1) * (h - 1))
    nbx, nby = (w + 7) // 8, (h + 7) // 8
    bid = ((z >> 3) * nby + (y >> 3)) * nbx + (x >> 3)
    assert np.all(np.diff(bid) >= 0), "bricks out of order"
    assert np.all(np.diff(ci)[np.diff(bid) == 0] > 0), "cubes of a brick out of order"
    assert np.isin(bid, np.asarray(ids).astype(np.int64)).all()
    return bid


def assert_equals_dense(roo, mesh, dims, bmin, bmax, kind, ids, cells, cids=None, ccells=None, min_verts=300):
    """the helper of every case with a dense comparator; returns (brick mesh, dense mesh)"""
    got = mesh.ExtractBrickMesh(dims, bmin, bmax, kind, ids, cells, cids, ccells, with_index=True)
    D = dense_volume(roo, dims, bmin, bmax, kind, ids, cells)
    Cv = dense_volume(roo, dims, bmin, bmax, "c32", cids, ccells) if cids is not None else None
    want = mesh.ExtractMesh(D, Cv, with_index=True)
    print("brick mesh: %d bricks, %d cubes, %d vertices; dense: %d cubes, %d vertices" % (len(ids), len(got[3]), len(got[0]), len(want[3]), len(want[0])))
    assert len(want[0]) > min_verts
    gci, gcnt, gv, gn, gc = by_cube(got)
    wci, wcnt, wv, wn, wc = by_cube(want)
    assert np.array_equal(gci, wci), "the active cubes differ"
    assert np.array_equal(gcnt, wcnt), "triangles per cube differ"
    assert np.array_equal(gv, wv), "vertex bits differ"
    assert np.array_equal(gn, wn), "normal bits differ"
    assert (gc is None) == (wc is None) and (gc is None or np.array_equal(gc, wc)), "colour bits differ"
    assert_brick_order(_np(got[3]), dims, _np(ids) if hasattr(ids, "cpu") else ids)
    return got, want


def u32(ids):
    return ids.cpu().numpy().view(np.uint32)


# ---- case 1: a sphere centred on a brick corner of a 40 x 24 x 32 frame (voxel 1/16), every brick live -------------------------------
DIMS1 = (40, 24, 32)


def box_of(dims, voxel):
    return (0.0, 0.0, 0.0), tuple((d - 1) * voxel for d in dims)


@pytest.fixture(scope="module")
def sphere(roo):
    bmin, bmax = box_of(DIMS1, 1 / 16)
    vol = roo.BoundedVolume(*DIMS1, bmin, bmax)
    roo.SdfSphere(vol, (1.0, 0.5, 1.0), 0.4)   # cell (16, 8, 16): the corner eight bricks share
    ids, cells = roo.BrickPack(vol, NAN)
    assert ids.numel() == 5 * 3 * 4
    return bmin, bmax, ids, cells


def test_gpu_brick_mesh_sphere_straddling_bricks(roo, sphere):
    from kangaroo_amd import mesh
    bmin, bmax, ids, cells = sphere
    got, _ = assert_equals_dense(roo, mesh, DIMS1, bmin, bmax, "f32", ids, cells)
    bid = assert_brick_order(_np(got[3]), DIMS1, u32(ids))
    assert len(np.unique(bid)) >= 8   # the surface lies in the eight bricks around the corner at least


def test_gpu_brick_mesh_ragged_frame_with_unobserved_cells(roo):
    """44 x 29 x 35: partial bricks on all three axes, a surface that leaves through the frame's faces (the gradient's clamps), NaN
    cells through the band, random bytes in the payload outside the frame"""
    import torch
    from kangaroo_amd import mesh
    dims = (44, 29, 35)
    bmin, bmax = box_of(dims, 1 / 16)
    vol = roo.BoundedVolume(*dims, bmin, bmax)
    roo.SdfSphere(vol, (0.5, 0.9, 1.0), 1.15)
    z, y, x = torch.meshgrid(*[torch.arange(n, device="cuda") for n in dims[::-1]], indexing="ij")
    vol.tensor()[..., 0][(z + y + x) % 7 == 0] = NAN
    ids, cells = roo.BrickPack(vol, NAN)
    host, idn = cells.cpu().numpy().reshape(-1, 8, 8, 8, 8).copy(), u32(ids).astype(np.int64)
    nbx, nby = 6, 4
    bx, by, bz = idn % nbx, (idn // nbx) % nby, idn // (nbx * nby)
    l = np.arange(8)
    outside = ((bz[:, None] * 8 + l)[:, :, None, None] >= dims[2]) | ((by[:, None] * 8 + l)[:, None, :, None] >= dims[1]) | \
        ((bx[:, None] * 8 + l)[:, None, None, :] >= dims[0])
    assert outside.any() and not outside.all()
    host[outside] = np.random.default_rng(3).integers(0, 256, (int(outside.sum()), 8), dtype=np.uint8)
    cells = torch.from_numpy(host.reshape(len(idn), -1)).cuda()
    assert_equals_dense(roo, mesh, dims, bmin, bmax, "f32", ids, cells)


def test_gpu_brick_mesh_with_absent_bricks(roo, sphere):
    """about 40 % of the bricks dropped, and every neighbour of one surface brick: cubes that touch an absent brick have no triangles,
    normals whose stencil reaches into one are zero -- as the dense mesh of the same subset"""
    import torch
    from kangaroo_amd import mesh
    bmin, bmax, ids, cells = sphere
    full = mesh.ExtractBrickMesh(DIMS1, bmin, bmax, "f32", ids, cells, with_index=True)
    idn = u32(ids).astype(np.int64)
    keep = np.random.default_rng(7).random(len(idn)) >= 0.4
    nbx, nby = 5, 3
    lone = (2 * nby + 1) * nbx + 2   # brick (2, 1, 2): one of the eight around the sphere's centre
    assert lone in assert_brick_order(_np(full[3]), DIMS1, idn)
    b = np.stack([idn % nbx, (idn // nbx) % nby, idn // (nbx * nby)], 1)
    near = np.all(np.abs(b - np.array([2, 1, 2])) <= 1, 1)
    keep[near] = False
    keep[idn == lone] = True
    sel = torch.from_numpy(np.nonzero(keep)[0]).cuda()
    got, _ = assert_equals_dense(roo, mesh, DIMS1, bmin, bmax, "f32", ids[sel], cells[sel], min_verts=30)
    assert 0 < len(got[3]) < len(full[3])
    assert lone in assert_brick_order(_np(got[3]), DIMS1, idn[keep])


def test_gpu_brick_mesh_half_cells_of_a_fused_room(roo):
    from kangaroo_amd import mesh
    dims, (w, h) = (72, 16, 24), (160, 120)
    bmin, bmax, near, far = scenes.SCENES["room"]
    K, tr = scenes.intrinsics(w, h), scenes.trunc_dist(bmin, bmax, dims)
    vol = roo.BoundedVolume(*dims, bmin, bmax, kind="f16")
    roo.SdfReset(vol, NAN)
    for i in range(3):
        T_wc = scenes.orbit_pose(i, 8)
        raw = T.upload_image(roo, scenes.render_depth("room", w, h, T_wc, K))
        f, vbo, nrm = roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h, "f32x4")
        roo.BilateralFilter(f, raw, **scenes.BILATERAL)
        roo.DepthToVbo(vbo, f, K)
        roo.NormalsFromVbo(nrm, vbo)
        roo.SdfFuse(vol, f, nrm, scenes.se3_inverse(T_wc), K, tr, scenes.MAX_W, scenes.MIN_COS_THETA)
    ids, cells = roo.BrickPack(vol, NAN)
    assert 0 < ids.numel() <= 9 * 2 * 3 and cells.shape[1] == 2048
    assert_equals_dense(roo, mesh, dims, bmin, bmax, "f16", ids, cells)


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_gpu_brick_mesh_colour_with_absent_colour_bricks(roo, kind):
    """the colour list is packed against 0.5, a list of its own; colour bricks under the surface are dropped from it, so it is another
    set of bricks than the SDF list: the colour reads 0.5 there, as the comparator's"""
    import torch
    import test_color_cpu as TC
    from kangaroo_amd import mesh
    ovol, ocvol, K, Kimg, tr, near, far, inputs = TC.color_setup(0, 160, 120, 160, 120, dims=(64, 64, 64))
    for fr in inputs:
        oracle.sdf_fuse_color(ovol, ocvol, fr["f"], fr["nrm"], fr["T_cw"], K, fr["rgb"], fr["T_iw"], Kimg, tr, 1000.0, 0.1, nthreads=0)
    dims = (64, 64, 64)
    vol = roo.BoundedVolume(*dims, ovol.boxmin, ovol.boxmax, kind=kind)
    vol.MemcpyFromHost(ovol.data)
    cvol = roo.BoundedVolume(*dims, ocvol.boxmin, ocvol.boxmax, kind="c32")
    cvol.MemcpyFromHost(ocvol.data)
    ids, cells = roo.BrickPack(vol, NAN)
    cids, ccells = roo.BrickPack(cvol, 0.5)
    first = mesh.ExtractBrickMesh(dims, vol.boxmin, vol.boxmax, kind, ids, cells, with_index=True)
    surface = np.unique(assert_brick_order(_np(first[3]), dims, u32(ids)))
    drop = np.intersect1d(surface, u32(cids).astype(np.int64))[::5][:6]
    assert len(drop) >= 3
    sel = torch.from_numpy(np.nonzero(~np.isin(u32(cids).astype(np.int64), drop))[0]).cuda()
    assert not np.array_equal(u32(ids), u32(cids[sel]))   # (the two lists are not the same set of bricks)
    got, want = assert_equals_dense(roo, mesh, dims, vol.boxmin, vol.boxmax, kind, ids, cells, cids[sel], ccells[sel])
    c = _np(got[2])
    assert c is not None and np.all(c[:, 3] == 1.0) and (c[:, 0] == 0.5).any() and (c[:, 0] != 0.5).any()


def test_gpu_brick_mesh_of_many_bricks_scans_across_blocks(roo):
    """16 x 16 x 1600: 800 bricks, each with surface -- more than one scan block of 256 bricks, cube indices far apart"""
    import torch
    from kangaroo_amd import mesh
    dims = (16, 16, 1600)
    bmin, bmax = box_of(dims, 1 / 16)
    vol = roo.BoundedVolume(*dims, bmin, bmax)
    z, y, x = torch.meshgrid(*[torch.arange(n, device="cuda", dtype=torch.float32) for n in dims[::-1]], indexing="ij")
    t = vol.tensor()
    t[..., 0] = x - 7.5 + 1.2 * torch.sin(z * (2 * np.pi / 8) + 0.3) + 0.01 * y
    t[..., 1] = 1.0
    ids, cells = roo.BrickPack(vol, NAN)
    assert ids.numel() == 800
    got, _ = assert_equals_dense(roo, mesh, dims, bmin, bmax, "f32", ids, cells)
    assert len(np.unique(assert_brick_order(_np(got[3]), dims, u32(ids)))) == 800


def test_gpu_brick_mesh_far_inside_a_4096_frame(roo, sphere):
    """the sphere's bricks at brick (500, 500, 500) of a 4096^3 frame with voxel 2^-6: ids near 2^27, cube indices beyond 2^32, the
    scratch of the small frame; no dense comparator exists -- the small frame of the same voxel is one"""
    import torch
    from kangaroo_amd import mesh
    _, _, ids, cells = sphere
    n, off, F = ids.numel(), 500, 4096
    idn = u32(ids).astype(np.int64)
    bx, by, bz = idn % 5, (idn // 5) % 3, idn // 15
    far_ids = ((bz + off) * 512 + by + off) * 512 + bx + off
    assert np.all(np.diff(far_ids) > 0) and far_ids.max() < 2 ** 31 and far_ids.min() > 2 ** 26   # (near 2^27)
    # the scratch of the small frame serves the far one: exactly case 1's bytes are accepted by a plan of either, and plan the same totals
    from kangaroo_amd import _lib
    L, need = _lib.load(), mesh.BrickMeshScratchBytes(n)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    far_dev = torch.from_numpy(far_ids.astype(np.uint32).view(np.int32)).cuda()
    planned = []
    for dims, lst in ((DIMS1, ids), ((F, F, F), far_dev)):
        fr = _lib.KfxVolume(0, None, dims[0], dims[1], 0, dims[2])
        for i in range(3):
            fr.boxmin[i], fr.boxmax[i] = 0.0, (dims[i] - 1) * 2.0 ** -6
        tot = (C.c_ulonglong * 2)()
        _lib.check(L.kfx_mesh_bricks_plan(C.byref(fr), 0, C.c_void_p(lst.data_ptr()), C.c_void_p(cells.data_ptr()), n, C.c_void_p(scratch.data_ptr()), need, tot, None))
        planned.append((tot[0], tot[1]))
    assert planned[0] == planned[1] and planned[0][0] > 100
    small =mesh.ExtractBrickMesh(DIMS1, *box_of(DIMS1, 2.0 ** -6), "f32", ids, cells, with_index=True)
    far = mesh.ExtractBrickMesh((F, F, F), *box_of((F, F, F), 2.0 ** -6), "f32", far_ids.astype(np.uint32), cells, with_index=True)
    sv, sn, _, sci, sto = [_np(a) for a in small]
    fv, fn, _, fci, fto = [_np(a) for a in far]
    assert len(sv) > 300 and fci.dtype == np.int64
    z, y, x = sci % 31, (sci // 31) % 23, sci // (31 * 23)
    want_ci = ((x + 8 * off) * (F - 1) + (y + 8 * off)) * (F - 1) + (z + 8 * off)
    assert np.array_equal(fci, want_ci) and len(np.unique(fci)) == len(fci) and fci.min() > 2 ** 32   # the same cubes, translated; no 32-bit wrap
    assert np.array_equal(fto, sto) and fv.shape == sv.shape
    shift = 8 * off * 2.0 ** -6
    err = np.abs((fv.astype(np.float64) - shift) - sv.astype(np.float64)).max()
    bound = 8 * np.spacing(np.float32(64))
    print("far frame: max position difference %.3g, bound %.3g" % (err, bound))
    assert err <= bound


def test_gpu_brick_mesh_writes_nothing_beyond_the_totals_and_refuses_other_totals(roo, sphere):
    import torch
    from kangaroo_amd import _lib, mesh
    L = _lib.load()
    bmin, bmax, ids, cells = sphere
    n = ids.numel()
    frame = _lib.KfxVolume(0, None, *DIMS1[:2], 0, DIMS1[2])
    for i in range(3):
        frame.boxmin[i], frame.boxmax[i] = bmin[i], bmax[i]
    nbytes = mesh.BrickMeshScratchBytes(n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    totals = (C.c_ulonglong * 2)()
    P = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(L.kfx_mesh_bricks_plan(C.byref(frame), 0, P(ids), P(cells), n, P(scratch), nbytes, totals, None))
    na, nt = int(totals[0]), int(totals[1])
    assert na > 100 and nt >= na
    pad = 256
    bufs = [torch.full((size + pad,), GUARD, dtype=torch.uint8, device="cuda") for size in (8 * na, 4 * na, 36 * nt, 36 * nt)]
    emit = lambda tot: L.kfx_mesh_bricks_emit(C.byref(frame), 0, P(ids), P(cells), n, None, None, 0, P(scratch), nbytes, tot, *[P(b) for b in bufs], None, None)
    for bad in ((na + 1, nt), (na, nt - 1), (na - 1, nt)):
        assert emit((C.c_ulonglong * 2)(*bad)) == E_RANGE
        torch.cuda.synchronize()
        assert all(bool((b == GUARD).all()) for b in bufs), "a refused emit wrote something"
    _lib.check(emit(totals))
    torch.cuda.synchronize()
    for b, size in zip(bufs, (8 * na, 4 * na, 36 * nt, 36 * nt)):
        assert bool((b[size:] == GUARD).all()), "written beyond the totals"
    ref = mesh.ExtractBrickMesh(DIMS1, bmin, bmax, "f32", ids, cells, with_index=True)
    assert np.array_equal(bufs[0][:8 * na].cpu().numpy().view(np.int64), _np(ref[3]))
    assert np.array_equal(bufs[2][:36 * nt].cpu().numpy().view(np.int32), _np(ref[0]).view(np.int32).reshape(-1))
    # no bricks: (0, 0), nothing launched, an empty mesh
    totals[0] = totals[1] = 99
    _lib.check(L.kfx_mesh_bricks_plan(C.byref(frame), 0, None, None, 0, P(scratch), nbytes, totals, None))
    assert (totals[0], totals[1]) == (0, 0)
    v, nrm, col = mesh.ExtractBrickMesh(DIMS1, bmin, bmax, "f32", np.zeros(0, np.uint32), np.zeros((0, 4096), np.uint8))
    assert v.shape == (0, 3) and nrm.shape == (0, 3) and col is None
    with pytest.raises(ValueError, match="ascending"):
        mesh.ExtractBrickMesh(DIMS1, bmin, bmax, "f32", np.array([3, 3], np.uint32), np.zeros((2, 4096), np.uint8))
    with pytest.raises(ValueError, match="come together"):
        mesh.ExtractBrickMesh(DIMS1, bmin, bmax, "f32", ids, cells, color_ids=np.zeros(0, np.uint32))


@pytest.mark.parametrize("order", ["repeated", "reversed", "shuffled"])
def test_gpu_brick_mesh_of_unsorted_or_repeated_device_ids_stays_inside_its_buffers(roo, sphere, order):
    """ids on the device cannot be validated by the host: the mesh is unspecified, the accesses are not.  The plan counts a cube from
    its list entry and the emit finds the cube's brick by search; `repeated` lists every id twice, first with a payload of many
    triangles per cube and then with the brick's own, so that the two disagree about a cube's triangles.  Outputs and scratch sit in front of 0xA5 guard regions."""
    import torch
    from kangaroo_amd import _lib, mesh
    L = _lib.load()
    bmin, bmax, ids, cells = sphere
    n0 = ids.numel()
    if order == "repeated":
        # entry 2 j: id j with a payload whose values alternate in sign from cell to cell (every cube of it has 4 triangles);
        # entry 2 j + 1: id j with the brick's own payload.  The search finds entry 2 j for the cubes counted from entry 2 j + 1.
        z, y, x = torch.meshgrid(*[torch.arange(8, device="cuda")] * 3, indexing="ij")
        checker = torch.stack([1.0 - 2.0 * ((x + y + z) & 1).float(), torch.ones(8, 8, 8, device="cuda")], -1).contiguous().view(torch.uint8).reshape(1, -1)
        ids = ids.repeat_interleave(2)
        cells = torch.stack([checker.expand(n0, -1), cells], 1).reshape(2 * n0, -1).contiguous()
    else:
        perm = torch.arange(n0 - 1, -1, -1) if order == "reversed" else torch.from_numpy(np.random.default_rng(11).permutation(n0))
        ids, cells = ids[perm.cuda()].contiguous(), cells[perm.cuda()].contiguous()
    n = ids.numel()
    before = (ids.clone(), cells.clone())
    frame = _lib.KfxVolume(0, None, *DIMS1[:2], 0, DIMS1[2])
    for i in range(3):
        frame.boxmin[i], frame.boxmax[i] = bmin[i], bmax[i]
    pad, nbytes = 1024, mesh.BrickMeshScratchBytes(n)
    scratch = torch.full((nbytes + pad,), GUARD, dtype=torch.uint8, device="cuda")
    totals = (C.c_ulonglong * 2)()
    P = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(L.kfx_mesh_bricks_plan(C.byref(frame), 0, P(ids), P(cells), n, P(scratch), nbytes, totals, None))
    na, nt = int(totals[0]), int(totals[1])
    print("%s ids: %d entries, planned %d cubes, %d triangles" % (order, n, na, nt))
    assert nt >= na and (order != "repeated" or na > 100)   # (every entry of the repeated list is counted from its own payload)
    sizes = (8 * na, 4 * na, 36 * nt, 36 * nt)
    bufs = [torch.full((size + pad,), GUARD, dtype=torch.uint8, device="cuda") for size in sizes]
    _lib.check(L.kfx_mesh_bricks_emit(C.byref(frame), 0, P(ids), P(cells), n, None, None, 0, P(scratch), nbytes, totals, *[P(b) for b in bufs], None, None))
    torch.cuda.synchronize()
    for b, size in zip(bufs, sizes):
        assert bool((b[size:] == GUARD).all()), "written beyond the totals"
    assert bool((scratch[nbytes:] == GUARD).all()), "written beyond the scratch"
    assert torch.equal(ids, before[0]) and torch.equal(cells, before[1])


def test_gpu_world_mesh_of_a_spilling_pipeline(roo, tmp_path):
    """the set-up of test_gpu_a_spilling_volume_gets_back_what_it_left_behind, then (8, 0, -8): both stores hold bricks, and the world
    mesh is the dense mesh of the 40 x 32 x 40 frame -- more than the shifted volume's own"""
    import torch
    from kangaroo_amd import bricks, mesh
    from kangaroo_amd.pipeline import FramePipeline
    N, w, h = 32, 80, 60
    lo, hi = (-1.0, -1.0, 2.0), (0.9375, 0.9375, 3.9375)
    p = FramePipeline(roo, (N, N, N), lo, hi, w, h, track=True, color=True, follow=dict(quantum=8, spill=True))
    for i in range(3):
        T_wc = scenes.orbit_pose(i, 8)
        raw = T.upload_image(roo, scenes.render_depth("room", w, h, T_wc, p.K))
        rgb = roo.Image(w, h, "u8x3").MemcpyFromHost(scenes.render_rgb("room", w, h, T_wc, p.Kimg))
        p.step(T_wc, raw, rgb)
    assert p.shifts == []
    before = by_cube(mesh.ExtractMesh(p.vol, p.cvol, with_index=True))
    p.shift_volume((8, 0, -8))
    torch.cuda.synchronize()
    sizes = (len(p.store), p.store.nbytes, len(p.cstore), p.cstore.nbytes)
    assert sizes[0] > 0 and sizes[2] > 0
    got = p.ExtractWorldMesh(with_index=True)
    (flo, fdims, bmin, bmax, ids, cells), (clo, cdims, cbmin, cbmax, cids, ccells) = p.world_bricks()
    assert tuple(fdims) == (40, 32, 40) == tuple(cdims) and tuple(flo) == (0, 0, -8) == tuple(clo)
    assert np.array_equal(bmin.view(np.uint32), cbmin.view(np.uint32)) and np.array_equal(bmax.view(np.uint32), cbmax.view(np.uint32))
    assert np.array_equal(bmin, np.array([-1.0, -1.0, 1.5], np.float32)) and np.array_equal(bmax, np.array([1.4375, 0.9375, 3.9375], np.float32))
    D = dense_volume(roo, fdims, bmin, bmax, "f32", ids, cells)
    Cv = dense_volume(roo, fdims, bmin, bmax, "c32", cids, ccells)
    want = mesh.ExtractMesh(D, Cv, with_index=True)
    g, wnt = by_cube(got), by_cube(want)
    for a, b in zip(g, wnt):
        assert np.array_equal(a, b)
    assert_brick_order(_np(got[3]), fdims, ids)
    alone = mesh.ExtractMesh(p.vol, p.cvol)
    print("world mesh %d triangles, the shifted volume alone %d" % (len(got[0]) // 3, len(alone[0]) // 3))
    assert len(got[0]) > len(alone[0]) > 0
    assert sizes == (len(p.store), p.store.nbytes, len(p.cstore), p.cstore.nbytes)   # the stores are as they were
    ntri = p.SaveWorldMesh(str(tmp_path / "world"))
    head = open(str(tmp_path / "world.ply"), "rb").read(600).decode("latin1")
    assert ntri == len(got[0]) // 3 and "element vertex %d\n" % (3 * ntri) in head and "element face %d\n" % ntri in head and "property float red" in head
    # and back: the frame is the volume again, and the world mesh the restored volume's, cube by cube
    p.shift_volume((-8, 0, 8))
    torch.cuda.synchronize()
    assert len(p.store) == 0 and len(p.cstore) == 0
    (flo, fdims, bmin, bmax, _, _), _ = p.world_bricks()
    assert tuple(flo) == (0, 0, 0) and tuple(fdims) == (N, N, N)
    assert np.array_equal(bmin.view(np.uint32), p.vol.boxmin.view(np.uint32)) and np.array_equal(bmax.view(np.uint32), p.vol.boxmax.view(np.uint32))
    again, restored = by_cube(p.ExtractWorldMesh(with_index=True)), by_cube(mesh.ExtractMesh(p.vol, p.cvol, with_index=True))
    for a, b, c in zip(again, restored, before):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    # a pipeline without follow= has no store: its world mesh is the brick mesh of the live volume
    q = FramePipeline(roo, (N, N, N), lo, hi, w, h)
    T_wc = scenes.orbit_pose(0, 8)
    q.step(T_wc, T.upload_image(roo, scenes.render_depth("room", w, h, T_wc, q.K)))
    assert q.store is None
    plain, dense = by_cube(q.ExtractWorldMesh(with_index=True)), by_cube(mesh.ExtractMesh(q.vol, with_index=True))
    assert len(plain[0]) > 100 and plain[4] is None
    for a, b in zip(plain[:4], dense[:4]):
        assert np.array_equal(a, b)
