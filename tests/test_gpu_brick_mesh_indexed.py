"""The indexed brick mesh (include/kfx_mesh_bricks_index.h, mesh.ExtractBrickMesh(indexed=True)) against its definition: the
sequential first-occurrence weld, by lattice edge, of the brick soup ExtractBrickMesh(with_index=True) returns for the same lists
(tests/brick_mesh_weld.py), keyed from the dense volume D those bricks unpack into, read back to the host.  Vertices, normals and
colours are compared as int32 bits, faces exactly.  The recipes are test_gpu_brick_mesh.py's, case by case."""
import ctypes as C

import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import oracle, scenes

import brick_mesh_weld as BW
import mesh_weld as W
import test_gpu_brick_mesh as TB
from test_gpu_brick_mesh import sphere   # noqa: F401  (the module's fixture: case 1's bricks)

pytestmark = pytest.mark.gpu

NAN = float("nan")
E_RANGE = -4
GUARD = 0xA5
DIMS1 = TB.DIMS1


def _np(t):
    return None if t is None else (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t))


def bits(a):
    return None if a is None else np.ascontiguousarray(_np(a)).view(np.int32)


def assert_is_the_weld(got, want, what=""):
    v, n, c, f = got
    wv, wn, wc, wf = want
    f = _np(f).view(np.uint32)
    assert f.shape == wf.shape and np.array_equal(f, wf), "%s: faces differ" % what
    assert len(_np(v)) == len(wv) and np.array_equal(bits(v), bits(wv)), "%s: vertex bits differ" % what
    assert np.array_equal(bits(n), bits(wn)), "%s: normal bits differ" % what
    assert (c is None) == (wc is None) and (c is None or np.array_equal(bits(c), bits(wc))), "%s: colour bits differ" % what


def check_case(roo, dims, bmin, bmax, kind, ids, cells, cids=None, ccells=None, min_tris=100, what=""):
    """the indexed mesh of the lists equals the weld of their soup; returns (indexed mesh, soup, D's values, edges with another first
    cube than in dense order)"""
    from kangaroo_amd import mesh
    soup = mesh.ExtractBrickMesh(dims, bmin, bmax, kind, ids, cells, cids, ccells, with_index=True)
    got = mesh.ExtractBrickMesh(dims, bmin, bmax, kind, ids, cells, cids, ccells, indexed=True)
    val = W.values(TB.dense_volume(roo, dims, bmin, bmax, kind, ids, cells).MemcpyToHost())
    sv, sn, sc, ci, to = [_np(a) for a in soup]
    want, other = BW.weld(val, sv, sn, sc, ci, to)
    V, Tn = len(want[0]), len(want[3])
    print("%s: %d bricks, T = %d, V = %d (%.1f %% of 3T), %d edges with another first cube than in dense order"
          % (what, len(ids), Tn, V, 100.0 * V / max(1, 3 * Tn), other))
    assert Tn > min_tris and V < 3 * Tn
    assert_is_the_weld(got, want, what)
    assert BW.ids_in_first_occurrence_order(_np(got[3]).view(np.uint32), V)
    return got, soup, val, other


# ---- 1: the sphere on the corner eight bricks share ------------------------------------------------------------------------------
def test_gpu_indexed_brick_mesh_welds_a_sphere_across_brick_faces_edges_and_the_shared_corner(roo, sphere, tmp_path):
    from kangaroo_amd import mesh
    bmin, bmax, ids, cells = sphere
    got, soup, val, other = check_case(roo, DIMS1, bmin, bmax, "f32", ids, cells, what="sphere")
    V, Tn = len(got[0]), len(got[3])
    faces = _np(got[3]).view(np.uint32)
    assert V == Tn // 2 + 2 and W.closed_with_euler_2(faces, V)
    assert other == 0
    D = TB.dense_volume(roo, DIMS1, bmin, bmax, "f32", ids, cells)
    dense = mesh.ExtractMesh(D, indexed=True)
    assert len(dense[0]) == V and len(dense[3]) == Tn
    # the same vertex set as the dense indexed mesh: where every cube is active the first cube is the same, and so are the values
    order = lambda v, n: np.unique(np.concatenate([bits(v), bits(n)], 1), axis=0)
    assert np.array_equal(order(got[0], got[1]), order(dense[0], dense[1]))
    with pytest.raises(ValueError, match="with_index"):
        mesh.ExtractBrickMesh(DIMS1, bmin, bmax, "f32", ids, cells, with_index=True, indexed=True)
    # SaveBrickMesh(indexed=True): V vertices of 24 bytes, T faces of 13
    assert mesh.SaveBrickMesh(str(tmp_path / "s"), DIMS1, bmin, bmax, "f32", ids, cells, indexed=True) == Tn
    v, n, c, f = read_ply(str(tmp_path / "s.ply"), V, Tn, 6)
    assert np.array_equal(bits(v), bits(got[0])) and np.array_equal(bits(n), bits(got[1])) and np.array_equal(f, faces)


def read_ply(path, V, Tn, props):
    """a binary PLY of write_ply's: the header states V and T, the file is the header + 4 props V + 13 T bytes, and the body decodes"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("latin1")
    assert "element vertex %d\n" % V in head and "element face %d\n" % Tn in head
    assert head.count("property float") == props
    assert len(raw) == end + 4 * props * V + 13 * Tn
    table = np.frombuffer(raw, "<f4", props * V, end).reshape(V, props)
    rows = np.frombuffer(raw, np.dtype([("k", "u1"), ("i", "<u4", 3)]), Tn, end + 4 * props * V)
    assert np.all(rows["k"] == 3)
    return table[:, :3], table[:, 3:6], (table[:, 6:] if props > 6 else None), rows["i"]


# ---- 2: the ragged frame with the NaN lattice: the case a copied dense owner rule fails ------------------------------------------
def ragged_lists(roo):
    """test_gpu_brick_mesh_ragged_frame_with_unobserved_cells's lists: 44 x 29 x 35, the % 7 NaN lattice, random bytes in the payload
    outside the frame"""
    import torch
    dims = (44, 29, 35)
    bmin, bmax = TB.box_of(dims, 1 / 16)
    vol = roo.BoundedVolume(*dims, bmin, bmax)
    roo.SdfSphere(vol, (0.5, 0.9, 1.0), 1.15)
    z, y, x = torch.meshgrid(*[torch.arange(n, device="cuda") for n in dims[::-1]], indexing="ij")
    vol.tensor()[..., 0][(z + y + x) % 7 == 0] = NAN
    ids, cells = roo.BrickPack(vol, NAN)
    host, idn = cells.cpu().numpy().reshape(-1, 8, 8, 8, 8).copy(), TB.u32(ids).astype(np.int64)
    nbx, nby = 6, 4
    bx, by, bz = idn % nbx, (idn // nbx) % nby, idn // (nbx * nby)
    l = np.arange(8)
    outside = ((bz[:, None] * 8 + l)[:, :, None, None] >= dims[2]) | ((by[:, None] * 8 + l)[:, None, :, None] >= dims[1]) | \
        ((bx[:, None] * 8 + l)[:, None, None, :] >= dims[0])
    assert outside.any() and not outside.all()
    host[outside] = np.random.default_rng(3).integers(0, 256, (int(outside.sum()), 8), dtype=np.uint8)
    return dims, bmin, bmax, ids, torch.from_numpy(host.reshape(len(idn), -1)).cuda()


def test_gpu_indexed_brick_mesh_of_a_ragged_frame_where_owners_differ_from_the_dense_order(roo):
    dims, bmin, bmax, ids, cells = ragged_lists(roo)
    got, soup, val, other = check_case(roo, dims, bmin, bmax, "f32", ids, cells, what="ragged")
    V = len(got[0])
    assert V == W.count_lattice_edges(val)
    assert other >= 1, "no edge has another first cube than in dense order: the case does not separate the two owner rules"
    # de-indexed, the mesh is the soup within the last bits: a dropped copy was interpolated from the edge's other end
    back = _np(got[0])[_np(got[3]).view(np.uint32).reshape(-1).astype(np.int64)]
    sv = _np(soup[0])
    bound = 4 * W.ulp(max(abs(float(c)) for c in tuple(bmin) + tuple(bmax)))
    err = float(np.abs(back.astype(np.float64) - sv.astype(np.float64)).max())
    print("ragged: de-indexed positions differ from the soup by at most %.3g (bound %.3g)" % (err, bound))
    assert err <= bound


# ---- 3: absent bricks ------------------------------------------------------------------------------------------------------------
def test_gpu_indexed_brick_mesh_with_absent_bricks_has_owners_at_faces_that_no_longer_exist(roo, sphere):
    import torch
    bmin, bmax, ids, cells = sphere
    idn = TB.u32(ids).astype(np.int64)
    keep = np.random.default_rng(7).random(len(idn)) >= 0.4
    nbx, nby = 5, 3
    lone = (2 * nby + 1) * nbx + 2   # brick (2, 1, 2): one of the eight around the sphere's centre
    b = np.stack([idn % nbx, (idn // nbx) % nby, idn // (nbx * nby)], 1)
    keep[np.all(np.abs(b - np.array([2, 1, 2])) <= 1, 1)] = False
    keep[idn == lone] = True
    sel = torch.from_numpy(np.nonzero(keep)[0]).cuda()
    got, soup, val, _ = check_case(roo, DIMS1, bmin, bmax, "f32", ids[sel], cells[sel], min_tris=10, what="absent bricks")
    assert lone in TB.assert_brick_order(_np(soup[3]), DIMS1, idn[keep])
    assert len(got[0]) == W.count_lattice_edges(val)
    assert not W.closed_with_euler_2(_np(got[3]).view(np.uint32), len(got[0]))   # (the surface is open where bricks are gone)


# ---- 4: half cells ---------------------------------------------------------------------------------------------------------------
def test_gpu_indexed_brick_mesh_of_half_cells_of_a_fused_room(roo):
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
    got, _, val, _ = check_case(roo, dims, bmin, bmax, "f16", ids, cells, what="half cells")
    assert len(got[0]) == W.count_lattice_edges(val)


# ---- 5: colour, with absent colour bricks ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused_colour_room():
    import test_color_cpu as TC
    ovol, ocvol, K, Kimg, tr, near, far, inputs = TC.color_setup(0, 160, 120, 160, 120, dims=(64, 64, 64))
    for fr in inputs:
        oracle.sdf_fuse_color(ovol, ocvol, fr["f"], fr["nrm"], fr["T_cw"], K, fr["rgb"], fr["T_iw"], Kimg, tr, 1000.0, 0.1, nthreads=0)
    return ovol, ocvol


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_gpu_indexed_brick_mesh_colours_are_the_first_occurrences(roo, fused_colour_room, kind):
    import torch
    from kangaroo_amd import mesh
    ovol, ocvol = fused_colour_room
    dims = (64, 64, 64)
    vol = roo.BoundedVolume(*dims, ovol.boxmin, ovol.boxmax, kind=kind)
    vol.MemcpyFromHost(ovol.data)
    cvol = roo.BoundedVolume(*dims, ocvol.boxmin, ocvol.boxmax, kind="c32")
    cvol.MemcpyFromHost(ocvol.data)
    ids, cells = roo.BrickPack(vol, NAN)
    cids, ccells = roo.BrickPack(cvol, 0.5)
    first = mesh.ExtractBrickMesh(dims, vol.boxmin, vol.boxmax, kind, ids, cells, with_index=True)
    surface = np.unique(TB.assert_brick_order(_np(first[3]), dims, TB.u32(ids)))
    drop = np.intersect1d(surface, TB.u32(cids).astype(np.int64))[::5][:6]
    assert len(drop) >= 3
    sel = torch.from_numpy(np.nonzero(~np.isin(TB.u32(cids).astype(np.int64), drop))[0]).cuda()
    got, _, _, _ = check_case(roo, dims, vol.boxmin, vol.boxmax, kind, ids, cells, cids[sel], ccells[sel], what="colour " + kind)
    c = _np(got[2])
    assert c is not None and c.shape == (len(got[0]), 4) and np.all(c[:, 3] == 1.0) and (c[:, 0] == 0.5).any() and (c[:, 0] != 0.5).any()
    # no colour bricks at all: every colour is 0.5
    grey = mesh.ExtractBrickMesh(dims, vol.boxmin, vol.boxmax, kind, ids, cells, np.zeros(0, np.uint32), np.zeros((0, 2048), np.uint8), indexed=True)
    assert np.array_equal(_np(grey[3]), _np(got[3])) and np.all(_np(grey[2])[:, :3] == 0.5) and np.all(_np(grey[2])[:, 3] == 1.0)


# ---- 6: many bricks: more than one brick scan block, more than one index scan block ----------------------------------------------
def test_gpu_indexed_brick_mesh_of_many_bricks_scans_across_blocks(roo):
    import torch
    dims = (16, 16, 1600)
    bmin, bmax = TB.box_of(dims, 1 / 16)
    vol = roo.BoundedVolume(*dims, bmin, bmax)
    z, y, x = torch.meshgrid(*[torch.arange(n, device="cuda", dtype=torch.float32) for n in dims[::-1]], indexing="ij")
    t = vol.tensor()
    t[..., 0] = x - 7.5 + 1.2 * torch.sin(z * (2 * np.pi / 8) + 0.3) + 0.01 * y
    t[..., 1] = 1.0
    ids, cells = roo.BrickPack(vol, NAN)
    assert ids.numel() == 800 > 256
    got, soup, val, _ = check_case(roo, dims, bmin, bmax, "f32", ids, cells, what="800 bricks")
    ci = _np(soup[3])
    bid = TB.assert_brick_order(ci, dims, TB.u32(ids))
    assert len(np.unique(bid)) == 800 and len(ci) > 256 * 3          # every brick has cubes; several blocks of 256 cubes
    assert len(got[0]) == W.count_lattice_edges(val)


# ---- 7: far inside a 4096^3 frame: ci and keys beyond 32 bits --------------------------------------------------------------------
def test_gpu_indexed_brick_mesh_far_inside_a_4096_frame(roo, sphere):
    from kangaroo_amd import mesh
    _, _, ids, cells = sphere
    off, F = 500, 4096
    idn = TB.u32(ids).astype(np.int64)
    bx, by, bz = idn % 5, (idn // 5) % 3, idn // 15
    far_ids = (((bz + off) * 512 + by + off) * 512 + bx + off).astype(np.uint32)
    box, far_box = TB.box_of(DIMS1, 2.0 ** -6), TB.box_of((F, F, F), 2.0 ** -6)
    soup = mesh.ExtractBrickMesh((F, F, F), *far_box, "f32", far_ids, cells, with_index=True)
    got = mesh.ExtractBrickMesh((F, F, F), *far_box, "f32", far_ids, cells, indexed=True)
    # no dense volume of the far frame exists: the small frame of the same voxel holds the same cells, 8 * off cells lower
    val = W.values(TB.dense_volume(roo, DIMS1, *box, "f32", ids, cells).MemcpyToHost())
    sv, sn, _, ci, to = [_np(a) for a in soup]
    assert ci.min() > 2 ** 32
    key, _ = BW.soup_keys(val, ci, to, len(sv) // 3, dims=(F, F, F), origin=(8 * off,) * 3)
    assert key.min() > 2 ** 32
    want, other = BW.weld(val, sv, sn, None, ci, to, dims=(F, F, F), origin=(8 * off,) * 3)
    assert_is_the_weld(got, want, "far frame")
    # and the small frame's indexed mesh has the same faces: the same cubes, translated
    small = mesh.ExtractBrickMesh(DIMS1, *box, "f32", ids, cells, indexed=True)
    assert np.array_equal(_np(small[3]), _np(got[3])) and len(small[0]) == len(got[0]) > 100
    err = np.abs((_np(got[0]).astype(np.float64) - 8 * off * 2.0 ** -6) - _np(small[0]).astype(np.float64)).max()
    assert err <= 8 * np.spacing(np.float32(64))


# ---- 8, 9: guards ----------------------------------------------------------------------------------------------------------------
def _frame(bmin, bmax):
    from kangaroo_amd import _lib
    frame = _lib.KfxVolume(0, None, *DIMS1[:2], 0, DIMS1[2])
    for i in range(3):
        frame.boxmin[i], frame.boxmax[i] = bmin[i], bmax[i]
    return frame


def _planned(L, frame, ids, cells, pad):
    """plan + index plan of raw lists into scratches with GUARD bytes behind them: (args of later calls, totals, V)"""
    import torch
    from kangaroo_amd import _lib, mesh
    P = lambda t: C.c_void_p(t.data_ptr())
    n = ids.numel()
    nbytes = mesh.BrickMeshScratchBytes(n)
    scratch = torch.full((nbytes + pad,), GUARD, dtype=torch.uint8, device="cuda")
    totals = (C.c_ulonglong * 2)()
    _lib.check(L.kfx_mesh_bricks_plan(C.byref(frame), 0, P(ids), P(cells), n, P(scratch), nbytes, totals, None))
    xbytes = L.kfx_mesh_bricks_index_scratch_bytes(n, totals)
    assert xbytes > 0
    xscratch = torch.full((xbytes + pad,), GUARD, dtype=torch.uint8, device="cuda")
    nv = C.c_ulonglong(0)
    _lib.check(L.kfx_mesh_bricks_index_plan(C.byref(frame), 0, P(ids), P(cells), n, P(scratch), nbytes, totals, P(xscratch), xbytes, C.byref(nv), None))
    return (scratch, nbytes, xscratch, xbytes), totals, int(nv.value)


def test_gpu_indexed_brick_mesh_writes_nothing_beyond_v_and_t_and_refuses_other_totals(roo, sphere):
    import torch
    from kangaroo_amd import _lib, mesh
    L = _lib.load()
    bmin, bmax, ids, cells = sphere
    n, frame, pad = ids.numel(), _frame(bmin, bmax), 4096
    P = lambda t: C.c_void_p(t.data_ptr())
    (scratch, nbytes, xscratch, xbytes), totals, V = _planned(L, frame, ids, cells, pad)
    na, nt = int(totals[0]), int(totals[1])
    assert na > 100 and nt >= na and V == nt // 2 + 2
    sizes = (12 * V, 12 * V, 12 * nt)
    bufs = [torch.full((size + pad,), GUARD, dtype=torch.uint8, device="cuda") for size in sizes]
    U2 = C.c_ulonglong * 2

    def emit(tot, v, xb=xbytes):
        return L.kfx_mesh_bricks_emit_indexed(C.byref(frame), 0, P(ids), P(cells), n, None, None, 0, P(scratch), nbytes, P(xscratch), xb, tot, v,
                                              P(bufs[0]), P(bufs[1]), None, P(bufs[2]), None)

    # totals or a V that are not the plans': KFX_E_RANGE after the read-back, nothing written (the index scratch is passed with its
    # slack, so that a larger layout is no reason of its own to refuse)
    for a, t, v in ((na + 1, nt, V), (na, nt - 1, V), (na - 1, nt, V), (na, nt, V + 1), (na, nt, V - 1)):
        assert emit(U2(a, t), v, xbytes + pad) == E_RANGE, (a, t, v)
        torch.cuda.synchronize()
        assert all(bool((b == GUARD).all()) for b in bufs), "a refused emit wrote something"
    nv = C.c_ulonglong(0)
    for a, t in ((na + 1, nt), (na, nt - 1)):
        assert L.kfx_mesh_bricks_index_plan(C.byref(frame), 0, P(ids), P(cells), n, P(scratch), nbytes, U2(a, t), P(xscratch), xbytes + pad,
                                            C.byref(nv), None) == E_RANGE
    torch.cuda.synchronize()
    assert bool((xscratch[xbytes:] == GUARD).all()) and bool((scratch[nbytes:] == GUARD).all())
    _lib.check(emit(totals, V))
    torch.cuda.synchronize()
    for b, size in zip(bufs, sizes):
        assert bool((b[size:] == GUARD).all()), "written beyond V or T"
    assert bool((scratch[nbytes:] == GUARD).all()) and bool((xscratch[xbytes:] == GUARD).all()), "written beyond a scratch"
    ref = mesh.ExtractBrickMesh(DIMS1, bmin, bmax, "f32", ids, cells, indexed=True)
    for b, size, r in zip(bufs, sizes, (ref[0], ref[1], ref[3])):
        assert np.array_equal(b[:size].cpu().numpy().view(np.int32), _np(r).view(np.int32).reshape(-1))
    # no bricks: an empty indexed mesh
    v, nrm, col, f = mesh.ExtractBrickMesh(DIMS1, bmin, bmax, "f32", np.zeros(0, np.uint32), np.zeros((0, 4096), np.uint8), indexed=True)
    assert v.shape == (0, 3) and nrm.shape == (0, 3) and col is None and f.shape == (0, 3)


@pytest.mark.parametrize("order", ["repeated", "reversed", "shuffled"])
def test_gpu_indexed_brick_mesh_of_unsorted_or_repeated_device_ids_stays_inside_its_buffers(roo, sphere, order):
    """test_gpu_brick_mesh.py's recipe: the mesh is unspecified, the accesses are not -- return code 0, every guard intact"""
    import torch
    from kangaroo_amd import _lib
    L = _lib.load()
    bmin, bmax, ids, cells = sphere
    n0 = ids.numel()
    if order == "repeated":
        z, y, x = torch.meshgrid(*[torch.arange(8, device="cuda")] * 3, indexing="ij")
        checker = torch.stack([1.0 - 2.0 * ((x + y + z) & 1).float(), torch.ones(8, 8, 8, device="cuda")], -1).contiguous().view(torch.uint8).reshape(1, -1)
        ids = ids.repeat_interleave(2)
        cells = torch.stack([checker.expand(n0, -1), cells], 1).reshape(2 * n0, -1).contiguous()
    else:
        perm = torch.arange(n0 - 1, -1, -1) if order == "reversed" else torch.from_numpy(np.random.default_rng(11).permutation(n0))
        ids, cells = ids[perm.cuda()].contiguous(), cells[perm.cuda()].contiguous()
    n, frame, pad = ids.numel(), _frame(bmin, bmax), 1024
    before = (ids.clone(), cells.clone())
    P = lambda t: C.c_void_p(t.data_ptr())
    (scratch, nbytes, xscratch, xbytes), totals, V = _planned(L, frame, ids, cells, pad)
    na, nt = int(totals[0]), int(totals[1])
    print("%s ids: %d entries, planned %d cubes, %d triangles, %d vertices" % (order, n, na, nt, V))
    assert nt >= na and V <= 3 * nt and (order != "repeated" or na > 100)
    sizes = (12 * V, 12 * V, 12 * nt)
    bufs = [torch.full((size + pad,), GUARD, dtype=torch.uint8, device="cuda") for size in sizes]
    _lib.check(L.kfx_mesh_bricks_emit_indexed(C.byref(frame), 0, P(ids), P(cells), n, None, None, 0, P(scratch), nbytes, P(xscratch), xbytes, totals, V,
                                              P(bufs[0]), P(bufs[1]), None, P(bufs[2]), None))
    torch.cuda.synchronize()
    for b, size in zip(bufs, sizes):
        assert bool((b[size:] == GUARD).all()), "written beyond V or T"
    assert bool((scratch[nbytes:] == GUARD).all()) and bool((xscratch[xbytes:] == GUARD).all()), "written beyond a scratch"
    assert torch.equal(ids, before[0]) and torch.equal(cells, before[1])


# ---- 10: the world mesh of a spilling pipeline, both stores ----------------------------------------------------------------------
@pytest.mark.parametrize("spill", [True, "device"])
def test_gpu_indexed_world_mesh_of_a_spilling_pipeline(roo, tmp_path, spill):
    """test_gpu_world_mesh_of_a_spilling_pipeline's set-up: 32^3, tracked, in colour, shifted by (8, 0, -8) so that the store holds bricks"""
    import torch
    from kangaroo_amd.pipeline import FramePipeline, SlabPipeline
    N, w, h = 32, 80, 60
    lo, hi = (-1.0, -1.0, 2.0), (0.9375, 0.9375, 3.9375)
    p = FramePipeline(roo, (N, N, N), lo, hi, w, h, track=True, color=True, follow=dict(quantum=8, spill=spill))
    for i in range(3):
        T_wc = scenes.orbit_pose(i, 8)
        raw = T.upload_image(roo, scenes.render_depth("room", w, h, T_wc, p.K))
        rgb = roo.Image(w, h, "u8x3").MemcpyFromHost(scenes.render_rgb("room", w, h, T_wc, p.Kimg))
        p.step(T_wc, raw, rgb)
    p.shift_volume((8, 0, -8))
    torch.cuda.synchronize()
    assert len(p.store) > 0 and len(p.cstore) > 0
    sizes = (len(p.store), p.store.nbytes, len(p.cstore), p.cstore.nbytes)
    soup = p.ExtractWorldMesh(with_index=True)
    got = p.ExtractWorldMesh(indexed=True)
    (flo, fdims, bmin, bmax, ids, cells), _ = p.world_bricks()
    assert tuple(fdims) == (40, 32, 40)
    val = W.values(TB.dense_volume(roo, fdims, bmin, bmax, "f32", ids, cells).MemcpyToHost())
    sv, sn, sc, ci, to = [_np(a) for a in soup]
    want, other = BW.weld(val, sv, sn, sc, ci, to)
    V, Tn = len(want[0]), len(want[3])
    print("world mesh (spill=%r): T = %d, V = %d, %d edges with another first cube than in dense order" % (spill, Tn, V, other))
    assert Tn > 1000 and want[2] is not None
    assert_is_the_weld(got, want, "world mesh")
    assert sizes == (len(p.store), p.store.nbytes, len(p.cstore), p.cstore.nbytes)   # the stores are as they were
    assert p.SaveWorldMesh(str(tmp_path / "world"), indexed=True) == Tn
    v, n, c, f = read_ply(str(tmp_path / "world.ply"), V, Tn, 10)
    assert np.array_equal(bits(v), bits(want[0])) and np.array_equal(bits(n), bits(want[1])) and np.array_equal(bits(c), bits(want[2]))
    assert np.array_equal(f, want[3])
    with pytest.raises(ValueError, match="with_index"):
        p.ExtractWorldMesh(with_index=True, indexed=True)
    if spill is True:   # a slab pipeline keeps refusing the world mesh, indexed or not
        s = SlabPipeline.__new__(SlabPipeline)   # (the refusal reads nothing of the pipeline)
        with pytest.raises(ValueError, match="world mesh"):
            s.ExtractWorldMesh(indexed=True)
        with pytest.raises(ValueError, match="world mesh"):
            s.SaveWorldMesh(str(tmp_path / "slab"), indexed=True)
