"""The mesh simplification on the device (include/kfx_mesh_simplify.h: mesh.SimplifyMesh and the simplify_cell keyword of the Extract
and Save calls) against the numpy oracle (tests/mesh_simplify.py) -- never against the library's own output: vertices, normals,
colours, faces and the vertex map bit for bit on the hand-made cases, on random meshes around the scan block edges, with many keys and
with one hot word, on the three-sphere volume, the fused colour room and a world mesh of packed bricks; a face id >= V, a zeroed or
foreign scratch and wrong counts are refused and nothing is written; two runs give the same output bytes."""
import ctypes as C

import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import oracle

import mesh_components as MC
import mesh_simplify as MS
import test_gpu_mesh_indexed as TI

pytestmark = pytest.mark.gpu

VOXEL = 2.0 / 48   # of the three-sphere volume


def _np(t):
    return None if t is None else t.cpu().numpy()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_faces(faces):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(faces, np.uint32).reshape(-1, 3)).view(np.int32)).cuda()


def assert_same(got, want, what=""):
    """device (verts, norms, colors, faces[, map]) against the oracle's, bit for bit"""
    for g, w in zip(got[:3], want[:3]):
        assert (g is None) == (w is None), what
        if w is not None:
            assert tuple(g.shape) == w.shape and T.nan_equal(_np(g).view(np.uint32), np.asarray(w).view(np.uint32)), what
    assert tuple(got[3].shape) == want[3].shape and np.array_equal(u32(got[3]), want[3]), what
    if len(got) > 4:
        assert np.array_equal(u32(got[4]), want[4]), what


def check_simplify(arrays, host, cell, origin=(0.0, 0.0, 0.0), what=""):
    """mesh.SimplifyMesh of device arrays against the oracle on their host copies; returns the oracle's"""
    from kangaroo_amd import mesh
    got = mesh.SimplifyMesh(*arrays, cell=cell, origin=origin, with_map=True)
    want = MS.simplify(*host, cell, origin)
    assert_same(got, want, (what, cell, origin))
    assert MS.properties(want)
    return want


def check_host_mesh(verts, faces, cell, origin=(0.0, 0.0, 0.0), what=""):
    """... of a host mesh, with rows of normals and colours that tell every vertex and word apart"""
    n = len(verts)
    norms = -np.arange(3 * n, dtype=np.float32).reshape(n, 3) - 1
    cols = np.arange(4 * n, dtype=np.float32).reshape(n, 4) + 0.5
    host = (verts, norms, cols, faces)
    return check_simplify((dev(verts), dev(norms), dev(cols), dev_faces(faces)), host, cell, origin, what)


@pytest.mark.parametrize("name", sorted(MS.HAND_MADE))
def test_gpu_hand_made_cases(roo, name):
    verts, faces, cell, origin, nv, nt, want_faces, vmap = MS.hand_made(name)
    want = check_host_mesh(verts, faces, cell, origin, name)
    assert (len(want[0]), len(want[3])) == (nv, nt) and np.array_equal(want[3], want_faces) and np.array_equal(want[4], vmap)


@pytest.mark.parametrize("n_verts", [255, 256, 257])
def test_gpu_random_meshes_at_the_scan_block_edges(roo, n_verts):
    """V = 255, 256 and 257 random vertices over 5^3 cells with random faces, and the same with the grid anchored elsewhere"""
    verts, faces, cell = MS.random_mesh(n_verts, 400, 5, 100 + n_verts)
    want = check_host_mesh(verts, faces, cell, what="random")
    assert 0 < len(want[3]) < 400 and 0 < len(want[0]) <= 125
    check_host_mesh(verts, faces, cell, origin=(0.013, -0.4, 7.0), what="random, anchored elsewhere")
    check_host_mesh(verts - np.float32(0.5), faces, cell, what="random, around the origin")   # negative cells


def test_gpu_many_keys_and_long_probe_runs(roo):
    """20 000 random vertices over 17^3 cells with 40 000 random faces: nearly every cell is a key, nearly every face a key of its own"""
    verts, faces, cell = MS.random_mesh(20000, 40000, 17, 5)
    want = check_host_mesh(verts, faces, cell, what="many keys")
    assert 4000 < len(want[0]) <= 17 ** 3 and 39000 < len(want[3]) < 40000


def test_gpu_every_minimum_on_one_word(roo):
    """5 000 vertices all in one cell -- every minimum lands on one word -- and two vertices in cells of their own: of the faces
    (i, 5000, 5001) the first survives, with the representative of the 5 000: the one nearest the centre"""
    rng = np.random.RandomState(7)
    verts = np.concatenate([rng.rand(5000, 3), [[1.5, 0.5, 0.5], [0.5, 1.5, 0.5]]]).astype(np.float32)
    verts[[1234, 4321]] = verts[77]   # three vertices with one d2: the tie goes to the smallest id, whatever it is
    faces = np.stack([rng.randint(0, 5000, 3000), rng.randint(0, 5000, 3000), rng.randint(0, 5000, 3000)], axis=1)
    faces = np.concatenate([faces, np.stack([np.arange(5000), np.full(5000, 5000), np.full(5000, 5001)], axis=1)[::-1]]).astype(np.uint32)
    want = check_host_mesh(verts, faces, 1.0, what="one cell")
    rep, _, d2 = MS.clusters(verts, 1.0)
    assert len(set(rep[:5000].tolist())) == 1 and d2[rep[0]] == d2[:5000].min()
    assert (len(want[0]), len(want[3])) == (3, 1)
    # ... and with the tie at the minimum itself
    verts[[1234, 4321]] = verts[rep[0]]
    want = check_host_mesh(verts, faces, 1.0, what="one cell, a tie at the minimum")
    assert MS.clusters(verts, 1.0)[0][0] == min(rep[0], 1234)


@pytest.fixture(scope="module")
def three_spheres(roo):
    """the three-sphere volume at 48^3: its indexed mesh on the device, and the oracle's weld of the oracle's soup"""
    from kangaroo_amd import mesh
    ovol = MC.three_spheres(oracle)
    vol = TI.upload(roo, ovol)
    want = TI.expected(ovol)
    got = mesh.ExtractMesh(vol, indexed=True)
    TI.check(got, want, "three spheres")
    return ovol, vol, got, (want[0], want[1], None, want[3])


@pytest.mark.parametrize("cells", [2, 4, 1.0 / 1024])
def test_gpu_three_spheres(roo, three_spheres, cells):
    """V = 2480, T = 4948 at cells of 2 and 4 voxel sizes (T' = 1006 and 288) and at 1/1024 of one, where every vertex has a cell of its
    own and the output is the input bit for bit; the output's properties checked on the device's arrays directly"""
    from kangaroo_amd import mesh
    ovol, vol, got, host = three_spheres
    V, Tn = len(host[0]), len(host[3])
    assert (V, Tn) == (2480, 4948)
    want = check_simplify(got, host, cells * VOXEL, what="three spheres")
    if cells >= 1:
        assert 0 < len(want[3]) < Tn and 0 < len(want[0]) < V
    else:
        assert MS.is_identity(host[0], host[3], want) and np.array_equal(want[4], np.arange(V))
    out = mesh.SimplifyMesh(*got, cell=cells * VOXEL)
    f, nv = u32(out[3]).astype(np.int64), len(out[0])
    assert len(out) == 4 and out[2] is None and tuple(out[1].shape) == (nv, 3)
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all()             # three distinct ids per face
    assert len(np.unique(np.sort(f, axis=1), axis=0)) == len(f)                                    # no two faces with one id set
    assert f.max() == nv - 1 and len(np.unique(f)) == nv                                           # every vertex referenced
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(out, got) if a is not None)
    # the keyword of ExtractMesh: after the filter
    kw = dict(min_faces=1000)
    filtered = MC.filter_mesh(*host, **kw)
    assert_same(mesh.ExtractMesh(vol, indexed=True, simplify_cell=cells * VOXEL, **kw), MS.simplify(*filtered, cells * VOXEL), "ExtractMesh")
    assert_same(mesh.ExtractMesh(vol, indexed=True, simplify_cell=cells * VOXEL), want[:4], "ExtractMesh, no filter")


def test_gpu_keyword_needs_an_indexed_mesh_of_a_whole_volume(roo, three_spheres):
    from kangaroo_amd import mesh
    ovol, vol, got, host = three_spheres
    for kw in (dict(simplify_cell=0.1), dict(indexed=True, simplify_cell=0.1, slab=(48, 0, -1.0, 1.0, 0, 48))):
        with pytest.raises(ValueError):
            mesh.ExtractMesh(vol, **kw)
    for bad in (0.0 - 1.0, float("nan"), float("inf")):
        with pytest.raises(Exception):
            mesh.SimplifyMesh(*got, cell=bad)
    assert_same(mesh.ExtractMesh(vol, indexed=True, simplify_cell=None), host, "off")
    assert_same(mesh.ExtractMesh(vol, indexed=True, simplify_cell=0), host, "off")


def test_gpu_save_mesh_with_a_cell(roo, three_spheres, tmp_path):
    from kangaroo_amd import mesh
    ovol, vol, got, host = three_spheres
    want = MS.simplify(*host, 2 * VOXEL)
    assert mesh.SaveMesh(str(tmp_path / "m"), vol, indexed=True, simplify_cell=2 * VOXEL) == len(want[3]) == 1006
    size, head, nv, nf, table, rows = TI.read_ply(str(tmp_path / "m.ply"))
    assert (nv, nf) == (len(want[0]), 1006) and T.nan_equal(table[:, :3], want[0]) and T.nan_equal(table[:, 3:], want[1])
    assert np.array_equal(rows["i"], want[3])
    with pytest.raises(ValueError):
        mesh.SaveMesh(str(tmp_path / "n"), vol, simplify_cell=2 * VOXEL)


def test_gpu_fused_colour_room(roo):
    """the fused colour room at 64^3 (V = 18 233, T = 32 994) at 2 voxel sizes: with normals and colours, with a colour array on 4-byte
    alignment only (the word path), and with positions alone"""
    import torch
    from kangaroo_amd import mesh
    ovol, ocvol, _ = TI.f32_case("fused_room_colour")
    vol, cvol = TI.upload(roo, ovol), TI.upload(roo, ocvol, kind="c32")
    host = TI.expected(ovol, ocvol)
    got = mesh.ExtractMesh(vol, cvol, indexed=True)
    TI.check(got, host, "colour room")
    assert host[2] is not None
    cell = 2 * 2.0 / 64
    want = check_simplify(got, host, cell, what="colour room")
    assert 0 < len(want[3]) < len(host[3]) and want[2].shape == (len(want[0]), 4)
    pad = torch.empty(4 * len(host[0]) + 1, dtype=torch.float32, device="cuda")
    odd = pad[1:].view(-1, 4)
    odd.copy_(got[2])
    assert odd.data_ptr() % 16 == 4
    check_simplify((got[0], got[1], odd, got[3]), host, cell, what="unaligned colours")
    check_simplify((got[0], None, None, got[3]), (host[0], None, None, host[3]), cell, what="positions alone")
    assert_same(mesh.ExtractMesh(vol, cvol, indexed=True, simplify_cell=cell), want[:4], "ExtractMesh(colour)")


def test_gpu_world_mesh_of_bricks_with_one_gone(roo):
    """the three-sphere volume packed into bricks, without the brick that holds the +x cap of the first sphere:
    ExtractBrickMesh(indexed=True, min_faces=, simplify_cell=) equals the oracle's filter followed by the oracle's simplification of
    the unfiltered ExtractBrickMesh(indexed=True) arrays"""
    import torch
    import test_gpu_brick_mesh as TB
    from kangaroo_amd import mesh
    ovol = MC.three_spheres(oracle)
    vol = TI.upload(roo, ovol)
    ids, cells = roo.BrickPack(vol, float("nan"))
    idn = TB.u32(ids).astype(np.int64)
    gone = (2 * 6 + 2) * 6 + 2   # brick (2, 2, 2) of 6 x 6 x 6
    assert gone in idn
    sel = torch.from_numpy(np.nonzero(idn != gone)[0]).cuda()
    args = ((48, 48, 48), vol.boxmin, vol.boxmax, "f32", ids[sel], cells[sel])
    full = mesh.ExtractBrickMesh(*args, indexed=True)
    host = (_np(full[0]), _np(full[1]), None, u32(full[3]))
    assert 4000 < len(host[3]) < 4948
    for min_faces, cell in ((133, 2 * VOXEL), (1000, 4 * VOXEL), (0, 2 * VOXEL)):
        want = MS.simplify(*MC.filter_mesh(*host, min_faces=min_faces), cell)
        assert 0 < len(want[3]) < len(host[3])
        assert_same(mesh.ExtractBrickMesh(*args, indexed=True, min_faces=min_faces, simplify_cell=cell), want, (min_faces, cell))
    with pytest.raises(ValueError):
        mesh.ExtractBrickMesh(*args, simplify_cell=2 * VOXEL)


def _plan(L, verts, faces, cell, V=None, zero=True):
    import torch
    V, Tn = len(verts) if V is None else V, len(faces)
    nbytes = L.kfx_mesh_simplify_scratch_bytes(V, Tn)
    scratch = (torch.zeros if zero else torch.empty)(nbytes, dtype=torch.uint8, device="cuda")
    kept = (C.c_ulonglong * 2)(5, 5)
    code = L.kfx_mesh_simplify_plan(C.c_void_p(verts.data_ptr()), C.c_void_p(faces.data_ptr()), Tn, V, (C.c_float * 3)(0, 0, 0), cell,
                                    C.c_void_p(scratch.data_ptr()), nbytes, kept, None)
    return code, scratch, nbytes, kept


def test_gpu_a_face_id_of_v_is_refused_and_nothing_is_written(roo, three_spheres):
    """a face list that contains the id V: the plan's first kernel reads `faces` alone and raises the error word, every later kernel
    tests it first, the plan returns KFX_E_RANGE, and the emit on that scratch is refused with the outputs untouched; so are a zeroed
    scratch, the scratch of another call, and counts that are not the plan's"""
    import torch
    from kangaroo_amd import _lib
    L = _lib.load()
    ovol, vol, got, host = three_spheres
    V, Tn = len(host[0]), len(host[3])
    ptr = lambda t: C.c_void_p(t.data_ptr())
    cell = 2 * VOXEL
    out = torch.full((V, 3), -7.0, dtype=torch.float32, device="cuda")
    fout = torch.full((Tn, 3), -7, dtype=torch.int32, device="cuda")
    vmap = torch.full((V,), -7, dtype=torch.int32, device="cuda")

    def emit(scratch, nbytes, kept, v=V):
        return L.kfx_mesh_simplify_emit(ptr(scratch), nbytes, v, Tn, kept, ptr(got[0]), None, None, ptr(got[3]), ptr(out), None, None, ptr(fout),
                                        ptr(vmap), None)

    for at in (0, 3 * 2000 + 1, 3 * Tn - 1):
        faces = got[3].clone()
        faces.view(-1)[at] = V
        code, scratch, nbytes, kept = _plan(L, got[0], faces, cell)
        assert code == -4 and (kept[0], kept[1]) == (0, 0), at
        assert b"face id" in L.kfx_last_error_string()
        words = scratch[:256].cpu().numpy().view(np.uint64)
        assert words[3] == 0 and words[4] == 1   # no stage reached; the error word
        # nothing indexed by a face id was written: rep[], used[], remap[] and fkeep[] are as the zeroed scratch and the init left them
        at_rep = 256 + 8 * 8192 + 4 * 16384
        assert not scratch[at_rep:].any()
        assert emit(scratch, nbytes, (C.c_ulonglong * 2)(509, 1006)) == -4
    want = MS.simplify(*host, cell)
    zero = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    assert emit(zero, nbytes, (C.c_ulonglong * 2)(509, 1006)) == -4
    # a foreign scratch: the clean-up's plan of the same mesh
    cbytes = L.kfx_mesh_components_scratch_bytes(V, Tn)
    foreign = torch.zeros(max(cbytes, nbytes), dtype=torch.uint8, device="cuda")
    counts = (C.c_ulonglong * 2)()
    _lib.check(L.kfx_mesh_components_plan(ptr(got[3]), Tn, V, ptr(foreign), cbytes, counts, None))
    assert emit(foreign, nbytes, (C.c_ulonglong * 2)(509, 1006)) == -4
    # a plan of this mesh: other counts, another V
    code, scratch, nbytes, kept = _plan(L, got[0], got[3], cell)
    assert code == 0 and (kept[0], kept[1]) == (len(want[0]), len(want[3])) == (509, 1006)
    assert emit(scratch, nbytes, (C.c_ulonglong * 2)(509, 1005)) == -4 and emit(scratch, nbytes, (C.c_ulonglong * 2)(508, 1006)) == -4
    big = torch.zeros(nbytes + (1 << 20), dtype=torch.uint8, device="cuda")
    big[:nbytes] = scratch
    assert emit(big, nbytes + (1 << 20), kept, v=V + 1) == -4
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((fout == -7).all()) and bool((vmap == -7).all())
    # ... and the plan's own counts are accepted: nothing beyond V' and T' is written
    assert emit(scratch, nbytes, kept) == 0
    torch.cuda.synchronize()
    assert_same((out[:509], None, None, fout[:1006], vmap), (want[0], None, None, want[3], want[4]), "after the refusals")
    assert bool((out[509:] == -7.0).all()) and bool((fout[1006:] == -7).all())


def test_gpu_two_runs_give_identical_output_bytes(roo):
    """the many-keys mesh twice, the second time on a scratch full of other bytes: every output byte equal (the scratch is exempt: the
    slot a key ends in depends on arrival)"""
    import torch
    from kangaroo_amd import mesh
    verts, faces, cell = MS.random_mesh(20000, 40000, 17, 5)
    arrays = (dev(verts), dev(-verts), None, dev_faces(faces))
    first = mesh.SimplifyMesh(*arrays, cell=cell, with_map=True)
    junk = torch.full((1 << 22,), 0x5a, dtype=torch.uint8, device="cuda")   # (what the allocator hands out next)
    del junk
    second = mesh.SimplifyMesh(*arrays, cell=cell, with_map=True)
    for a, b in zip(first, second):
        assert (a is None and b is None) or torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("spill", [True, "device"])
def test_gpu_world_mesh_of_a_spilling_pipeline(roo, tmp_path, spill):
    """a 32^3 tracked colour pipeline shifted by (8, 0, -8) so that the store holds bricks, both stores:
    ExtractWorldMesh / SaveWorldMesh(indexed=True, min_faces=, simplify_cell=) is the oracle's filter followed by the oracle's
    simplification, anchored at the world origin, of the plain indexed world mesh; a slab pipeline refuses the keyword"""
    import torch
    from kangaroo_amd import scenes
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
    assert len(p.store) > 0
    full = p.ExtractWorldMesh(indexed=True)
    host = (_np(full[0]), _np(full[1]), _np(full[2]), u32(full[3]))
    cell = 2 * (0.9375 + 1.0) / N
    want = MS.simplify(*host, cell)[:4]
    assert 0 < len(want[3]) < len(host[3]) and want[2] is not None
    assert_same(p.ExtractWorldMesh(indexed=True, simplify_cell=cell), want, "world mesh")
    both = MS.simplify(*MC.filter_mesh(*host, min_faces=20), cell)[:4]
    assert_same(p.ExtractWorldMesh(indexed=True, min_faces=20, simplify_cell=cell), both, "world mesh, filtered")
    assert p.SaveWorldMesh(str(tmp_path / "world"), indexed=True, simplify_cell=cell) == len(want[3])
    head = open(str(tmp_path / "world.ply"), "rb").read(600).decode("latin1")
    assert "element vertex %d\n" % len(want[0]) in head and "element face %d\n" % len(want[3]) in head
    with pytest.raises(ValueError, match="indexed"):
        p.ExtractWorldMesh(simplify_cell=cell)
    if spill is True:
        s = SlabPipeline.__new__(SlabPipeline)   # (the refusal reads nothing of the pipeline)
        with pytest.raises(ValueError):
            s.ExtractMesh(indexed=True, simplify_cell=cell)
