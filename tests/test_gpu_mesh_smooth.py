"""The mesh smoothing on the device (include/kfx_mesh_smooth.h: mesh.MeshAdjacency, SmoothMesh, VertexNormals and the smooth keyword of
the Extract and Save calls) against the numpy oracle (tests/mesh_smooth.py) -- never against the library's own output: incidence lists,
flags, smoothed positions and normals bit for bit on the hand-made cases, on random meshes around the scan block edges, on a hub that
crosses the builder's narrow / wide threshold, on the three-sphere volume, the fused colour room and a world mesh of packed bricks; a face
id >= V and adjacency arrays that are zeroed or another mesh's are refused and nothing is written; two runs give the same output bytes."""
import ctypes as C

import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import oracle

import mesh_components as MC
import mesh_simplify as MS
import mesh_smooth as SM
import test_gpu_mesh_indexed as TI

pytestmark = pytest.mark.gpu

VOXEL = 2.0 / 48   # of the three-sphere volume
ADJ_WIDE = 64      # mesh_smooth_host.h: a vertex with MORE incidences than this is ranked and flagged by a workgroup


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


def same_words(got, want, what=""):
    """a device float32 tensor against the oracle's array, word for word"""
    g, w = u32(got), np.ascontiguousarray(want, np.float32).view(np.uint32)
    assert g.shape == w.shape, what
    bad = np.flatnonzero((g != w).any(axis=1)) if g.ndim == 2 else np.flatnonzero(g != w)
    assert len(bad) == 0, (what, len(bad), bad[:5], _np(got)[bad[:5]], np.asarray(want)[bad[:5]])


def check_adjacency(faces_dev, faces, n_verts, what=""):
    """mesh.MeshAdjacency against the oracle's; returns the oracle's"""
    from kangaroo_amd import mesh
    want = SM.adjacency(n_verts, faces)
    got = mesh.MeshAdjacency(faces_dev, n_verts, with_flags=True)
    for g, w, name in zip(got, want, ("inc_start", "inc", "flags")):
        assert np.array_equal(u32(g), w), (what, name)
    plain = mesh.MeshAdjacency(faces_dev, n_verts)
    assert len(plain) == 2 and np.array_equal(u32(plain[0]), want[0]) and np.array_equal(u32(plain[1]), want[1]), what
    return want


def check_mesh(verts, faces, runs, what=""):
    """adjacency, the smoothing with each of `runs` (keywords of SM.smooth) and the normals of a host mesh against the oracle"""
    from kangaroo_amd import mesh
    dv, df = dev(verts), dev_faces(faces)
    adj = check_adjacency(df, faces, len(verts), what)
    for kw in runs:
        want = SM.smooth(verts, faces, adj=adj, **kw)
        args = dict(iterations=kw.get("iterations", 5), lam=kw.get("lam", 0.5), mu=kw.get("mu", -0.53), pin_boundary=bool(kw.get("pin_mask", 0)))
        got, norms = mesh.SmoothMesh(dv, df, normals=True, **args)
        same_words(got, want, (what, kw))
        same_words(norms, SM.vertex_normals(want, faces, adj=adj), (what, kw, "normals"))
        assert got.data_ptr() != dv.data_ptr()
    same_words(mesh.VertexNormals(dv, df), SM.vertex_normals(verts, faces, adj=adj), (what, "normals of the input"))
    return adj


TAUBIN2 = [dict(iterations=2, pin_mask=0), dict(iterations=2, pin_mask=1)]


@pytest.mark.parametrize("name", sorted(SM.HAND_MADE))
def test_gpu_hand_made_cases(roo, name):
    verts, faces, case = SM.hand_made(name)
    adj = check_mesh(verts, faces, [dict(iterations=1, mu=0.0, pin_mask=0), dict(iterations=1, mu=0.0, pin_mask=1), dict(iterations=3, pin_mask=0),
                                    dict(iterations=3, pin_mask=1), dict(iterations=0)], name)
    assert adj[0].tolist() == case["inc_start"] and adj[1].tolist() == case["inc"] and adj[2].tolist() == case["flags"]


@pytest.mark.parametrize("n_verts", [255, 256, 257])
def test_gpu_random_meshes_at_the_scan_block_edges_in_v(roo, n_verts):
    """V = 255, 256 and 257 with 400 random faces: boundary and degenerate vertices in each, unreferenced ones in the first two,
    non-manifold ones in the last"""
    verts, faces = SM.random_mesh(n_verts, 400, 100 + n_verts)
    adj = check_mesh(verts, faces, TAUBIN2, "random")
    assert all((adj[2] & bit).any() for bit in (SM.BOUNDARY, SM.DEGENERATE, SM.NONMANIFOLD if n_verts == 257 else SM.ISOLATED))


@pytest.mark.parametrize("n_faces", [85, 86, 171])
def test_gpu_random_meshes_at_the_scan_block_edges_in_t(roo, n_faces):
    """3T = 255, 258 and 513: the corner slots straddle one and two blocks of 256"""
    verts, faces = SM.random_mesh(60, n_faces, 200 + n_faces)
    adj = check_mesh(verts, faces, TAUBIN2, "random")
    assert all((adj[2] & bit).any() for bit in (SM.BOUNDARY, SM.NONMANIFOLD, SM.DEGENERATE))


def test_gpu_a_hub_of_3000_faces(roo):
    """3000 faces (i, hub, j) given in DESCENDING face order after 3000 random faces among the other vertices: the hub has 3000
    incidences, far beyond ADJ_WIDE = 64, so it is ranked and flagged by a workgroup while the others (about 6 each) go lane by lane;
    some of the others cross 64 too, on a second mesh.  The hub's list must ascend, and one pass is a 6000-term sum in fixed order."""
    rng = np.random.RandomState(3)
    n, hub = 3001, 1500
    others = np.array([v for v in range(n) if v != hub])
    verts = rng.rand(n, 3).astype(np.float32)
    rand = others[rng.randint(0, n - 1, size=(3000, 3))]
    spokes = np.stack([others[rng.randint(0, n - 1, 3000)], np.full(3000, hub), others[rng.randint(0, n - 1, 3000)]], axis=1)
    order = np.argsort(-spokes[:, 0], kind="stable")   # (descending in the first corner: the slots arrive in no helpful order)
    faces = np.concatenate([rand, spokes[order]]).astype(np.uint32)
    adj = check_mesh(verts, faces, [dict(iterations=1, mu=0.0, pin_mask=0), dict(iterations=1, pin_mask=1)], "hub")
    start, inc, flags = adj
    seg = inc[start[hub]:start[hub + 1]].astype(np.int64)
    assert len(seg) == 3000 > ADJ_WIDE and (np.diff(seg) > 0).all() and seg[0] == 3 * 3000 + 1
    deg = np.diff(start.astype(np.int64))
    assert deg[others].max() <= ADJ_WIDE          # every other vertex takes the narrow path
    assert flags[hub] & SM.BOUNDARY and not flags[hub] & SM.DEGENERATE
    # the threshold itself: vertices with exactly 64, 65 and 66 incidences in one mesh
    f2 = []
    for v, d in ((0, 64), (1, 65), (2, 66)):
        f2 += [[v, 3 + (7 * k) % 200, 3 + (11 * k + 1) % 200] for k in range(d)]
    f2 = np.asarray(f2[::-1], np.uint32)
    v2 = rng.rand(203, 3).astype(np.float32)
    adj = check_mesh(v2, f2, [dict(iterations=1, pin_mask=0)], "threshold")
    assert np.diff(adj[0].astype(np.int64))[:3].tolist() == [64, 65, 66]


@pytest.fixture(scope="module")
def three_spheres(roo):
    """the three-sphere volume at 48^3: its indexed mesh on the device, and the oracle's weld of the oracle's soup"""
    from kangaroo_amd import mesh
    ovol = MC.three_spheres(oracle)
    vol = TI.upload(roo, ovol)
    want = TI.expected(ovol)
    got = mesh.ExtractMesh(vol, indexed=True)
    TI.check(got, want, "three spheres")
    host = (want[0], want[1], None, want[3])
    return ovol, vol, got, host, SM.adjacency(len(want[0]), want[3])


def want_smoothed(host, adj=None, **kw):
    """the oracle's (verts, norms, colors, faces) of a mesh after smooth= with SmoothMesh's defaults: the boundary pinned"""
    verts, norms, colors, faces = host
    adj = adj if adj is not None else SM.adjacency(len(verts), faces)
    out = SM.smooth(verts, faces, adj=adj, iterations=kw.get("iterations", 5), lam=kw.get("lam", 0.5), mu=kw.get("mu", -0.53),
                    pin_mask=1 if kw.get("pin_boundary", True) else 0)
    return out, SM.vertex_normals(out, faces, adj=adj), colors, faces


def assert_mesh(got, want, what=""):
    same_words(got[0], want[0], (what, "verts"))
    same_words(got[1], want[1], (what, "norms"))
    assert (got[2] is None) == (want[2] is None), what
    if want[2] is not None:
        same_words(got[2], want[2], (what, "colours"))
    assert np.array_equal(u32(got[3]), want[3]), what


@pytest.mark.parametrize("iterations", [0, 1, 5])
def test_gpu_three_spheres(roo, three_spheres, iterations):
    """V = 2480, T = 4948, closed: adjacency, 0 / 1 / 5 iterations with nothing pinned and with the boundary pinned, the normals of the
    smoothed positions, and the keyword of ExtractMesh"""
    from kangaroo_amd import mesh
    ovol, vol, got, host, adj = three_spheres
    assert (len(host[0]), len(host[3])) == (2480, 4948) and not adj[2].any()
    if iterations == 0:
        check_adjacency(got[3], host[3], 2480, "three spheres")
        same_words(mesh.VertexNormals(got[0], got[3]), SM.vertex_normals(host[0], host[3], adj=adj), "normals of the input")
    for pin in (0, 1):
        want = SM.smooth(host[0], host[3], iterations=iterations, pin_mask=pin, adj=adj)
        out, norms = mesh.SmoothMesh(got[0], got[3], iterations=iterations, pin_boundary=bool(pin), normals=True)
        same_words(out, want, ("three spheres", iterations, pin))
        same_words(norms, SM.vertex_normals(want, host[3], adj=adj), ("three spheres, normals", iterations, pin))
        assert (iterations == 0) == np.array_equal(want.view(np.uint32), host[0].view(np.uint32))
    assert_mesh(mesh.ExtractMesh(vol, indexed=True, smooth=iterations), want_smoothed(host, adj, iterations=iterations), "ExtractMesh")


def test_gpu_keyword_forms_and_refusals(roo, three_spheres, tmp_path):
    from kangaroo_amd import mesh
    ovol, vol, got, host, adj = three_spheres
    kw = dict(iterations=2, lam=0.25, mu=0.0, pin_boundary=False)
    assert_mesh(mesh.ExtractMesh(vol, indexed=True, smooth=kw), want_smoothed(host, adj, **kw), "a dict")
    TI.check(mesh.ExtractMesh(vol, indexed=True, smooth=None), TI.expected(ovol), "off")
    for bad in (dict(smooth=3), dict(indexed=True, smooth=3, slab=(48, 0, -1.0, 1.0, 0, 48)), dict(indexed=True, smooth=dict(rounds=3)),
                dict(indexed=True, smooth=-1), dict(indexed=True, smooth=0.5), dict(indexed=True, smooth=True)):
        with pytest.raises(ValueError):
            mesh.ExtractMesh(vol, **bad)
    for bad in (dict(lam=0.0), dict(lam=1.5), dict(mu=0.1), dict(lam=float("nan")), dict(iterations=-1)):
        with pytest.raises(Exception):
            mesh.SmoothMesh(got[0], got[3], **bad)
    # after the filter and the simplification
    cell = 2 * VOXEL
    simple = MS.simplify(*MC.filter_mesh(*host, min_faces=1000), cell)[:4]
    assert_mesh(mesh.ExtractMesh(vol, indexed=True, min_faces=1000, simplify_cell=cell, smooth=3), want_smoothed(simple, iterations=3), "after both")
    # the file
    want = want_smoothed(host, adj, iterations=2)
    assert mesh.SaveMesh(str(tmp_path / "m"), vol, indexed=True, smooth=2) == 4948
    size, head, nv, nf, table, rows = TI.read_ply(str(tmp_path / "m.ply"))
    assert (nv, nf) == (2480, 4948) and np.array_equal(table[:, :3].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(table[:, 3:].view(np.uint32), want[1].view(np.uint32)) and np.array_equal(rows["i"], want[3])
    with pytest.raises(ValueError):
        mesh.SaveMesh(str(tmp_path / "n"), vol, smooth=2)


def test_gpu_fused_colour_room(roo):
    """the fused colour room at 64^3 (V = 18 233, T = 32 994), an open surface with floaters: positions and normals are the oracle's, the
    colours are untouched"""
    from kangaroo_amd import mesh
    ovol, ocvol, _ = TI.f32_case("fused_room_colour")
    vol, cvol = TI.upload(roo, ovol), TI.upload(roo, ocvol, kind="c32")
    host = TI.expected(ovol, ocvol)
    adj = SM.adjacency(len(host[0]), host[3])
    assert host[2] is not None and (adj[2] & SM.BOUNDARY).any()
    got = mesh.ExtractMesh(vol, cvol, indexed=True)
    check_adjacency(got[3], host[3], len(host[0]), "colour room")
    for kw in (dict(iterations=3), dict(iterations=2, pin_boundary=False)):
        want = want_smoothed(host, adj, **kw)
        assert (want[0] != host[0]).any()
        assert_mesh(mesh.ExtractMesh(vol, cvol, indexed=True, smooth=kw), want, ("colour room", kw))
    cell = 2 * 2.0 / 64
    simple = MS.simplify(*host, cell)[:4]
    assert_mesh(mesh.ExtractMesh(vol, cvol, indexed=True, simplify_cell=cell, smooth=2), want_smoothed(simple, iterations=2), "simplify, then smooth")


@pytest.mark.parametrize("spill", [True, "device"])
def test_gpu_world_mesh_of_a_spilling_pipeline(roo, tmp_path, spill):
    """a 32^3 tracked colour pipeline shifted by (8, 0, -8) so that the store holds bricks, both stores:
    ExtractWorldMesh / SaveWorldMesh(indexed=True, smooth=) is the oracle's smoothing of the plain indexed world mesh, colours untouched;
    after simplify_cell= it is the oracle's simplification followed by the oracle's smoothing; a slab pipeline refuses the keyword"""
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
    assert host[2] is not None
    want = want_smoothed(host, iterations=3)
    assert_mesh(p.ExtractWorldMesh(indexed=True, smooth=3), want, "world mesh")
    cell = 2 * (0.9375 + 1.0) / N
    simple = MS.simplify(*MC.filter_mesh(*host, min_faces=20), cell)[:4]
    assert_mesh(p.ExtractWorldMesh(indexed=True, min_faces=20, simplify_cell=cell, smooth=dict(iterations=2, pin_boundary=False)),
                want_smoothed(simple, iterations=2, pin_boundary=False), "world mesh, filtered and simplified")
    assert p.SaveWorldMesh(str(tmp_path / "world"), indexed=True, smooth=3) == len(want[3])
    size, head, nv, nf, table, rows = TI.read_ply(str(tmp_path / "world.ply"))
    assert np.array_equal(table[:, :3].view(np.uint32), want[0].view(np.uint32))
    with pytest.raises(ValueError, match="indexed"):
        p.ExtractWorldMesh(smooth=3)
    if spill is True:
        s = SlabPipeline.__new__(SlabPipeline)   # (the refusal reads nothing of the pipeline)
        with pytest.raises(ValueError, match="welded within its rank"):
            s.ExtractMesh(indexed=True, smooth=3)


def test_gpu_refusals_leave_the_outputs_untouched(roo, three_spheres):
    """a face list that contains the id V: the first kernel of each call reads `faces` alone and raises the error word, every later kernel
    tests it first, the call returns KFX_E_RANGE and the outputs, pre-filled with a pattern, are untouched.  The smoothing and the
    normals carry no state in their scratch -- what they take from an earlier call is the adjacency, and adjacency arrays that are
    zeroed, or another mesh's, are refused the same way; a scratch full of zeros or of another call's bytes changes nothing."""
    import torch
    from kangaroo_amd import _lib, mesh
    L = _lib.load()
    ovol, vol, got, host, adj = three_spheres
    V, Tn = 2480, 4948
    ptr = lambda t: C.c_void_p(t.data_ptr())
    start, inc, flags = mesh.MeshAdjacency(got[3], V, with_flags=True)
    nbytes = {"adj": L.kfx_mesh_adjacency_scratch_bytes(V, Tn), "smooth": L.kfx_mesh_smooth_scratch_bytes(V, Tn), "normals": 256}
    scratch = torch.zeros(max(nbytes.values()), dtype=torch.uint8, device="cuda")
    out = torch.full((V, 3), -7.0, dtype=torch.float32, device="cuda")
    o_start = torch.full((V + 1,), -7, dtype=torch.int32, device="cuda")
    o_inc = torch.full((3 * Tn,), -7, dtype=torch.int32, device="cuda")
    o_flags = torch.full((V,), -7, dtype=torch.int32, device="cuda")

    def call_adj(faces):
        return L.kfx_mesh_adjacency(ptr(faces), Tn, V, ptr(o_start), ptr(o_inc), ptr(o_flags), ptr(scratch), nbytes["adj"], None)

    def call_smooth(faces, s=start, i=inc, f=flags, sc=scratch):
        return L.kfx_mesh_smooth(ptr(got[0]), ptr(faces), Tn, V, ptr(s), ptr(i), ptr(f), 2, 0.5, -0.53, 1, ptr(out), ptr(sc), nbytes["smooth"], None)

    def call_normals(faces, s=start, i=inc):
        return L.kfx_mesh_vertex_normals(ptr(got[0]), ptr(faces), Tn, V, ptr(s), ptr(i), ptr(out), ptr(scratch), 256, None)

    def untouched():
        torch.cuda.synchronize()
        return bool((out == -7.0).all()) and bool((o_start == -7).all()) and bool((o_inc == -7).all()) and bool((o_flags == -7).all())

    for at in (0, 3 * 2000 + 1, 3 * Tn - 1):
        faces = got[3].clone()
        faces.view(-1)[at] = V
        for call in (call_adj, call_smooth, call_normals):
            assert call(faces) == -4, (at, call.__name__)
            assert b"face id" in L.kfx_last_error_string()
        assert untouched(), at
    # the adjacency of nothing, and of another mesh with the same V and T: the faces in reverse order
    zeros = (torch.zeros_like(start), torch.zeros_like(inc))
    other = mesh.MeshAdjacency(torch.flip(got[3], [0]).contiguous(), V)
    assert call_smooth(got[3], s=zeros[0], i=zeros[1]) == -4 and b"adjacency" in L.kfx_last_error_string()
    assert call_normals(got[3], s=zeros[0], i=zeros[1]) == -4
    assert call_smooth(got[3], s=other[0], i=other[1]) == -4
    big = inc.clone()
    big[17] = 3 * Tn
    assert call_smooth(got[3], i=big) == -4 and call_normals(got[3], i=big) == -4
    down = start.clone()
    down[100] = down[101] + 1
    assert call_smooth(got[3], s=down) == -4 and call_normals(got[3], s=down) == -4
    assert untouched()
    # ... and the same calls with the mesh's own arrays are accepted, whatever the scratch held before
    want = SM.smooth(host[0], host[3], iterations=2, pin_mask=1, adj=adj)
    foreign = torch.full_like(scratch, 0x5a)
    _lib.check(L.kfx_mesh_adjacency(ptr(got[3]), Tn, V, ptr(o_start), ptr(o_inc), ptr(o_flags), ptr(foreign), nbytes["adj"], None))
    for sc in (scratch.zero_(), foreign):
        out.fill_(-7.0)
        assert call_smooth(got[3], sc=sc) == 0
        same_words(out, want, "after the refusals")
    assert call_adj(got[3]) == 0
    assert np.array_equal(u32(o_start), adj[0]) and np.array_equal(u32(o_inc), adj[1]) and np.array_equal(u32(o_flags), adj[2])


def test_gpu_two_runs_give_identical_output_bytes(roo):
    """a random mesh of 20 000 vertices and 40 000 faces twice, the second time on a scratch full of other bytes: every output byte equal
    (the scratch is exempt: where the fill puts a slot depends on arrival)"""
    import torch
    from kangaroo_amd import mesh
    verts, faces = SM.random_mesh(20000, 40000, 5)
    dv, df = dev(verts), dev_faces(faces)
    first = mesh.MeshAdjacency(df, 20000, with_flags=True) + mesh.SmoothMesh(dv, df, iterations=3, normals=True)
    junk = torch.full((1 << 22,), 0x5a, dtype=torch.uint8, device="cuda")   # (what the allocator hands out next)
    del junk
    second = mesh.MeshAdjacency(df, 20000, with_flags=True) + mesh.SmoothMesh(dv, df, iterations=3, normals=True)
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    adj = SM.adjacency(20000, faces)
    for g, w in zip(first[:3], adj):
        assert np.array_equal(u32(g), w)
    same_words(first[3], SM.smooth(verts, faces, iterations=3, pin_mask=1, adj=adj), "random, 3 iterations")
