"""The mesh clean-up on the device (include/kfx_mesh_clean.h: mesh.MeshComponents, mesh.FilterMesh and the min_faces / largest keywords
of the Extract calls) against the numpy oracle (tests/mesh_components.py) -- never against the library's own output: labels, face
counts and the filtered arrays bit for bit on hand-made face lists (long paths, deep trees, one hot word), on the three-sphere volume,
the ragged NaN-lattice volume, the fused colour room and a world mesh of packed bricks; a face id >= V is refused and nothing is
written; a filter re-planned on one scratch equals a fresh run."""
import ctypes as C

import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import oracle

import mesh_components as MC
import mesh_weld as W
import test_gpu_mesh_indexed as TI

pytestmark = pytest.mark.gpu


def _np(t):
    return None if t is None else t.cpu().numpy()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def dev_faces(faces):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(faces, np.uint32).reshape(-1, 3)).view(np.int32)).cuda()


def check_components(faces, n, want=None):
    """mesh.MeshComponents of a host face list against the oracle (and the known answer, where there is one)"""
    from kangaroo_amd import mesh
    vc, cf = mesh.MeshComponents(dev_faces(faces), n)
    wvc, wcf = MC.components(faces, n)
    assert np.array_equal(u32(vc), wvc) and np.array_equal(u32(cf), wcf)
    if want is not None:
        assert wvc.tolist() == want[0] and wcf.tolist() == want[1]
    return wvc, wcf


def check_filter(arrays, host, min_faces=0, largest=False, what=""):
    """mesh.FilterMesh of device arrays against the oracle's selection of their host copies, bit for bit; returns the oracle's"""
    from kangaroo_amd import mesh
    got = mesh.FilterMesh(*arrays, min_faces=min_faces, largest=largest)
    want = MC.filter_mesh(*host, min_faces=min_faces, largest=largest)
    assert_same(got, want, (what, min_faces, largest))
    return want


def assert_same(got, want, what=""):
    for g, w in zip(got[:3], want[:3]):
        assert (g is None) == (w is None), what
        if w is not None:
            assert tuple(g.shape) == w.shape and T.nan_equal(_np(g).view(np.uint32), np.asarray(w).view(np.uint32)), what
    assert tuple(got[3].shape) == want[3].shape and np.array_equal(u32(got[3]), want[3]), what


@pytest.mark.parametrize("name", sorted(MC.HAND_MADE))
def test_gpu_components_of_hand_made_meshes(roo, name):
    """one triangle; two triangles sharing exactly one vertex; two disjoint triangles; isolated vertices between them; degenerate faces"""
    faces, n, vc, cf = MC.HAND_MADE[name]
    check_components(faces, n, (vc, cf))
    # the filter on them: rows of a table that tells every vertex and word apart, a NaN payload among them
    import torch
    verts = np.arange(3 * n, dtype=np.float32).reshape(n, 3)
    verts.view(np.uint32)[0, 1] = 0x7fc12345
    norms, cols = -verts, np.arange(4 * n, dtype=np.float32).reshape(n, 4) + 0.5
    host = (verts, norms, cols, np.asarray(faces, np.uint32))
    arrays = tuple(torch.from_numpy(a).cuda() for a in host[:3]) + (dev_faces(faces),)
    for min_faces, largest in ((0, False), (1, False), (2, False), (0, True), (3, True)):
        check_filter(arrays, host, min_faces, largest, name)


@pytest.mark.parametrize("name", ["permuted_strip", "descending_strip", "fan"])
def test_gpu_components_of_strips_and_the_fan(roo, name):
    """a strip of 5 000 triangles whose ids are a fixed random permutation: long paths across many workgroups; the same strip with ids
    descending along it: the deepest trees min-hooking can build; a fan of 4 096 faces around one hub: every union and every count on
    one word"""
    faces, n = {"permuted_strip": MC.permuted_strip, "descending_strip": MC.descending_strip, "fan": MC.fan}[name]()
    vc, cf = check_components(faces, n)
    assert not vc.any() and cf.tolist() == [len(faces)]
    # beside a second component and isolated vertices: ids 3 v of the strip / fan, 3 v + 1 of a small strip, 3 v + 2 unused
    small, ns = MC.descending_strip(700)
    both = np.concatenate([3 * small.astype(np.int64) + 1, 3 * faces.astype(np.int64)])
    vc, cf = check_components(both, 3 * n)
    assert cf[:2].tolist() == [len(faces), 700] and not cf[2:].any() and len(cf) == 2 + n + (n - ns)


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


def test_gpu_three_spheres_components_and_filter(roo, three_spheres):
    """V = 2480, T = 4948, 3 closed components of 132, 2260 and 2556 faces; min_faces = 1000 leaves T' = 4816, V' = 2412, two closed
    parts; largest leaves 2556 faces; min_faces = 0 returns the input bit for bit"""
    from kangaroo_amd import mesh
    ovol, vol, got, host = three_spheres
    V, Tn = len(host[0]), len(host[3])
    assert (V, Tn) == (2480, 4948)
    vc, cf = mesh.MeshComponents(got[3], V)
    wvc, wcf = MC.components(host[3], V)
    assert np.array_equal(u32(vc), wvc) and np.array_equal(u32(cf), wcf) and sorted(wcf.tolist()) == [132, 2260, 2556]
    want = check_filter(got, host, min_faces=1000)
    assert (len(want[0]), len(want[3])) == (2412, 4816)
    parts = MC.split_parts(want[3], 2412)
    assert len(parts) == 2 and all(W.closed_with_euler_2(f, nv) for f, nv in parts)
    want = check_filter(got, host, largest=True)
    assert len(want[3]) == 2556 and W.closed_with_euler_2(want[3], len(want[0]))
    check_filter(got, host, min_faces=133, largest=True)
    check_filter(got, host, min_faces=2557, largest=True)
    same = mesh.FilterMesh(*got)
    assert_same(same, host, "identity")
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(same, got) if a is not None)
    # the keywords of ExtractMesh and SaveMesh
    assert_same(mesh.ExtractMesh(vol, indexed=True, min_faces=1000), MC.filter_mesh(*host, min_faces=1000), "ExtractMesh(min_faces)")
    assert_same(mesh.ExtractMesh(vol, indexed=True, largest=True), MC.filter_mesh(*host, largest=True), "ExtractMesh(largest)")
    for kw in (dict(min_faces=5), dict(largest=True), dict(indexed=True, min_faces=5, slab=(48, 0, -1.0, 1.0, 0, 48))):
        with pytest.raises(ValueError):
            mesh.ExtractMesh(vol, **kw)


def test_gpu_save_mesh_with_a_filter(roo, three_spheres, tmp_path):
    from kangaroo_amd import mesh
    ovol, vol, got, host = three_spheres
    assert mesh.SaveMesh(str(tmp_path / "m"), vol, indexed=True, min_faces=1000) == 4816
    size, head, nv, nf, table, rows = TI.read_ply(str(tmp_path / "m.ply"))
    want = MC.filter_mesh(*host, min_faces=1000)
    assert (nv, nf) == (2412, 4816) and T.nan_equal(table[:, :3], want[0]) and T.nan_equal(table[:, 3:], want[1])
    assert np.array_equal(rows["i"], want[3])
    with pytest.raises(ValueError):
        mesh.SaveMesh(str(tmp_path / "n"), vol, min_faces=1000)


def test_gpu_ragged_unobserved_volume(roo):
    """21 x 13 x 34 with the NaN lattice and a padded pitch: V = 828, T = 983, 13 components of 1 to 227 faces; the filter at 2, 13
    and 228, the last of which leaves nothing: empty tensors, no launch error"""
    import torch
    from kangaroo_amd import mesh
    ovol, _, pitch = TI.f32_case("ragged_unobserved")
    vol = TI.upload(roo, ovol, pitch=pitch)
    wv, wn, _, wf = TI.expected(ovol)
    host = (wv, wn, None, wf)
    got = mesh.ExtractMesh(vol, indexed=True)
    assert_same(got, host, "ragged")
    assert (len(wv), len(wf)) == (828, 983)
    vc, cf = mesh.MeshComponents(got[3], len(wv))
    wvc, wcf = MC.components(wf, len(wv))
    assert np.array_equal(u32(vc), wvc) and np.array_equal(u32(cf), wcf)
    assert len(wcf) == 13 and int(wcf.min()) == 1 and int(wcf.max()) == 227
    for m in (2, 13):
        want = check_filter(got, host, min_faces=m)
        assert 0 < len(want[3]) < 983
    v, n, c, f = mesh.FilterMesh(*got, min_faces=228)
    torch.cuda.synchronize()
    assert tuple(v.shape) == (0, 3) and tuple(n.shape) == (0, 3) and c is None and tuple(f.shape) == (0, 3)
    v, n, c, f = mesh.ExtractMesh(vol, indexed=True, min_faces=228)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)


def test_gpu_fused_colour_room_rows_are_the_oracles_selection(roo):
    """the fused colour room at 64^3: filtered vertices, normals and colours are the oracle's selection of the input rows, bit for bit"""
    from kangaroo_amd import mesh
    ovol, ocvol, _ = TI.f32_case("fused_room_colour")
    vol, cvol = TI.upload(roo, ovol), TI.upload(roo, ocvol, kind="c32")
    host = TI.expected(ovol, ocvol)
    got = mesh.ExtractMesh(vol, cvol, indexed=True)
    TI.check(got, host, "colour room")
    assert host[2] is not None
    wvc, wcf = MC.components(host[3], len(host[0]))
    assert len(wcf) > 1, "the room's mesh is one component: the case filters nothing"
    second = int(np.sort(wcf)[-2])
    for min_faces, largest in ((second + 1, False), (max(second, 1), False), (0, True)):
        want = check_filter(got, host, min_faces, largest, "colour room")
        assert 0 < len(want[3]) <= len(host[3]) and want[2].shape == (len(want[0]), 4)
    assert_same(mesh.ExtractMesh(vol, cvol, indexed=True, min_faces=second + 1), MC.filter_mesh(*host, min_faces=second + 1))
    # a colour array on 4-byte alignment only takes the word path: the same rows
    import torch
    pad = torch.empty(4 * len(host[0]) + 1, dtype=torch.float32, device="cuda")
    odd = pad[1:].view(-1, 4)
    odd.copy_(got[2])
    assert odd.data_ptr() % 16 == 4
    check_filter((got[0], got[1], odd, got[3]), host, second + 1, False, "unaligned colours")
    check_filter((got[0], None, None, got[3]), (host[0], None, None, host[3]), second + 1, False, "positions alone")


def test_gpu_world_mesh_of_bricks_with_one_gone(roo):
    """the three-sphere volume packed into bricks, without the brick that holds the +x cap of the first sphere: labels and filtered arrays
    equal the oracle applied to the unfiltered ExtractBrickMesh(indexed=True) arrays"""
    import torch
    import test_gpu_brick_mesh as TB
    from kangaroo_amd import mesh
    ovol = MC.three_spheres(oracle)
    vol = TI.upload(roo, ovol)
    ids, cells = roo.BrickPack(vol, float("nan"))
    idn = TB.u32(ids).astype(np.int64)
    gone = (2 * 6 + 2) * 6 + 2   # brick (2, 2, 2) of 6 x 6 x 6: cells 16 .. 23, around the sphere's surface at x = 21
    assert gone in idn
    sel = torch.from_numpy(np.nonzero(idn != gone)[0]).cuda()
    args = ((48, 48, 48), vol.boxmin, vol.boxmax, "f32", ids[sel], cells[sel])
    full = mesh.ExtractBrickMesh(*args, indexed=True)
    host = (_np(full[0]), _np(full[1]), None, u32(full[3]))
    V, Tn = len(host[0]), len(host[3])
    assert 4000 < Tn < 4948 and not W.closed_with_euler_2(host[3], V)
    vc, cf = mesh.MeshComponents(full[3], V)
    wvc, wcf = MC.components(host[3], V)
    assert np.array_equal(u32(vc), wvc) and np.array_equal(u32(cf), wcf) and sorted(wcf.tolist())[::2] == [132, 2260]
    assert 2000 < sorted(wcf.tolist())[1] < 2556   # (the cut sphere: open, fewer faces, still one part)
    for kw in (dict(min_faces=133), dict(min_faces=1000), dict(largest=True), dict(min_faces=100000)):
        assert_same(mesh.ExtractBrickMesh(*args, indexed=True, **kw), MC.filter_mesh(*host, **kw), kw)
    with pytest.raises(ValueError):
        mesh.ExtractBrickMesh(*args, min_faces=5)


def _plan(L, faces, V):
    import torch
    Tn = len(faces)
    nbytes = L.kfx_mesh_components_scratch_bytes(V, Tn)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    counts = (C.c_ulonglong * 2)()
    code = L.kfx_mesh_components_plan(C.c_void_p(faces.data_ptr()), Tn, V, C.c_void_p(scratch.data_ptr()), nbytes, counts, None)
    return code, scratch, nbytes, counts


def test_gpu_a_face_id_of_v_is_refused_and_nothing_is_written(roo, three_spheres):
    """a face list that contains the id V: the plan's first kernel reads `faces` alone and raises the error word, every later kernel
    tests it first, the plan returns KFX_E_RANGE, and every later call on that scratch is refused with the outputs untouched"""
    import torch
    from kangaroo_amd import _lib
    L = _lib.load()
    ovol, vol, got, host = three_spheres
    V, Tn = len(host[0]), len(host[3])
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for at in (0, 3 * 2000 + 1, 3 * Tn - 1):
        faces = got[3].clone()
        faces.view(-1)[at] = V
        code, scratch, nbytes, counts = _plan(L, faces, V)
        assert code == -4 and (counts[0], counts[1]) == (0, 0), at
        assert b"face id" in L.kfx_last_error_string()
        words = scratch[:256].cpu().numpy().view(np.uint64)
        assert words[3] == 0 and words[4] == 1   # no stage reached; the error word
        at_cnt = 256 + (4 * V + 255) // 256 * 256
        assert not scratch[at_cnt:at_cnt + 4 * V].any()   # (no face was counted: cnt[] is as the init left it)
        vc = torch.full((V,), -7, dtype=torch.int32, device="cuda")
        cf = torch.full((V,), -7, dtype=torch.int32, device="cuda")
        assert L.kfx_mesh_components_emit(ptr(scratch), nbytes, V, Tn, (C.c_ulonglong * 2)(3, 2556), ptr(vc), ptr(cf), None) == -4
        kept = (C.c_ulonglong * 2)(5, 5)
        assert L.kfx_mesh_filter_plan(ptr(scratch), nbytes, V, Tn, ptr(faces), 10, 0, kept, None) == -4 and (kept[0], kept[1]) == (0, 0)
        out = torch.full((V, 3), -7.0, dtype=torch.float32, device="cuda")
        fout = torch.full((Tn, 3), -7, dtype=torch.int32, device="cuda")
        assert L.kfx_mesh_filter_emit(ptr(scratch), nbytes, V, Tn, (C.c_ulonglong * 2)(V, Tn), ptr(got[0]), None, None, ptr(faces),
                                      ptr(out), None, None, ptr(fout), None) == -4
        torch.cuda.synchronize()
        assert bool((vc == -7).all()) and bool((cf == -7).all()) and bool((out == -7.0).all()) and bool((fout == -7).all())
    # a scratch no plan has filled, and one planned for another mesh, are refused too
    zero = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    assert L.kfx_mesh_filter_plan(ptr(zero), nbytes, V, Tn, ptr(got[3]), 10, 0, kept, None) == -4
    code, scratch, nbytes, counts = _plan(L, got[3], V)
    assert code == 0 and (counts[0], counts[1]) == (3, 2556)
    big = torch.zeros(nbytes + 4096, dtype=torch.uint8, device="cuda")
    big[:nbytes] = scratch
    assert L.kfx_mesh_filter_plan(ptr(big), nbytes + 4096, V + 1, Tn, ptr(got[3]), 10, 0, kept, None) == -4
    # the filter emit before any filter plan, and with counts that are not the plan's
    assert L.kfx_mesh_filter_emit(ptr(scratch), nbytes, V, Tn, (C.c_ulonglong * 2)(2412, 4816), ptr(got[0]), None, None, ptr(got[3]),
                                  ptr(out), None, None, ptr(fout), None) == -4
    _lib.check(L.kfx_mesh_filter_plan(ptr(scratch), nbytes, V, Tn, ptr(got[3]), 1000, 0, kept, None))
    assert (kept[0], kept[1]) == (2412, 4816)
    assert L.kfx_mesh_filter_emit(ptr(scratch), nbytes, V, Tn, (C.c_ulonglong * 2)(2412, 4815), ptr(got[0]), None, None, ptr(got[3]),
                                  ptr(out), None, None, ptr(fout), None) == -4
    assert L.kfx_mesh_components_emit(ptr(scratch), nbytes, V, Tn, (C.c_ulonglong * 2)(4, 2556), ptr(vc), ptr(cf), None) == -4
    torch.cuda.synchronize()
    assert bool((vc == -7).all()) and bool((out == -7.0).all()) and bool((fout == -7).all())


def test_gpu_replanning_the_filter_on_one_scratch_equals_a_fresh_run(roo, three_spheres):
    """one labelling, the filter planned at 1000, emitted, planned again at 133 and with largest, each equal to the oracle (so to a fresh
    run); the labels emitted after the filter plans are still the oracle's; two runs give identical bytes, scratch and all"""
    import torch
    from kangaroo_amd import _lib
    L = _lib.load()
    ovol, vol, got, host = three_spheres
    V, Tn = len(host[0]), len(host[3])
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def run():
        code, scratch, nbytes, counts = _plan(L, got[3], V)
        assert code == 0
        outs = []
        for min_faces, largest in ((1000, 0), (133, 0), (0, 1), (0, 0)):
            kept = (C.c_ulonglong * 2)()
            _lib.check(L.kfx_mesh_filter_plan(ptr(scratch), nbytes, V, Tn, ptr(got[3]), min_faces, largest, kept, None))
            kv, kt = int(kept[0]), int(kept[1])
            v, n = (torch.full((kv + 1, 3), -7.0, dtype=torch.float32, device="cuda") for _ in range(2))
            f = torch.full((kt + 1, 3), -7, dtype=torch.int32, device="cuda")
            _lib.check(L.kfx_mesh_filter_emit(ptr(scratch), nbytes, V, Tn, kept, ptr(got[0]), ptr(got[1]), None, ptr(got[3]), ptr(v), ptr(n), None,
                                              ptr(f), None))
            torch.cuda.synchronize()
            assert bool((v[kv] == -7.0).all()) and bool((n[kv] == -7.0).all()) and bool((f[kt] == -7).all())   # nothing beyond V' and T'
            assert_same((v[:kv], n[:kv], None, f[:kt]), MC.filter_mesh(*host, min_faces=min_faces, largest=bool(largest)), (min_faces, largest))
            outs += [v, n, f]
        vc = torch.empty(V, dtype=torch.int32, device="cuda")
        cf = torch.empty(int(counts[0]), dtype=torch.int32, device="cuda")
        _lib.check(L.kfx_mesh_components_emit(ptr(scratch), nbytes, V, Tn, counts, ptr(vc), ptr(cf), None))
        wvc, wcf = MC.components(host[3], V)
        assert np.array_equal(u32(vc), wvc) and np.array_equal(u32(cf), wcf)
        torch.cuda.synchronize()
        return outs + [vc, cf, scratch]

    first, second = run(), run()
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(first, second))
