"""Colour mode on Z-slabs (include/kfx_slab_color.h): the colour SdfFuse on a slab, the colour in the exact march (rounds and packed
row-tiles), the slab rank's frame object and the slab meshes -- every plane, pixel and vertex colour bit-identical to the single-volume
colour operators in both numerics modes, and to the CPU oracle in exact numerics.  The ranks are emulated in one process.

Inputs: test_color_cpu.color_setup -- the 64^3 room, 160 x 120 depth and RGB, 3 frames (the colour camera a few centimetres beside
the depth camera).  The whole-volume results are computed once per numerics mode and shared."""
import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import oracle, scenes

pytestmark = pytest.mark.gpu

N, W, H, FRAMES = 64, 160, 120, 3
_cache = {}


def upload_rgb(roo, arr):
    im = roo.Image(arr.shape[1], arr.shape[0], "u8x3")
    im.MemcpyFromHost(arr)
    return im


def images(roo, w=W, h=H):
    return roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h)


def host(imgs):
    return [x.MemcpyToHost() for x in imgs]


def whole(roo, math, dims=(N, N, N)):
    """SdfFuseColor on the whole volume, frame by frame (host copies of both volumes after every frame), the colour and the grey
    rendering of the last pose; in exact numerics all of it checked against the oracle.  Computed once, never modified."""
    key = (math, dims)
    if key in _cache:
        return _cache[key]
    import test_color_cpu as TC
    ovol, ocvol, K, Kimg, tr, near, far, inputs = TC.color_setup(0, W, H, W, H, dims=dims, frames=FRAMES)
    bmin, bmax = scenes.SCENES["room"][:2]
    prev = roo.set_math_mode(math)
    try:
        vol, cvol = roo.BoundedVolume(*dims, bmin, bmax), roo.BoundedVolume(*dims, bmin, bmax, kind="c32")
        roo.SdfReset(vol, float("nan"))
        roo.ColorReset(cvol)
        frames = []
        for fr in inputs:
            g = dict(f=T.upload_image(roo, fr["f"].data), nrm=T.upload_image(roo, fr["nrm"].data), rgb=upload_rgb(roo, fr["rgb"].data),
                     T_cw=fr["T_cw"], T_iw=fr["T_iw"], T_wc=fr["T_wc"])
            roo.SdfFuseColor(vol, cvol, g["f"], g["nrm"], g["T_cw"], K, g["rgb"], g["T_iw"], Kimg, tr, scenes.MAX_W, scenes.MIN_COS_THETA)
            g["vol"], g["cvol"] = vol.MemcpyToHost(), cvol.MemcpyToHost()
            if math == "exact":
                oracle.sdf_fuse_color(ovol, ocvol, fr["f"], fr["nrm"], fr["T_cw"], K, fr["rgb"], fr["T_iw"], Kimg, tr, scenes.MAX_W, scenes.MIN_COS_THETA, nthreads=0)
                assert T.nan_equal(g["vol"], ovol.data), T.mismatch_report(g["vol"], ovol.data)
                assert T.nan_equal(g["cvol"], ocvol.data), T.mismatch_report(g["cvol"], ocvol.data)
            frames.append(g)
        T_wc = inputs[-1]["T_wc"]
        col, grey = images(roo), images(roo)
        roo.RaycastSdfColor(*col, vol, cvol, T_wc, K, near, far, tr, True)
        roo.RaycastSdf(*grey, vol, T_wc, K, near, far, tr, True)
        want, shade = host(col), host(grey)[2]
        if math == "exact" and dims == (N, N, N):
            od, on, oi = oracle.Image(W, H), oracle.Image(W, H, channels=4), oracle.Image(W, H)
            oracle.raycast_sdf_color(od, on, oi, ovol, ocvol, T_wc, K, near, far, tr, True, nthreads=0)
            for a, b in zip(want, (od.data, on.data, oi.data)):
                assert T.nan_equal(a, b), T.mismatch_report(a, b)
    finally:
        roo.set_math_mode(prev)
    hit = np.isfinite(want[0])
    m = dict(K=K, Kimg=Kimg, tr=tr, near=near, far=far, bmin=bmin, bmax=bmax, dims=dims, frames=frames, vol=vol, cvol=cvol, T_wc=T_wc,
             want=want, shade=shade, hit=hit)
    _cache[key] = m
    return m


def check_rendering_is_colour(m):
    """the conditions that keep an image test from passing on nothing -- or on a Phong image"""
    hit, img = m["hit"], m["want"][2]
    assert hit.mean() > 0.3, hit.mean()
    assert np.ptp(img[hit]) > 0.2, np.ptp(img[hit])
    assert (img[hit] != m["shade"][hit]).mean() > 0.5, (img[hit] != m["shade"][hit]).mean()


def stored_ranges(d, world, ghost):
    from kangaroo_amd.pipeline import slab_range
    spans = [slab_range(d, r, world) for r in range(world)]
    return spans, [(max(z0 - ghost, 0), min(z1 + ghost, d)) for z0, z1 in spans]


def local_slabs(roo, m, s0, s1, colour_pitch=None):
    """a rank's own storage for planes [s0, s1): SDF and colour volumes with the local box (BoundedVolume::SubBoundingVolume's)"""
    W_, H_, D_ = m["dims"]
    box = m["vol"].ZSlab(s0, s1)
    v = roo.BoundedVolume(W_, H_, s1 - s0, box.boxmin, box.boxmax)
    c = roo.BoundedVolume(W_, H_, s1 - s0, box.boxmin, box.boxmax, kind="c32", pitch=colour_pitch)
    return v, c


def fuse_in_slabs(roo, m, world, ghost, colour_pitch=None):
    """every rank integrates its stored planes frame by frame; after each frame they equal the whole volume's planes"""
    D_ = m["dims"][2]
    spans, stored = stored_ranges(D_, world, ghost)
    zmin, zmax = float(m["bmin"][2]), float(m["bmax"][2])
    ranks = [local_slabs(roo, m, s0, s1, colour_pitch) for s0, s1 in stored]
    for v, c in ranks:
        roo.SdfReset(v, float("nan"))
        roo.ColorReset(c)
    for k, g in enumerate(m["frames"]):
        for r, ((v, c), (s0, s1)) in enumerate(zip(ranks, stored)):
            if k % 2 == 0:   # the stored planes at once (ghost planes recomputed) ...
                roo.SdfFuseColorSlab(v, c, (D_, s0, zmin, zmax), g["f"], g["nrm"], g["T_cw"], m["K"], g["rgb"], g["T_iw"], m["Kimg"], m["tr"],
                                     scenes.MAX_W, scenes.MIN_COS_THETA, full_extent="slab")
            else:            # ... or in two launches on views that start anywhere: the owned planes, then the ghost planes around them
                z0, z1 = spans[r]
                for a, b in ((z0, z1), (s0, z0), (z1, s1)):
                    if b > a:
                        roo.SdfFuseColorSlab(v.ZSlab(a - s0, b - s0), c.ZSlab(a - s0, b - s0), (D_, a, zmin, zmax), g["f"], g["nrm"], g["T_cw"], m["K"],
                                             g["rgb"], g["T_iw"], m["Kimg"], m["tr"], scenes.MAX_W, scenes.MIN_COS_THETA, full_extent="slab")
            gv, gc = v.MemcpyToHost(), c.MemcpyToHost()
            assert T.nan_equal(gv, g["vol"][s0:s1]), (k, r, T.mismatch_report(gv, g["vol"][s0:s1]))
            assert T.nan_equal(gc, g["cvol"][s0:s1]), (k, r, T.mismatch_report(gc, g["cvol"][s0:s1]))
    return ranks, spans, stored


@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("world,ghost", [(2, 2), (3, 2), (3, 7)])
def test_gpu_colour_fuse_on_slabs(roo, world, ghost, math):
    """World 3 owns 22 / 21 / 21 planes: slabs (and the views inside them) start on multiples of neither 8 nor 16."""
    m = whole(roo, math)
    changed = (m["frames"][-1]["cvol"] != 0.5).mean()
    assert changed > 0.2, changed
    prev = roo.set_math_mode(math)
    try:
        fuse_in_slabs(roo, m, world, ghost)
    finally:
        roo.set_math_mode(prev)


@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("colour_pitch", [None, 164])
def test_gpu_colour_fuse_on_ragged_slabs(roo, colour_pitch, math):
    """40 x 36 x 44 in 2 slabs: the reference's extents on the whole volume (x, y to multiples of 16: 32 x 32, every plane).  A colour
    row pitch of 164 bytes breaks the tiled kernel's 8-byte alignment on the local view: that slab takes the untiled kernel."""
    m = whole(roo, math, dims=(40, 36, 44))
    last = m["frames"][-1]["cvol"]
    assert (last[:, :32, :32] != 0.5).mean() > 0.2 and (last[:, 32:] == 0.5).all() and (last[:, :, 32:] == 0.5).all()
    prev = roo.set_math_mode(math)
    try:
        fuse_in_slabs(roo, m, 2, 2, colour_pitch)
    finally:
        roo.set_math_mode(prev)


def slab_views(m, stored):
    return [(m["vol"].ZSlab(s0, s1), m["cvol"].ZSlab(s0, s1)) for s0, s1 in stored]


@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_gpu_colour_march_in_rounds(roo, world, math):
    """The rounds of test_gpu_exact_slab_raycast_rounds with the colour kernel: per-slab states, integer-sum merge of the touched
    pixels' march planes, the result planes summed at the end.  Depth, normals and colour equal RaycastSdfColor on the whole volume."""
    import torch
    m = whole(roo, math)
    check_rendering_is_colour(m)
    spans, stored = stored_ranges(N, world, 2)
    views = slab_views(m, stored)
    zmin, zmax = float(m["bmin"][2]), float(m["bmax"][2])
    states = [torch.empty((9, H, W), dtype=torch.float32, device="cuda") for _ in range(world)]
    prev = roo.set_math_mode(math)
    try:
        rounds = 0
        while True:
            for r in range(world):
                roo.RaycastSdfSlabColor(states[r], rounds == 0, views[r][0], views[r][1], (N, stored[r][0], zmin, zmax), spans[r][0], spans[r][1], W, H,
                                        m["T_wc"], m["K"], m["near"], m["far"], m["tr"], True)
            rounds += 1
            march = [s[0:5].view(torch.int32) for s in states]
            total = torch.zeros_like(march[0])
            for x in march:
                total += torch.where((x[4] != 0).unsqueeze(0), x, torch.zeros_like(x))
            assert bool(((total[4] == 0) | (total[4] == 0x3F800000)).all())   # one toucher per pixel and round
            for x in march:
                x.copy_(torch.where((total[4] != 0).unsqueeze(0), total, x))
            status = states[0][3]
            if not bool(((status == 0) | (status == 3)).any()):
                break
            assert rounds <= world + 3
        assert rounds > 1
        out = torch.zeros((4, H, W), dtype=torch.int32, device="cuda")
        for s in states:
            out += s[5:9].view(torch.int32)
        states[0][5:9].view(torch.int32).copy_(out)
        got = images(roo)
        roo.RaycastStateToImages(*got, states[0])
    finally:
        roo.set_math_mode(prev)
    for a, b in zip(host(got), m["want"]):
        assert T.nan_equal(a, b), T.mismatch_report(a, b)


@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("tiles", [1, 4, 7])
def test_gpu_colour_march_in_packed_tiles(roo, tiles, math):
    """kfx_raycast_sdf_slab_tiles_color on the hand-over's own state: three packed march planes per row-tile (layout_flags 2), hits
    finalised wherever their stencil is stored (4), ghost 7, world 3; 7 tiles of 18 rows leave a last tile of 12.  Each round every
    rank visits every tile and adopts what its neighbours held after the previous round (their newer, still open snapshots: tile-major
    buffers, 1); a pixel is finalised by exactly one rank, whose lambda, status, normal and colour make the images."""
    import ctypes as C
    import torch
    from kangaroo_amd import _lib
    from kangaroo_amd.roo import _fp
    L = _lib.load()
    m = whole(roo, math)
    world, ghost = 3, 7
    spans, stored = stored_ranges(N, world, ghost)
    views = slab_views(m, stored)
    zmin, zmax = float(m["bmin"][2]), float(m["bmax"][2])
    R = (H + tiles - 1) // tiles
    nt = (H + R - 1) // R
    P = (R * W + 63) // 64 * 64
    M = [torch.zeros((nt, 3, P), dtype=torch.float32, device="cuda") for _ in range(world)]
    Rz = [torch.zeros((nt, 4, P), dtype=torch.float32, device="cuda") for _ in range(world)]
    fin = [torch.zeros((H, W), dtype=torch.int32, device="cuda") for _ in range(world)]
    t, _t = _fp(m["T_wc"], 12)
    k, _k = _fp(m["K"], 4)
    ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None   # noqa: E731
    prev = roo.set_math_mode(math)
    try:
        for rnd in range(world + 3):
            snap = [x.clone() for x in M]
            for r in range(world):
                sl = _lib.KfxSlab(N, stored[r][0], zmin, zmax)
                for tl in range(nt):
                    v0, v1 = tl * R, min(tl * R + R, H)
                    _lib.check(L.kfx_raycast_sdf_slab_tiles_color(ptr(M[r]), ptr(Rz[r]), P, R, v0, v1, 1 if rnd == 0 else 0, ptr(fin[r]), 1 if r == 0 else 0,
                                                                  ptr(snap[r - 1]) if (rnd and r > 0) else None,
                                                                  ptr(snap[r + 1]) if (rnd and r + 1 < world) else None, 1 | 2 | 4,
                                                                  views[r][0].ref(), views[r][1].ref(), C.byref(sl), spans[r][0], spans[r][1], W, H, t, k,
                                                                  m["near"], m["far"], m["tr"], 1, None))
            done = sum(fin)
            assert int(done.max()) <= 1
            if int(done.min()) == 1:
                break
        assert int(done.min()) == 1, "%d rays without a final status" % int((done == 0).sum())
        assert rnd >= 1
    finally:
        roo.set_math_mode(prev)

    def plane(x, c):   # plane c of the tiles as an (H, W) image
        rows = [x[tl, c, :R * W].reshape(R, W)[:min(R, H - tl * R)] for tl in range(nt)]
        return torch.cat(rows)
    pick = lambda arrs: sum(torch.where(fin[r] != 0, arrs[r].view(torch.int32), torch.zeros_like(fin[r])) for r in range(world)).view(torch.float32)   # noqa: E731
    lam, code = pick([plane(M[r], 0) for r in range(world)]), pick([plane(M[r], 2) for r in range(world)])
    res = [pick([plane(Rz[r], c) for r in range(world)]) for c in range(4)]
    hit = (code == -1.0) & (lam > 0)
    assert bool(((code == -1.0) | (code == -2.0)).all())
    zero = torch.zeros_like(lam)
    depth = torch.where(hit, lam, torch.full_like(lam, float("nan"))).cpu().numpy()
    norm = torch.stack([torch.where(hit, res[c], zero) for c in range(3)] + [hit.to(torch.float32)], dim=-1).cpu().numpy()
    img = torch.where(hit, res[3], zero).cpu().numpy()
    for a, b in zip((depth, norm, img), m["want"]):
        assert T.nan_equal(a, b), T.mismatch_report(a, b)


class OneRank:
    """torch.distributed's rank / world queries for a pipeline of one rank (its collectives are never entered)"""
    @staticmethod
    def get_rank():
        return 0

    @staticmethod
    def get_world_size():
        return 1


@pytest.mark.parametrize("raycast", ["exact", "composite"])
def test_gpu_colour_slab_frame_one_rank(roo, raycast):
    """SlabPipeline(driver="c", color=True) of one rank -- kfx_slab_frame_step after kfx_slab_frame_set_color -- against
    FramePipeline(color=True, track=False) over 4 frames: SDF volume, colour volume and the three images are equal; set_color(None)
    returns the frame to grey."""
    import torch
    from kangaroo_amd import slab as S
    from kangaroo_amd.pipeline import FramePipeline, SlabPipeline
    bmin, bmax, near, far = scenes.SCENES["room"]
    comm = S.Comm.threads(1)[0]
    try:
        sp = SlabPipeline(roo, OneRank, (N, N, N), bmin, bmax, W, H, near=near, far=far, driver="c", comm=comm, color=True, raycast=raycast)
        mono = FramePipeline(roo, (N, N, N), bmin, bmax, W, H, near=near, far=far, color=True, track=False)
        for i in range(4):
            T_wc = scenes.orbit_pose(i, 8)
            raw = scenes.render_depth("room", W, H, T_wc, sp.K)
            rgb = scenes.render_rgb("room", W, H, T_wc, sp.Kimg)
            for p in (sp, mono):
                p.raw.MemcpyFromHost(raw)
                p.rgb.MemcpyFromHost(rgb)
                p.step(T_wc)
            sp.wait_composite()
            sp.sframe.sync()
            torch.cuda.synchronize()
            for a, b in zip(host((sp.ray_d, sp.ray_n, sp.ray_i)), host((mono.ray_d, mono.ray_n, mono.ray_i))):
                assert T.nan_equal(a, b), (i, T.mismatch_report(a, b))
        assert T.nan_equal(sp.vol.MemcpyToHost(), mono.vol.MemcpyToHost())
        assert T.nan_equal(sp.cvol.MemcpyToHost(), mono.cvol.MemcpyToHost())
        col = sp.ray_i.MemcpyToHost()
        hit = np.isfinite(sp.ray_d.MemcpyToHost())
        assert hit.mean() > 0.3 and np.ptp(col[hit]) > 0.2 and (sp.cvol.MemcpyToHost() != 0.5).mean() > 0.2
        sp.sframe.set_color(None)                        # grey again: the Phong shade of the same model
        sp.sframe.step(T_wc, None, None, 4)
        sp.sframe.sync()
        grey = images(roo)
        roo.RaycastSdf(*grey, mono.vol, T_wc, sp.K, near, far, sp.trunc, True)
        assert T.nan_equal(sp.ray_i.MemcpyToHost(), grey[2].MemcpyToHost()) and (col[hit] != grey[2].MemcpyToHost()[hit]).mean() > 0.5
        sp.sframe.set_color(sp.cvol, sp.rgb, sp.Kimg, sp.T_cd)
        sp.sframe.reset()                                # kfx_slab_frame_reset: both slabs
        torch.cuda.synchronize()
        assert np.isnan(sp.vol.MemcpyToHost()[..., 0]).all() and (sp.cvol.MemcpyToHost() == 0.5).all()
        del sp
    finally:
        comm.destroy()


def test_gpu_colour_slab_meshes(roo):
    """The fused colour room in 3 slabs, ghost 2: the ranks' meshes, ordered by global cube index, are the single-volume colour mesh in
    vertices, normals and colours; a ghost of 1 is still refused."""
    import torch
    from kangaroo_amd import _lib, mesh
    m = whole(roo, "exact")
    verts, norms, colors, index, offs = mesh.ExtractMesh(m["vol"], m["cvol"], with_index=True)
    assert len(verts) // 3 > 1000 and colors is not None and np.ptp(colors[:, 0].cpu().numpy()) > 0.2
    zmin, zmax = float(m["bmin"][2]), float(m["bmax"][2])
    spans, stored = stored_ranges(N, 3, 2)
    parts = []
    for (z0, z1), (s0, s1) in zip(spans, stored):
        v, c = local_slabs(roo, m, s0, s1)
        v.planes(0, v.d).copy_(m["vol"].planes(s0, s1))
        c.planes(0, c.d).copy_(m["cvol"].planes(s0, s1))
        parts.append(mesh.ExtractMesh(v, c, slab=(N, s0, zmin, zmax, z0, z1), with_index=True))
        assert parts[-1][2] is not None
    def per_triangle(part):
        """(cube index of every triangle, the part's arrays as one row per triangle) in the part's own order"""
        idx, off = part[3].cpu().numpy(), part[4].cpu().numpy().view(np.uint32).astype(np.int64)
        ntri = len(part[0]) // 3
        assert (np.diff(idx) > 0).all() and (len(off) == 0 or off[0] == 0)
        counts = np.diff(np.concatenate([off, [ntri]]))
        assert (counts > 0).all()
        return np.repeat(idx, counts), [part[k].cpu().numpy().reshape(ntri, -1) for k in range(3)]
    want_cube, want = per_triangle((verts, norms, colors, index, offs))
    cubes, rows = zip(*[per_triangle(p) for p in parts])
    cube = np.concatenate(cubes)
    order = np.argsort(cube, kind="stable")     # a cube belongs to one rank and its triangles stay in their order
    assert np.array_equal(cube[order], want_cube)
    for name, k in (("vertices", 0), ("normals", 1), ("colours", 2)):
        got = np.concatenate([r[k] for r in rows])[order]
        assert T.nan_equal(got, want[k]), (name, T.mismatch_report(got, want[k]))
    (z0, z1), (s0, s1) = spans[1], (spans[1][0] - 1, spans[1][1] + 1)                 # ghost 1
    v, c = local_slabs(roo, m, s0, s1)
    with pytest.raises(_lib.KfxError, match="do not cover"):
        mesh.ExtractMesh(v, c, slab=(N, s0, zmin, zmax, z0, z1))
