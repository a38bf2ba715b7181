"""RaycastSdf straight from packed bricks (include/kfx_raycast_bricks.h, roo.RaycastSdfBricks) against its definition: the existing
RaycastSdf (RaycastSdfColor) on the dense volume D that is NaN everywhere and then gets the same bricks unpacked (C: 0.5, then the
colour bricks).  All three images as int32 bits, the no-hit pixels included; the images are pitched, with 0xA5 guard bytes in the
padding and behind the last row, which must stay.  The scenes are brick_raycast_cases.py's; test_brick_raycast_cases_cpu.py shows on
the oracle that they hit, miss and change under the drop rule, and the same floors are asserted here on the GPU comparator."""
import os
import subprocess
import sys

import numpy as np
import pytest

import brick_raycast_cases as BC
import kfx_testlib as T
from kfx_testlib import scenes

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 0xA5


def u32(ids):
    return ids.cpu().numpy().view(np.uint32)


class Guarded:
    """depth / normals / shade of w x h pixels in pitched storage filled with 0xA5: at least 256 bytes of padding per row and behind
    the last row"""

    def __init__(self, roo, w, h):
        import torch
        self.w, self.h, self.images, self.stores = w, h, [], []
        for kind, elem in (("f32", 4), ("f32x4", 16), ("f32", 4)):
            pitch = (w * elem + 255) // 256 * 256 + 256
            store = torch.full((pitch * h + 1024,), GUARD, dtype=torch.uint8, device="cuda")
            self.stores.append((store, pitch, w * elem))
            self.images.append(roo.Image(w, h, kind, pitch=pitch, _storage=store, _offset=0))

    def read(self):
        """the three images as int32 bits, after the guards have been checked"""
        import torch
        torch.cuda.synchronize()
        for store, pitch, row in self.stores:
            rows = store[:pitch * self.h].reshape(self.h, pitch)
            assert bool((rows[:, row:] == GUARD).all()), "written into the row padding"
            assert bool((store[pitch * self.h:] == GUARD).all()), "written behind the last row"
        return [im.MemcpyToHost().view(np.int32) for im in self.images]


def dense_volume(roo, dims, bmin, bmax, kind, ids, cells):
    """the definition's D (kind f32 / f16: NaN, then the bricks) or C (kind c32: 0.5, then the bricks)"""
    D = roo.BoundedVolume(*[int(d) for d in dims], bmin, bmax, kind=kind)
    if kind == "c32":
        roo.ColorReset(D)
    else:
        roo.SdfReset(D, NAN)
    if ids is not None and len(ids):
        roo.BrickUnpack(D, ids, cells)
    return D


def dense_images(roo, D, T_wc, K, size, far, subpix=True, Cv=None):
    w, h = size
    d, n, i = roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h)
    if Cv is not None:
        roo.RaycastSdfColor(d, n, i, D, Cv, T_wc, K, BC.NEAR, far, BC.TRUNC, subpix)
    else:
        roo.RaycastSdf(d, n, i, D, T_wc, K, BC.NEAR, far, BC.TRUNC, subpix)
    return [im.MemcpyToHost().view(np.int32) for im in (d, n, i)]


def assert_same_bits(got, want, what=""):
    for name, g, w in zip(("depth", "normal", "shade"), got, want):
        bad = int(np.count_nonzero(g != w))
        assert bad == 0, "%s: %d %s words differ from the dense rendering's" % (what, bad, name)


def hits_of(images):
    return int(np.count_nonzero(images[0].view(np.float32) > 0))


def assert_floors(want, what):
    pixels, hits = want[0].size, hits_of(want)
    print("%s: the comparator hits %d of %d pixels" % (what, hits, pixels))
    assert hits >= BC.HIT_FLOOR * pixels and pixels - hits >= BC.MISS_FLOOR * pixels, (what, hits, pixels)
    # a no-hit pixel is (NaN, (0, 0, 0, 0), 0) and a hit has w = 1 in its normal
    miss = ~(want[0].view(np.float32) > 0)
    assert np.all(np.isnan(want[0].view(np.float32)[miss])) and np.all(want[1][miss] == 0) and np.all(want[2][miss] == 0)
    assert np.all(want[1].view(np.float32)[~miss][:, 3] == 1.0)


def differing(a, b):
    return int(np.count_nonzero((a[0] != b[0]) | np.any(a[1] != b[1], axis=-1)))


# ---- the scenes on the device -----------------------------------------------------------------------------------------------------
_scene_cache = {}


def scene(roo, case, kind="f32"):
    """(bmin, bmax, ids, cells) of the case's volume, BrickPack(vol, NaN); case C with random bytes in the payload outside the frame"""
    import torch
    key = (case if case != "A2" and case != "B" and case != "D" else "A", kind)   # (A, A2, B, D share the volume)
    if key in _scene_cache:
        return _scene_cache[key]
    c = BC.CASES[case]
    dims = c["dims"]
    bmin, bmax = BC.box(dims)
    vol = roo.BoundedVolume(*dims, bmin, bmax, kind=kind)
    roo.SdfSphere(vol, c["center"], c["r"])
    if c.get("nan7"):
        vol.tensor()[..., 0][torch.from_numpy(BC.nan7_mask(dims)).cuda()] = NAN
    ids, cells = roo.BrickPack(vol, NAN)
    if case == "S":
        keep = BC.shell_keep(vol.MemcpyToHost()[..., 0], dims)
        assert np.array_equal(u32(ids), np.arange(c["kept"][1], dtype=np.uint32)) and len(keep) == c["kept"][0]
        sel = torch.from_numpy(keep.astype(np.int64)).cuda()
        ids, cells = ids[sel].contiguous(), cells[sel].contiguous()
    else:
        assert ids.numel() == c["dropped"][1]
    if c.get("nan7"):
        elem = vol.ELEM
        host, idn = cells.cpu().numpy().reshape(-1, 8, 8, 8, elem).copy(), u32(ids)
        bx, by, bz = BC.brick_coords(idn, dims)
        l = np.arange(8)
        outside = ((bz[:, None] * 8 + l)[:, :, None, None] >= dims[2]) | ((by[:, None] * 8 + l)[:, None, :, None] >= dims[1]) | \
            ((bx[:, None] * 8 + l)[:, None, None, :] >= dims[0])
        assert outside.any() and not outside.all()
        host[outside] = np.random.default_rng(3).integers(0, 256, (int(outside.sum()), elem), dtype=np.uint8)
        cells = torch.from_numpy(host.reshape(len(idn), -1)).cuda()
    _scene_cache[key] = (bmin, bmax, ids, cells)
    return _scene_cache[key]


def listed(case, ids, cells, dropped):
    """the case's list: all of its bricks, or those the drop rule leaves"""
    import torch
    if not dropped:
        return ids, cells
    keep = ~BC.drop5(u32(ids), BC.CASES[case]["dims"])
    assert int((~keep).sum()) == BC.CASES[case]["dropped"][0]
    sel = torch.from_numpy(np.nonzero(keep)[0]).cuda()
    return ids[sel].contiguous(), cells[sel].contiguous()


def run_case(roo, case, dropped, kind="f32", subpix=True):
    """render the case's list from bricks and from its dense D; returns (brick images, dense images, all-bricks dense images)"""
    c = BC.CASES[case]
    dims, size, far = c["dims"], c["size"], c["far"]
    bmin, bmax, ids0, cells0 = scene(roo, case, kind)
    ids, cells = listed(case, ids0, cells0, dropped)
    T_wc, K = BC.pose(case), BC.intrinsics(case)
    out = Guarded(roo, *size)
    roo.RaycastSdfBricks(*out.images, dims, bmin, bmax, kind, ids, cells, T_wc, K, BC.NEAR, far, BC.TRUNC, subpix)
    got = out.read()
    want = dense_images(roo, dense_volume(roo, dims, bmin, bmax, kind, ids, cells), T_wc, K, size, far, subpix)
    what = "case %s %s%s%s" % (case, kind, " drop5" if dropped else "", "" if subpix else " no subpix")
    assert_floors(want, what)
    full = want
    if dropped:
        full = dense_images(roo, dense_volume(roo, dims, bmin, bmax, kind, ids0, cells0), T_wc, K, size, far, subpix)
        diff = differing(want, full)
        print("%s: %d pixels differ from the all-bricks rendering" % (what, diff))
        assert diff >= BC.DIFFER_FLOOR * want[0].size
    assert_same_bits(got, want, what)
    return got, want, full


@pytest.mark.parametrize("dropped", [True, False], ids=["drop5", "all"])
@pytest.mark.parametrize("case", ["A", "A2", "B", "C", "D"], ids=lambda c: "case" + c)
def test_gpu_brick_raycast_equals_the_dense_raycast(roo, case, dropped):
    got, want, full = run_case(roo, case, dropped)
    # (the oracle's counts of the cases module are asserted on the CPU; here they are reported beside the device comparator's)
    counts = (hits_of(full), hits_of(want), differing(want, full)) if dropped else (hits_of(want),)
    print("case %s: comparator counts %s, the oracle's %s" % (case, counts, BC.CASES[case]["counts"]))


def test_gpu_brick_raycast_without_subpixel_refinement(roo):
    got, want, _ = run_case(roo, "A", True, subpix=False)
    sub = run_case(roo, "A", True)[0]
    hit = lambda images: images[0].view(np.float32) > 0
    assert np.array_equal(hit(got), hit(sub)) and differing(got, sub) > 0   # the same hits at other depths


def test_gpu_brick_raycast_of_a_shell_marches_through_absent_bricks(roo):
    got, want, _ = run_case(roo, "S", False)
    assert hits_of(want) == BC.CASES["S"]["counts"][1]


@pytest.mark.parametrize("dropped", [True, False], ids=["drop5", "all"])
@pytest.mark.parametrize("case", ["A", "C"], ids=lambda c: "case" + c)
def test_gpu_brick_raycast_half_cells(roo, case, dropped):
    run_case(roo, case, dropped, kind="f16")


@pytest.mark.parametrize("colour_list", ["all", "drop5", "none"])
def test_gpu_brick_raycast_colour(roo, colour_list):
    """case A with a ramp in the colour volume; the colour list complete, under the drop rule (another set of bricks than the SDF
    list: 0.5 there), or empty (0.5 at every hit)"""
    import torch
    case = "A"
    c = BC.CASES[case]
    dims, size, far = c["dims"], c["size"], c["far"]
    bmin, bmax, ids, cells = scene(roo, case)
    cvol = roo.BoundedVolume(*dims, bmin, bmax, kind="c32")
    z, y, x = torch.meshgrid(*[torch.arange(n, device="cuda", dtype=torch.float32) for n in dims[::-1]], indexing="ij")
    cvol.tensor()[..., 0] = 0.2 + 0.01 * x + 0.013 * y + 0.007 * z
    cids, ccells = roo.BrickPack(cvol, 0.5)
    assert cids.numel() == c["dropped"][1]
    if colour_list == "drop5":
        cids, ccells = listed(case, cids, ccells, True)
    elif colour_list == "none":
        cids, ccells = cids[:0].contiguous(), ccells[:0].contiguous()
    T_wc, K = BC.pose(case), BC.intrinsics(case)
    out = Guarded(roo, *size)
    roo.RaycastSdfBricks(*out.images, dims, bmin, bmax, "f32", ids, cells, T_wc, K, BC.NEAR, far, BC.TRUNC, True, cids=cids, ccells=ccells, color=True)
    got = out.read()
    D = dense_volume(roo, dims, bmin, bmax, "f32", ids, cells)
    Cv = dense_volume(roo, dims, bmin, bmax, "c32", cids, ccells)
    want = dense_images(roo, D, T_wc, K, size, far, True, Cv)
    assert_floors(want, "colour " + colour_list)
    assert_same_bits(got, want, "colour " + colour_list)
    shade = got[2].view(np.float32)[got[0].view(np.float32) > 0]
    if colour_list == "none":
        assert np.all(shade == 0.5)
    elif colour_list == "drop5":
        assert (shade == 0.5).any() and (shade != 0.5).any()
    else:
        assert (shade != 0.5).mean() > 0.9
    if colour_list == "all":   # color=False with a colour list given: the grey rendering
        grey = Guarded(roo, *size)
        roo.RaycastSdfBricks(*grey.images, dims, bmin, bmax, "f32", ids, cells, T_wc, K, BC.NEAR, far, BC.TRUNC, True, cids=cids, ccells=ccells)
        assert_same_bits(grey.read(), dense_images(roo, D, T_wc, K, size, far), "grey with a colour list")


def test_gpu_brick_raycast_one_plan_serves_poses_and_image_sizes_and_is_not_written(roo):
    bmin, bmax, ids0, cells0 = scene(roo, "A")
    ids, cells = listed("A", ids0, cells0, True)
    dims, far = BC.CASES["A"]["dims"], BC.CASES["A"]["far"]
    plan = roo.RaycastBricksPlan(dims, ids)
    assert plan.numel() == roo.RaycastBricksScratchBytes(ids.numel()) == 256 + 8 * 128
    before = plan.clone()
    hdr = before[:24].cpu().numpy()
    assert tuple(hdr[:8].view(np.uint32)) == (ids.numel(), 0) and tuple(hdr[8:24].view(np.uint64)) == (128, 0)   # the header's record
    D = dense_volume(roo, dims, bmin, bmax, "f32", ids, cells)
    for case, size in (("A", (96, 72)), ("B", (67, 45))):
        T_wc, K = BC.pose(case), BC.intrinsics(case, size)
        out = Guarded(roo, *size)
        roo.RaycastSdfBricks(*out.images, dims, bmin, bmax, "f32", ids, cells, T_wc, K, BC.NEAR, far, BC.TRUNC, True, plan=plan)
        got = out.read()
        want = dense_images(roo, D, T_wc, K, size, far)
        assert_floors(want, "one plan, pose %s at %d x %d" % (case, *size))
        assert_same_bits(got, want, "one plan, pose " + case)
        assert bool((plan == before).all()), "the render wrote the scratch"


def test_gpu_brick_raycast_skips_an_id_beyond_the_frame(roo):
    import torch
    bmin, bmax, ids0, cells0 = scene(roo, "A")
    ids, cells = listed("A", ids0, cells0, True)
    c = BC.CASES["A"]
    nb = c["dropped"][1]
    beyond = torch.from_numpy(np.array([nb + 3], np.uint32).view(np.int32)).cuda()
    junk = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (1, 4096), dtype=np.uint8)).cuda()
    ids2, cells2 = torch.cat([ids, beyond]).contiguous(), torch.cat([cells, junk]).contiguous()
    T_wc, K = BC.pose("A"), BC.intrinsics("A")
    out = Guarded(roo, *c["size"])
    roo.RaycastSdfBricks(*out.images, c["dims"], bmin, bmax, "f32", ids2, cells2, T_wc, K, BC.NEAR, c["far"], BC.TRUNC, True)
    got = out.read()
    want = dense_images(roo, dense_volume(roo, c["dims"], bmin, bmax, "f32", ids, cells), T_wc, K, c["size"], c["far"])
    assert_floors(want, "an id beyond the frame")
    assert_same_bits(got, want, "an id beyond the frame")


def test_gpu_brick_raycast_of_no_bricks_misses_everywhere(roo):
    c = BC.CASES["A"]
    bmin, bmax = BC.box(c["dims"])
    T_wc, K = BC.pose("A"), BC.intrinsics("A")
    out = Guarded(roo, *c["size"])
    roo.RaycastSdfBricks(*out.images, c["dims"], bmin, bmax, "f32", np.zeros(0, np.uint32), np.zeros((0, 4096), np.uint8), T_wc, K, BC.NEAR, c["far"], BC.TRUNC)
    got = out.read()
    want = dense_images(roo, dense_volume(roo, c["dims"], bmin, bmax, "f32", None, None), T_wc, K, c["size"], c["far"])
    assert hits_of(want) == 0 and np.all(np.isnan(want[0].view(np.float32)))
    assert_same_bits(got, want, "no bricks")
    with pytest.raises(ValueError, match="ascending"):
        roo.RaycastSdfBricks(*out.images, c["dims"], bmin, bmax, "f32", np.array([3, 3], np.uint32), np.zeros((2, 4096), np.uint8), T_wc, K, BC.NEAR, c["far"], BC.TRUNC)
    with pytest.raises(ValueError, match="come together"):
        roo.RaycastSdfBricks(*out.images, c["dims"], bmin, bmax, "f32", np.zeros(0, np.uint32), np.zeros((0, 4096), np.uint8), T_wc, K, BC.NEAR, c["far"], BC.TRUNC,
                             cids=np.zeros(0, np.uint32))


def test_gpu_brick_raycast_without_the_sampler_shortcuts(roo):
    """KFX_SAMPLER_SHORTCUTS=0 (read once per process): the comparator's hardware-division and 64-bit address paths, and cell_of's
    hardware division in the brick march -- case C in a fresh child process"""
    env = dict(os.environ, KFX_SAMPLER_SHORTCUTS="0")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "equals_the_dense_raycast and caseC"],
                         env=env, capture_output=True, text=True, timeout=600, cwd=T.ROOT)
    assert out.returncode == 0 and "2 passed" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


def test_gpu_raycast_world_of_a_spilling_pipeline(roo):
    """the set-up of test_gpu_world_mesh_of_a_spilling_pipeline: after (8, 0, -8) both stores hold bricks, and the world seen from the
    first frame's pose is the dense rendering of the 40 x 32 x 40 frame -- more than the shifted volume shows"""
    import torch
    from kangaroo_amd.pipeline import FramePipeline
    N, w, h = 32, 80, 60
    lo, hi = (-1.0, -1.0, 2.0), (0.9375, 0.9375, 3.9375)
    p = FramePipeline(roo, (N, N, N), lo, hi, w, h, track=True, color=True, follow=dict(quantum=8, spill=True))
    T0 = scenes.orbit_pose(0, 8)
    for i in range(3):
        T_wc = scenes.orbit_pose(i, 8)
        raw = T.upload_image(roo, scenes.render_depth("room", w, h, T_wc, p.K))
        rgb = roo.Image(w, h, "u8x3").MemcpyFromHost(scenes.render_rgb("room", w, h, T_wc, p.Kimg))
        p.step(T_wc, raw, rgb)
    assert p.shifts == []
    bits = lambda images: [im.MemcpyToHost().view(np.int32) for im in images]

    def dense(vol, cvol, color, size=(w, h), K=None):
        d, n, i = roo.Image(*size), roo.Image(*size, "f32x4"), roo.Image(*size)
        K = p.K if K is None else K
        if color:
            roo.RaycastSdfColor(d, n, i, vol, cvol, T0, K, p.near, p.far, p.trunc, True)
        else:
            roo.RaycastSdf(d, n, i, vol, T0, K, p.near, p.far, p.trunc, True)
        return bits((d, n, i))

    before = [dense(p.vol, p.cvol, color) for color in (False, True)]
    p.shift_volume((8, 0, -8))
    torch.cuda.synchronize()
    assert len(p.store) > 0 and len(p.cstore) > 0
    view = p.world_view()
    assert view.dims == (40, 32, 40) and view.lo == (0, 0, -8) and view.cids is not None
    D = dense_volume(roo, view.dims, view.boxmin, view.boxmax, "f32", view.ids, view.cells)
    Cv = dense_volume(roo, view.dims, view.boxmin, view.boxmax, "c32", view.cids, view.ccells)
    for color in (False, True):
        want = dense(D, Cv, color)
        pixels, hits = want[0].size, hits_of(want)
        print("world view, colour %s: the comparator hits %d of %d pixels" % (color, hits, pixels))
        assert hits >= BC.HIT_FLOOR * pixels
        assert_same_bits(bits(p.RaycastWorld(T0, color=color)), want, "RaycastWorld")
        assert_same_bits(bits(p.RaycastWorld(T0, color=color, view=view)), want, "RaycastWorld(view=)")
        alone = dense(p.vol, p.cvol, color)
        assert differing(want, alone) > 0, "the world is rendered as the shifted volume alone"
    # another size and other intrinsics, through the same view
    small = (53, 41)
    Ks = scenes.intrinsics(*small)
    assert_same_bits(bits(p.RaycastWorld(T0, K=Ks, w=small[0], h=small[1], view=view)), dense(D, Cv, False, small, Ks), "RaycastWorld at 53 x 41")
    # and back: the frame is the volume again, the world is the live volume's own rendering; the earlier view is still the earlier world
    p.shift_volume((-8, 0, 8))
    torch.cuda.synchronize()
    assert len(p.store) == 0 and len(p.cstore) == 0
    for color in (False, True):
        live = dense(p.vol, p.cvol, color)
        assert_same_bits(bits(p.RaycastWorld(T0, color=color)), live, "RaycastWorld after shifting back")
        assert_same_bits(live, before[int(color)], "the restored volume")
        assert_same_bits(bits(p.RaycastWorld(T0, color=color, view=view)), dense(D, Cv, color), "a view taken before the shift")
    with pytest.raises(ValueError, match="color=True"):
        FramePipeline(roo, (N, N, N), lo, hi, w, h).RaycastWorld(T0, color=True)
    # a pipeline without follow= has no store: it renders its live volume
    q = FramePipeline(roo, (N, N, N), lo, hi, w, h)
    q.step(T0, T.upload_image(roo, scenes.render_depth("room", w, h, T0, q.K)))
    assert q.store is None
    d, n, i = roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h)
    roo.RaycastSdf(d, n, i, q.vol, T0, q.K, q.near, q.far, q.trunc, True)
    want = bits((d, n, i))
    assert hits_of(want) >= BC.HIT_FLOOR * want[0].size
    assert_same_bits(bits(q.RaycastWorld(T0)), want, "RaycastWorld without a store")
    assert_same_bits(bits(q.RaycastWorld(T0, view=q.world_view())), want, "a world view without a store")
