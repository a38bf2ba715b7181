"""Colour mode at the speed of the grey path (include/kfx_color.h):
  * kfx_sdf_fuse_color_tracked changes no SDF or colour cell and keeps a true brick summary;
  * the colour renderings through the class-table march and the all-levels march (march + kfx_raycast_color_hits) equal the
    in-kernel colour of kfx_raycast_sdf_color bit for bit in exact numerics, and stay within the fast-mode tolerance otherwise;
  * views, untracked launches, and the pipelines' colour mode."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import oracle, scenes

pytestmark = pytest.mark.gpu

T_CD = np.array([[1, 0, 0, 0.025], [0, 1, 0, -0.003], [0, 0, 1, 0.002]], np.float32)   # colour <- depth camera (test_color_cpu.color_setup)


def color_pose(T_cw):
    return (np.vstack([T_CD, [0, 0, 0, 1]]) @ np.vstack([T_cw, [0, 0, 0, 1]]))[:3].astype(np.float32)


def upload_rgb(roo, arr):
    im = roo.Image(arr.shape[1], arr.shape[0], "u8x3")
    im.MemcpyFromHost(arr)
    return im


def frame_inputs(roo, scene, w, h, cw, ch, i, maps):
    """The i-th orbit frame: filtered depth and normals (into `maps`, on the GPU), the RGB image, the poses."""
    K, Kimg = scenes.intrinsics(w, h), scenes.intrinsics(cw, ch)
    f, vbo, nrm = maps
    T_wc = scenes.orbit_pose(i, 30)
    roo.BilateralFilter(f, T.upload_image(roo, scenes.render_depth(scene, w, h, T_wc, K)), **scenes.BILATERAL)
    roo.DepthToVbo(vbo, f, K)
    roo.NormalsFromVbo(nrm, vbo)
    T_cw = scenes.se3_inverse(T_wc)
    T_iw = color_pose(T_cw)
    T_wi = scenes.se3_inverse(T_iw)
    rgb = scenes.render_rgb(scene, cw, ch, T_wi, Kimg)
    return dict(T_wc=T_wc, T_cw=T_cw, T_iw=T_iw, rgb_np=rgb, rgb=upload_rgb(roo, rgb))


def images(roo, w, h, vbo=False):
    return [roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h)] + ([roo.Image(w, h, "f32x4")] if vbo else [])


def host(imgs):
    return [x.MemcpyToHost() for x in imgs]


def all_equal(a, b):
    return all(T.nan_equal(x, y) for x, y in zip(host(a), host(b)))


def colour_gradient_bound(cvol):
    """max |difference of neighbouring colour cells| / min voxel edge: how fast a trilinear sample can change per metre"""
    c = cvol.tensor()[..., 0]
    step = max(float((c[1:] - c[:-1]).abs().max()), float((c[:, 1:] - c[:, :-1]).abs().max()), float((c[:, :, 1:] - c[:, :, :-1]).abs().max()))
    return step / float(cvol.VoxelSizeUnits().min())


CASES = [("room", (128, 128, 128), 320, 240, 320, 240), ("full", (96, 96, 96), 160, 120, 192, 144), ("room", (100, 84, 92), 200, 150, 160, 120)]


@pytest.mark.parametrize("scene,dims,w,h,cw,ch", CASES)
@pytest.mark.parametrize("math", ["exact", "fast"])
def test_gpu_colour_tracked_fuse_and_table_march(roo, scene, dims, w, h, cw, ch, math):
    """(1) tracked colour fusion changes no value and keeps a true summary; (2) colour through the table march."""
    from test_gpu_summary import export, check_conservative, check_classes
    bmin, bmax, near, far = scenes.SCENES[scene]
    K, Kimg = scenes.intrinsics(w, h), scenes.intrinsics(cw, ch)
    tr = scenes.trunc_dist(bmin, bmax, dims)
    with_oracle = math == "exact" and dims != (128, 128, 128)
    prev = roo.set_math_mode(math)
    try:
        va, vb = roo.BoundedVolume(*dims, bmin, bmax), roo.BoundedVolume(*dims, bmin, bmax)
        ca, cb = roo.BoundedVolume(*dims, bmin, bmax, kind="c32"), roo.BoundedVolume(*dims, bmin, bmax, kind="c32")
        summ = roo.SdfSummary(vb)
        roo.SdfReset(va, float("nan"))
        roo.SdfReset(vb, float("nan"), summary=summ)
        roo.ColorReset(ca)
        roo.ColorReset(cb)
        if with_oracle:
            ov, oc = oracle.Volume(*dims, bmin, bmax), oracle.ColorVolume(*dims, bmin, bmax)
            oracle.sdf_reset(ov, float("nan"))
            oracle.color_reset(oc)
        maps = (roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h, "f32x4"))
        tol = 1e-5 if math == "fast" else 0.0
        for i in range(4):
            fr = frame_inputs(roo, scene, w, h, cw, ch, i, maps)
            args = (maps[0], maps[2], fr["T_cw"], K, fr["rgb"], fr["T_iw"], Kimg, tr, scenes.MAX_W, scenes.MIN_COS_THETA)
            roo.SdfFuseColor(va, ca, *args)
            roo.SdfFuseColor(vb, cb, *args, summary=summ)
            # (1) tracking changes neither volume
            sdf_a, col_a = va.MemcpyToHost(), ca.MemcpyToHost()
            assert T.nan_equal(sdf_a, vb.MemcpyToHost()) and T.nan_equal(col_a, cb.MemcpyToHost())
            if with_oracle:
                of, on = oracle.Image.from_numpy(maps[0].MemcpyToHost()), oracle.Image.from_numpy(maps[2].MemcpyToHost())
                orgb = oracle.Image(cw, ch, np.uint8, 3)
                orgb.data[...] = fr["rgb_np"]
                oracle.sdf_fuse_color(ov, oc, of, on, fr["T_cw"], K, orgb, fr["T_iw"], Kimg, tr, scenes.MAX_W, scenes.MIN_COS_THETA, nthreads=0)
                assert T.nan_equal(sdf_a, ov.data), T.mismatch_report(sdf_a, ov.data)
                assert T.nan_equal(col_a, oc.data), T.mismatch_report(col_a, oc.data)
            # the summary covers the volume's real contents, and is kept (not just invalidated)
            R, classes = export(roo, summ, tol, tr, fine_shift=4)
            stats = check_conservative(vb, R)
            check_classes(vb, classes, tol, np.float32(tr))
            R, classes = export(roo, summ, tol, tr, fine_shift=3)
            counts = check_classes(vb, classes, tol, np.float32(tr))
            n_free, n_entries = counts[3][1] + counts[3][3], classes[3].numel()
            print("frame %d: free 8^3 entries %d of %d, %s" % (i, n_free, n_entries, stats))
            if math == "exact":
                if i == 0 and all(d % 8 == 0 for d in dims):
                    assert n_free > 0
            else:
                assert n_free > (0.05 if dims[0] % 8 == 0 else 0.02) * n_entries, (n_free, n_entries, stats)
            # (2) colour through the table march
            a, b = images(roo, w, h), images(roo, w, h)
            roo.set_math_mode("exact")
            roo.RaycastSdfColor(*a, va, ca, fr["T_wc"], K, near, far, tr, True)              # the reference march, colour in the kernel
            roo.set_math_mode(math)
            roo.RaycastSdfColor(*b, vb, cb, fr["T_wc"], K, near, far, tr, True, summary=summ)
            (da, na, ia), (db, nb, ib) = host(a), host(b)
            if math == "exact":
                assert T.nan_equal(da, db) and T.nan_equal(na, nb)
                assert T.nan_equal(ia, ib), T.mismatch_report(ia, ib)
                if with_oracle:
                    od, onn, oi = oracle.Image(w, h), oracle.Image(w, h, channels=4), oracle.Image(w, h)
                    oracle.raycast_sdf_color(od, onn, oi, ov, oc, fr["T_wc"], K, near, far, tr, True, nthreads=0)
                    assert T.nan_equal(db, od.data) and T.nan_equal(nb, onn.data)
                    assert T.nan_equal(ib, oi.data), T.mismatch_report(ib, oi.data)
            else:
                hit_a, hit_b = np.isfinite(da), np.isfinite(db)
                assert (hit_a != hit_b).sum() <= max(3, 2e-4 * w * h), (hit_a != hit_b).sum()
                both = hit_a & hit_b
                assert both.sum() > 0.03 * w * h
                assert np.abs(da[both] - db[both]).max() < 1e-4, np.abs(da[both] - db[both]).max()
                cosang = np.clip(np.sum(na[both][:, :3].astype(np.float64) * nb[both][:, :3], axis=1), -1, 1)
                assert np.arccos(cosang).max() < 2e-3
                # the project's depth tolerance times how fast the colour can change along any direction
                bound = 1e-4 * np.sqrt(3.0) * colour_gradient_bound(cb) + 1e-6
                worst = float(np.abs(ia[both] - ib[both]).max())
                print("frame %d: colour difference on common hits %.3g (bound %.3g)" % (i, worst, bound))
                assert worst <= bound, (worst, bound)
                assert (ib[~hit_b] == 0).all()
    finally:
        roo.set_math_mode(prev)


def fused_model(roo, scene, dims, w, h, frames=2, summary=True):
    bmin, bmax, near, far = scenes.SCENES[scene]
    K = scenes.intrinsics(w, h)
    tr = scenes.trunc_dist(bmin, bmax, dims)
    vol, cvol = roo.BoundedVolume(*dims, bmin, bmax), roo.BoundedVolume(*dims, bmin, bmax, kind="c32")
    summ = roo.SdfSummary(vol)
    roo.SdfReset(vol, float("nan"), summary=summ)
    roo.ColorReset(cvol)
    maps = (roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h, "f32x4"))
    for i in range(frames):
        fr = frame_inputs(roo, scene, w, h, w, h, i, maps)
        roo.SdfFuseColor(vol, cvol, maps[0], maps[2], fr["T_cw"], K, fr["rgb"], fr["T_iw"], K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, summary=summ)
    return vol, cvol, summ, K, tr, near, far, fr["T_wc"]


@pytest.mark.parametrize("math", ["exact", "fast"])
def test_gpu_colour_pass_equals_the_in_kernel_colour(roo, math):
    """(3) RaycastSdf followed by kfx_raycast_color_hits = kfx_raycast_sdf_color, all three images, in both numerics modes --
    also with the whole colour volume beside a SubBoundingVolume of the SDF volume (main.cpp:284)."""
    N, w, h = 128, 320, 240
    prev = roo.set_math_mode(math)
    try:
        vol, cvol, summ, K, tr, near, far, T_wc = fused_model(roo, "room", (N, N, N), w, h)
        sub = vol.SubBoundingVolume((-0.6, -0.7, 2.4), (0.7, 0.5, 3.9))
        assert (sub.w, sub.h, sub.d) != (N, N, N)
        for v in (vol, sub):
            a, b = images(roo, w, h), images(roo, w, h)
            roo.RaycastSdfColor(*a, v, cvol, T_wc, K, near, far, tr, True)
            roo.RaycastSdf(*b, v, T_wc, K, near, far, tr, True)
            grey = b[2].MemcpyToHost()
            roo.RaycastColorHits([(b[0], b[2])], cvol, T_wc, [K])
            assert all_equal(a, b)
            hit = np.isfinite(b[0].MemcpyToHost())
            assert hit.mean() > 0.05 and not T.nan_equal(grey, b[2].MemcpyToHost())   # the pass did write: the Phong shade is gone
    finally:
        roo.set_math_mode(prev)


@pytest.mark.parametrize("scene", ["room", "full"])
def test_gpu_colour_renderings_of_pyramid_levels(roo, scene):
    """(4) RaycastSdfColorLevels, with and without the summary: every image and vertex map equals the per-level
    RaycastSdfColor (+ DepthToVbo) of the same numerics mode."""
    N, w, h = 128, 320, 240
    prev = roo.set_math_mode("exact")
    try:
        vol, cvol, summ, K, tr, near, far, T_wc = fused_model(roo, scene, (N, N, N), w, h)
        levels = [0, 2, 3]
        Ks = [scenes.intrinsics_level(K, l) for l in levels]
        for math in ("exact", "fast"):
            roo.set_math_mode(math)
            for s in (None, summ):
                one = [images(roo, w >> l, h >> l, vbo=True) for l in levels]
                roo.RaycastSdfColorLevels([tuple(o) for o in one], vol, cvol, T_wc, Ks, near, far, tr, True, summary=s)
                for o, l, Kl in zip(one, levels, Ks):
                    ref = images(roo, w >> l, h >> l, vbo=True)
                    roo.RaycastSdfColor(ref[0], ref[1], ref[2], vol, cvol, T_wc, Kl, near, far, tr, True, summary=s)
                    roo.DepthToVbo(ref[3], ref[0], Kl)
                    assert all_equal(o, ref), (math, l, s is not None)
                    if math == "exact" and s is not None:   # ... which in exact numerics is the plain colour march
                        plain = images(roo, w >> l, h >> l)
                        roo.RaycastSdfColor(*plain, vol, cvol, T_wc, Kl, near, far, tr, True)
                        assert all_equal(o[:3], plain), l
                    assert np.isfinite(o[0].MemcpyToHost()).sum() > 0.02 * (w >> l) * (h >> l)
    finally:
        roo.set_math_mode(prev)


def test_gpu_colour_summary_views_and_untracked_launches(roo):
    """(5) 8-aligned views (SDF and colour) keep tracking; an unaligned view or a launch that takes the untiled kernel (odd
    extent) leaves every entry unknown; the images always equal the plain colour march (exact numerics)."""
    from test_gpu_summary import export, check_conservative, check_classes
    N, w, h = 96, 160, 120
    bmin, bmax, near, far = scenes.SCENES["room"]
    K = scenes.intrinsics(w, h)
    tr = scenes.trunc_dist(bmin, bmax, (N, N, N))
    vol, cvol = roo.BoundedVolume(N, N, N, bmin, bmax), roo.BoundedVolume(N, N, N, bmin, bmax, kind="c32")
    summ = roo.SdfSummary(vol)
    maps = (roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h, "f32x4"))
    fr = frame_inputs(roo, "room", w, h, w, h, 1, maps)

    def fuse(start, size, **kw):
        roo.SdfFuseColor(vol.SubVolume(start, size), cvol.SubVolume(start, size), maps[0], maps[2], fr["T_cw"], K, fr["rgb"], fr["T_iw"], K, tr,
                         scenes.MAX_W, scenes.MIN_COS_THETA, summary=summ, **kw)

    def same_images(v):
        a, b = images(roo, w, h), images(roo, w, h)
        roo.RaycastSdfColor(*a, v, cvol, fr["T_wc"], K, near, far, tr, True)
        roo.RaycastSdfColor(*b, v, cvol, fr["T_wc"], K, near, far, tr, True, summary=summ)
        return all_equal(a, b)

    def all_unknown():
        R, classes = export(roo, summ, 0.0, tr)
        return check_conservative(vol, R)["mixed"] == R.shape[0] * R.shape[1] * R.shape[2] and all(int((c != 0).sum()) == 0 for c in classes.values())

    def reset():
        roo.SdfReset(vol, float("nan"), summary=summ)
        roo.ColorReset(cvol)

    reset()
    assert same_images(vol)
    fuse((16, 8, 24), (64, 80, 56))
    R, classes = export(roo, summ, 0.0, tr)
    st = check_conservative(vol, R)
    check_classes(vol, classes, 0.0, np.float32(tr))
    assert st["uniform_ranges"] > 0 and st["all_nan"] > 0 and st["mixed"] > 0, st
    assert same_images(vol) and same_images(vol.SubVolume((16, 8, 24), (64, 80, 56)))
    fuse((3, 8, 24), (64, 80, 56))                       # a view that does not start on multiples of 8 cells
    assert all_unknown() and same_images(vol)
    reset()
    fuse((16, 8, 24), (63, 80, 56), full_extent=True)    # an odd extent: the untiled k_sdf_fuse_color
    assert all_unknown() and same_images(vol)
    assert int(np.isfinite(vol.MemcpyToHost()[..., 0]).sum()) > 0


UNTILED_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %(tests)r)
import kfx_testlib as T
from kfx_testlib import scenes
from kangaroo_amd import roo
import test_gpu_colour_tracked as M
from test_gpu_summary import export, check_conservative
vol, cvol, summ, K, tr, near, far, T_wc = M.fused_model(roo, "room", (96, 96, 96), 160, 120, frames=1)
R, classes = export(roo, summ, 0.0, tr)
assert check_conservative(vol, R)["mixed"] == R.shape[0] * R.shape[1] * R.shape[2] and all(int((c != 0).sum()) == 0 for c in classes.values())
a, b = M.images(roo, 160, 120), M.images(roo, 160, 120)
roo.RaycastSdfColor(*a, vol, cvol, T_wc, K, near, far, tr, True)
roo.RaycastSdfColor(*b, vol, cvol, T_wc, K, near, far, tr, True, summary=summ)
assert M.all_equal(a, b) and np.isfinite(a[0].MemcpyToHost()).mean() > 0.2
print("untiled-ok")
"""


def test_gpu_colour_untiled_kernel_invalidates_the_summary(tmp_path):
    """(5) KFX_FUSE_TILED=0 (read once per process): the tracked colour call runs k_sdf_fuse_color and says so in the summary."""
    script = tmp_path / "untiled.py"
    script.write_text(UNTILED_CHILD % {"tests": os.path.join(T.ROOT, "tests")})
    env = dict(os.environ, KFX_FUSE_TILED="0", KFX_RAYCAST_SUMMARY="1")
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "untiled-ok" in out.stdout, out.stdout + out.stderr


# ---- (6) pipelines ------------------------------------------------------------------------------------------------------
def run_frame_pipeline(roo, track, frames=6):
    from kangaroo_amd.pipeline import FramePipeline
    N, w, h = 64, 160, 120
    bmin, bmax, near, far = scenes.SCENES["room"]
    pipe = FramePipeline(roo, (N, N, N), bmin, bmax, w, h, near=near, far=far, track=track, color=True, T_cd=T_CD)
    assert pipe.kframe is None
    out = []
    for i in range(frames):
        T_wc = scenes.orbit_pose(i, 30)
        pipe.raw.MemcpyFromHost(scenes.render_depth("room", w, h, T_wc, pipe.K))
        pipe.rgb.MemcpyFromHost(scenes.render_rgb("room", w, h, scenes.se3_inverse(color_pose(scenes.se3_inverse(T_wc))), pipe.Kimg))
        pipe.step(T_wc)
        out.append(host([pipe.ray_d, pipe.ray_n, pipe.ray_i, pipe.filtered, pipe.normals]))
    return pipe, out


def test_gpu_frame_pipeline_colour_mode(roo):
    """FramePipeline(color=True): tracked and plain give the same volumes and images, and both equal a loop of oracle calls on the
    same inputs (the pipeline's filtered depth and normals: the bilateral filter's exponentials are not the host's bit for bit)."""
    import torch
    N, w, h, frames = 64, 160, 120, 6
    bmin, bmax, near, far = scenes.SCENES["room"]
    prev = roo.set_math_mode("exact")
    try:
        pt, img_t = run_frame_pipeline(roo, True, frames)
        pp, img_p = run_frame_pipeline(roo, False, frames)
        assert pt.track and pt.summary is not None and not pp.track
        vt, ct = pt.vol.MemcpyToHost(), pt.cvol.MemcpyToHost()
        assert T.nan_equal(vt, pp.vol.MemcpyToHost()) and T.nan_equal(ct, pp.cvol.MemcpyToHost())
        K, tr = pt.K, pt.trunc
        ov, oc = oracle.Volume(N, N, N, bmin, bmax), oracle.ColorVolume(N, N, N, bmin, bmax)
        oracle.sdf_reset(ov, float("nan"))
        oracle.color_reset(oc)
        for i in range(frames):
            T_wc = scenes.orbit_pose(i, 30)
            T_cw = scenes.se3_inverse(T_wc)
            T_iw = color_pose(T_cw)
            assert T.nan_equal(img_t[i][3], img_p[i][3]) and T.nan_equal(img_t[i][4], img_p[i][4])
            f, nrm = oracle.Image.from_numpy(img_t[i][3]), oracle.Image.from_numpy(img_t[i][4])
            rgb = oracle.Image(w, h, np.uint8, 3)
            rgb.data[...] = scenes.render_rgb("room", w, h, scenes.se3_inverse(T_iw), pt.Kimg)
            oracle.sdf_fuse_color(ov, oc, f, nrm, T_cw, K, rgb, T_iw, pt.Kimg, tr, scenes.MAX_W, scenes.MIN_COS_THETA, nthreads=0)
            od, on, oi = oracle.Image(w, h), oracle.Image(w, h, channels=4), oracle.Image(w, h)
            oracle.raycast_sdf_color(od, on, oi, ov, oc, T_wc, K, near, far, tr, True, nthreads=0)
            for got in (img_t[i], img_p[i]):
                assert T.nan_equal(got[0], od.data) and T.nan_equal(got[1], on.data), i
                assert T.nan_equal(got[2], oi.data), (i, T.mismatch_report(got[2], oi.data))
        assert T.nan_equal(vt, ov.data) and T.nan_equal(ct, oc.data)
        assert np.isfinite(img_t[-1][0]).mean() > 0.2
        # fast against exact: the thresholds of test_gpu_colour_fusion_fast_mode
        roo.set_math_mode("fast")
        pf, _ = run_frame_pipeline(roo, True, frames)
        a, ca, b, cb = pt.vol.tensor(), pt.cvol.tensor(), pf.vol.tensor(), pf.cvol.tensor()
        na, nb = torch.isnan(a[..., 0]), torch.isnan(b[..., 0])
        assert int((na != nb).sum()) <= 20
        both = ~na & ~nb
        d = (a[..., 0][both] - b[..., 0][both]).abs()
        assert float((d > 1e-4).float().mean()) < 1e-4 and float(d.median()) < 1e-6
        dc = (ca[..., 0][both] - cb[..., 0][both]).abs()
        assert float((dc > 2e-3).float().mean()) < 1e-4, float(dc.max())
        assert float(dc.median()) < 1e-6
    finally:
        roo.set_math_mode(prev)


def test_gpu_tracking_pipeline_colour_mode(roo):
    """TrackingPipeline(color=True) at the size of test_gpu_tracking_pipeline_follows_the_orbit: the tables and the one-launch
    rendering change no pose and no cell (exact numerics), no frame is lost, the position error stays within that test's bound."""
    from kangaroo_amd.pipeline import TrackingPipeline
    N, w, h, frames = 128, 640, 480, 8
    bmin, bmax, near, far = scenes.SCENES["room"]
    K = scenes.intrinsics(w, h)
    truth = [scenes.orbit_pose(i, 30) for i in range(frames)]
    depth = [scenes.render_depth("room", w, h, P, K) for P in truth]
    rgbs = [scenes.render_rgb("room", w, h, scenes.se3_inverse(color_pose(scenes.se3_inverse(P))), K) for P in truth]
    drift_if_static = float(np.linalg.norm(truth[-1][:3, 3] - truth[0][:3, 3]))
    prev = roo.set_math_mode("exact")
    try:
        runs = {}
        for track, one in ((True, True), (False, True), (True, False)):
            pipe = TrackingPipeline(roo, (N, N, N), bmin, bmax, w, h, near=near, far=far, track=track, one_raycast=one, color=True, T_cd=T_CD)
            assert pipe.one_raycast == one and pipe.track == track
            poses, worst = [], 0.0
            for i in range(frames):
                pipe.raw.MemcpyFromHost(depth[i])
                pipe.rgb.MemcpyFromHost(rgbs[i])
                T_est = pipe.step(T_wl_init=truth[i] if i == 0 else None)
                assert pipe.tracking_good and np.isfinite(pipe.rmse), (track, one, i)
                poses.append(T_est.copy())
                worst = max(worst, float(np.linalg.norm(T_est[:3, 3] - truth[i][:3, 3])))
            assert pipe.resets == 0 and worst < 0.2 * drift_if_static, (track, one, worst, drift_if_static)
            runs[(track, one)] = (poses, pipe.vol.MemcpyToHost(), pipe.cvol.MemcpyToHost(), host([pipe.pyr_i[0]])[0])
        ref = runs[(True, True)]
        for key in ((False, True), (True, False)):
            got = runs[key]
            assert all(np.array_equal(p, q) for p, q in zip(ref[0], got[0])), key
            assert T.nan_equal(ref[1], got[1]) and T.nan_equal(ref[2], got[2]) and T.nan_equal(ref[3], got[3]), key
        c = ref[2][..., 0]
        assert ((c != 0.5) & (c >= 0) & (c <= 1)).any() and np.ptp(ref[3][np.isfinite(ref[3]) & (ref[3] > 0)]) > 0.05   # the rendering shows the albedo
    finally:
        roo.set_math_mode(prev)
