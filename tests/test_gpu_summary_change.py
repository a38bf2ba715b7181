"""The class tables are rebuilt only when a brick changes its class (summary.hip, summary_classes_prepare): a table build that
follows nothing but tracked SdfFuse launches is conditional -- its two launches return at once unless one of those launches saw a
brick change its class mask (brick_class_mask, kfx_device.h) -- and every other writer of the summary forces a build.
  * streams of 90 frames from SdfReset (S_room and S_full, exact and fast numerics, fp32 and half cells, fine levels of 8^3 and
    of 16^3 cells): after every frame the tables the library holds equal, word for word and with the same published count, the
    tables a forced build makes from the same brick ranges, and they hold against the real cells;
  * conditional builds really build (the first frames of every stream) and really return early (fast numerics, S_full, once the
    first orbit is over -- after the test has checked on the volume itself that no brick sits on the edge of the tables' band);
  * exact numerics: the tracked images equal the plain march's bit for bit on every frame, also where no ray enters the box;
  * after every other writer (reset, invalidate, rebuild, a pipeline that stopped tracking for a while, a fuse on a sub-volume
    view, an untracked fuse + invalidate) the next tables are the forced build's."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import scenes
from test_gpu_summary import export, check_classes
from test_gpu_half_summary import band, vref_of, check_classes as check_classes_h

pytestmark = pytest.mark.gpu

W, H = 160, 120
ORBIT = 30


def debug_lib():
    from kangaroo_amd import _lib
    L = _lib.load_debug()
    L.kfx_debug_summary_export.restype = C.c_int
    L.kfx_debug_summary_export.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
    L.kfx_debug_summary_conditional_builds.restype = C.c_int
    L.kfx_debug_summary_conditional_builds.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
    return L


def layout(summ, shift):
    dims = (C.c_int * 12)()
    assert debug_lib().kfx_debug_summary_export(summ.handle, 0.0, 1.0, shift, None, None, dims, None) == 0   # (no table is built without C_out)
    return list(dims)


def shift_used(summ):
    """class_view's rule (raycast.hip): the finest level whose tables fit KFX_RAYCAST_CLASS_KB (default 16) KiB."""
    kb = min(max(int(os.environ.get("KFX_RAYCAST_CLASS_KB", "16")), 1), 60)
    for s in (3, 4):
        if layout(summ, s)[9] * 4 <= kb * 1024:
            return s
    return 5


def conditional_builds(summ):
    """(conditional builds that built, conditional builds that returned early) since the summary was created"""
    out = (C.c_int * 2)()
    assert debug_lib().kfx_debug_summary_conditional_builds(summ.handle, out, None) == 0
    return out[0], out[1]


def tables(summ, tol, vref, shift):
    """The words of the two levels (padding between them left out) and the published count of the tables for (tol, vref, shift):
    the library's own if it holds tables for these parameters and knows of no writer since, else a build."""
    import torch
    dims = layout(summ, shift)
    Cw = torch.zeros(dims[9], dtype=torch.int32, device="cuda")
    out = (C.c_int * 12)()
    assert debug_lib().kfx_debug_summary_export(summ.handle, tol, vref, shift, None, C.c_void_p(Cw.data_ptr()), out, None) == 0
    torch.cuda.synchronize()
    d = summ.vol.d
    parts = [Cw[first:first + rw * ny * -(-d // (1 << s))] for s, (first, rw, ny) in ((shift, dims[3:6]), (5, dims[6:9])) if s == 5 or shift < 5]
    return torch.cat(parts).clone(), out[11]


def held_equal_forced(roo, summ, vol, tol, vref, shift, check):
    """The tables the library holds for the march's own parameters against a forced build from the same brick ranges (a build
    for the other fine level in between: a change of parameters forces), and against the volume's real cells."""
    import torch
    held, held_count = tables(summ, tol, vref, shift)
    export(roo, summ, tol, vref, fine_shift=4 if shift == 3 else 3)
    forced, forced_count = tables(summ, tol, vref, shift)
    differ = int((held != forced).sum())
    assert differ == 0, "%d table words differ from a forced build's" % differ
    assert held_count == forced_count, (held_count, forced_count)
    _, classes = export(roo, summ, tol, vref, fine_shift=shift)   # (decodes, and compares the published count with the 32^3-cell level)
    check(vol, classes, tol, np.float32(vref) if vol.kind == "f32" else vref)
    return classes


def images(roo):
    return [roo.Image(W, H), roo.Image(W, H, "f32x4"), roo.Image(W, H)]


def bit_equal(a, b):
    return all(T.nan_equal(x.MemcpyToHost(), y.MemcpyToHost()) for x, y in zip(a, b))


def frame_inputs(roo, scene, K, i, cache):
    if i % ORBIT not in cache:
        T_wc = scenes.orbit_pose(i % ORBIT, ORBIT)
        f, vbo, nrm = roo.Image(W, H), roo.Image(W, H, "f32x4"), roo.Image(W, H, "f32x4")
        roo.BilateralFilter(f, T.upload_image(roo, scenes.render_depth(scene, W, H, T_wc, K)), **scenes.BILATERAL)
        roo.DepthToVbo(vbo, f, K)
        roo.NormalsFromVbo(nrm, vbo)
        cache[i % ORBIT] = (T_wc, f, nrm)
    return cache[i % ORBIT]


def no_brick_on_the_edge_of_the_band(vol, tr, tol):
    """Per 8^3 brick: the lowest valued cell is either +trunc as far as the tables can tell (>= (1 - tol) trunc) or well inside the
    truncation band (< (1 - 1e-3) trunc): no brick whose class a rounding could flip from frame to frame."""
    import torch
    v = vol.tensor()[..., 0].float()
    d, h, w = v.shape
    assert d % 8 == 0 and h % 8 == 0 and w % 8 == 0
    br = v.view(d // 8, 8, h // 8, 8, w // 8, 8).permute(0, 2, 4, 1, 3, 5).reshape(-1, 512)
    lo = torch.where(torch.isnan(br), torch.full_like(br, float("inf")), br).amin(-1)
    lo = lo[torch.isfinite(lo)]
    edge = (lo < (1.0 - tol) * tr) & (lo >= (1.0 - 1e-3) * tr)
    return int(edge.sum()), int(lo.numel())


def away_pose():
    """a camera that looks away from the box: no ray enters it"""
    return np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 0]], np.float32)


def run_stream(roo, scene, N, math, kind, frames=90):
    """One stream; returns its figures (the assertions on the tables are made here, frame by frame)."""
    bmin, bmax, near, far = scenes.SCENES[scene]
    K = scenes.intrinsics(W, H)
    tr = scenes.trunc_dist(bmin, bmax, (N, N, N))
    half = kind == "f16"
    vref = vref_of(tr) if half else tr
    tol = (band() if half else 1e-5) if math == "fast" else 0.0
    check = check_classes_h if half else check_classes
    prev = roo.set_math_mode(math)
    try:
        vol = roo.BoundedVolume(N, N, N, bmin, bmax, kind=kind) if half else roo.BoundedVolume(N, N, N, bmin, bmax)
        summ = roo.SdfSummary(vol)
        shift = shift_used(summ)
        roo.SdfReset(vol, float("nan"), summary=summ)
        # the empty model rendered first (SdfReset forces that build): from here on every build of the stream is conditional, and
        # the first frame's must really build -- every brick it observes changes its class
        roo.RaycastSdf(*images(roo), vol, scenes.orbit_pose(0, ORBIT), K, near, far, tr, True, summary=summ)
        assert conditional_builds(summ) == (0, 0)
        held_equal_forced(roo, summ, vol, tol, vref, shift, check)
        cache, per_frame, nonzero = {}, [], 0
        for i in range(frames):
            T_wc, f, nrm = frame_inputs(roo, scene, K, i, cache)
            before = conditional_builds(summ)
            roo.SdfFuse(vol, f, nrm, scenes.se3_inverse(T_wc), K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, summary=summ)
            b = images(roo)
            roo.RaycastSdf(*b, vol, T_wc, K, near, far, tr, True, summary=summ)
            after = conditional_builds(summ)
            built, early = after[0] - before[0], after[1] - before[1]
            # the call follows this function's own forced builds and a tracked SdfFuse: conditional
            assert built + early == 1, (i, built, early)
            assert i > 0 or built == 1
            per_frame.append((built, early))
            classes = held_equal_forced(roo, summ, vol, tol, vref, shift, check)
            nonzero = max(nonzero, int((classes[5] != 0).sum()))
            if math == "exact":
                a = images(roo)
                roo.RaycastSdf(*a, vol, T_wc, K, near, far, tr, True)
                assert bit_equal(a, b), (scene, N, kind, i)
                assert np.isfinite(a[0].MemcpyToHost()).sum() > 0.02 * W * H
                if i % 15 == 0:
                    a, b = images(roo), images(roo)
                    roo.RaycastSdf(*a, vol, away_pose(), K, near, far, tr, True)
                    roo.RaycastSdf(*b, vol, away_pose(), K, near, far, tr, True, summary=summ)
                    assert bit_equal(a, b) and not np.isfinite(a[0].MemcpyToHost()).any()
        res = dict(scene=scene, N=N, math=math, kind=kind, shift=shift,
                   built=sum(p[0] for p in per_frame), early=sum(p[1] for p in per_frame),
                   built_first_orbit=sum(p[0] for p in per_frame[:ORBIT]), early_after_first_orbit=sum(p[1] for p in per_frame[ORBIT:]),
                   coarse_entries_nonzero=nonzero)
        if math == "fast" and scene == "full":
            res["bricks_on_edge"], res["bricks_valued"] = no_brick_on_the_edge_of_the_band(vol, tr, tol)
        print("stream", json.dumps(res), flush=True)
        assert res["built_first_orbit"] > 0, res   # the scene is being discovered: bricks change class, the tables are rebuilt
        if "bricks_on_edge" in res:
            # the wall is fixed in the volume's frame: once the orbit has been seen no brick changes class, and the builds must
            # return early.  fp32 cells: checked first on the volume itself that no brick sits on the edge of the tables' 1e-5
            # (half cells: the band is 2^-3 wide and cells inside it drift; the figure is printed)
            if not half:
                assert res["bricks_on_edge"] == 0 and res["bricks_valued"] > 0, res
            assert res["early_after_first_orbit"] > 0, res
        return res
    finally:
        roo.set_math_mode(prev)


STREAMS = [("full", 128, "fast", "f32"), ("full", 96, "exact", "f32"), ("room", 96, "fast", "f32"), ("room", 128, "exact", "f32"),
           ("full", 96, "fast", "f16"), ("room", 96, "exact", "f16")]


@pytest.mark.parametrize("scene,N,math,kind", STREAMS)
def test_gpu_tables_of_a_stream_equal_forced_builds(roo, scene, N, math, kind):
    """Fine level of 8^3 cells (what class_view picks at these sizes).  Figures of the streams: printed (pytest -s)."""
    import torch
    res = run_stream(roo, scene, N, math, kind)
    assert res["shift"] == 3
    torch.cuda.synchronize()


@pytest.mark.parametrize("scene,N,math,kind", [("full", 128, "fast", "f32"), ("room", 128, "exact", "f32"), ("full", 128, "fast", "f16")])
def test_gpu_tables_of_a_stream_equal_forced_builds_16_cell_fine_level(scene, N, math, kind):
    """KFX_RAYCAST_CLASS_KB=1 makes class_view pick the 16^3-cell fine level (the headline's, at 512^3) at these sizes; the knob
    is read once, so the stream runs in a process of its own."""
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" % (T.ROOT, os.path.join(T.ROOT, "tests")) + \
           "import test_gpu_summary_change as M\nfrom kangaroo_amd import roo\n" + \
           "res = M.run_stream(roo, %r, %d, %r, %r)\nassert res['shift'] == 4, res\nprint('STREAM_OK')\n" % (scene, N, math, kind)
    env = dict(os.environ)
    env["KFX_RAYCAST_CLASS_KB"] = "1"
    env["KFX_RAYCAST_SUMMARY"] = "1"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)
    print(out.stdout)
    assert out.returncode == 0 and "STREAM_OK" in out.stdout, out.stdout + out.stderr


def test_gpu_other_writers_force_a_build(roo):
    """SdfReset(tracked), invalidate, rebuild, a fuse on a sub-volume view, an untracked SdfFuse followed by invalidate: after each,
    the tables the next tracked RaycastSdf marches through are those of a forced build."""
    N = 96
    scene = "room"
    bmin, bmax, near, far = scenes.SCENES[scene]
    K = scenes.intrinsics(W, H)
    tr = scenes.trunc_dist(bmin, bmax, (N, N, N))
    prev = roo.set_math_mode("fast")
    try:
        vol = roo.BoundedVolume(N, N, N, bmin, bmax)
        summ = roo.SdfSummary(vol)
        shift = shift_used(summ)
        roo.SdfReset(vol, float("nan"), summary=summ)
        cache = {}

        def fuse(i, v=vol, **kw):
            T_wc, f, nrm = frame_inputs(roo, scene, K, i, cache)
            roo.SdfFuse(v, f, nrm, scenes.se3_inverse(T_wc), K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, **kw)
            return T_wc

        def march_and_check(T_wc):
            roo.RaycastSdf(*images(roo), vol, T_wc, K, near, far, tr, True, summary=summ)
            return held_equal_forced(roo, summ, vol, 1e-5, tr, shift, check_classes)

        for i in range(6):
            march_and_check(fuse(i, summary=summ))
        n0 = conditional_builds(summ)
        roo.SdfReset(vol, float("nan"), summary=summ)                       # kfx_sdf_reset_tracked
        c = march_and_check(scenes.orbit_pose(0, ORBIT))
        assert int((c[5] == 2).sum()) == c[5].numel()
        march_and_check(fuse(6, summary=summ))
        roo.SdfSphere(vol, (0.0, 0.0, 3.0), 0.5)
        summ.invalidate()                                                   # kfx_sdf_summary_invalidate
        c = march_and_check(scenes.orbit_pose(1, ORBIT))
        assert int((c[5] != 0).sum()) == 0
        summ.rebuild()                                                      # kfx_sdf_summary_rebuild
        march_and_check(scenes.orbit_pose(2, ORBIT))
        roo.SdfReset(vol, float("nan"), summary=summ)
        for i in range(3):
            march_and_check(fuse(i, summary=summ))
        view = vol.SubVolume((16, 8, 24), (64, 80, 56))                     # an 8-aligned view keeps tracking: conditional
        march_and_check(fuse(3, v=view, summary=summ))
        ragged = vol.SubVolume((3, 8, 24), (64, 80, 56))                    # an unaligned one cannot: invalidated inside the call
        c = march_and_check(fuse(4, v=ragged, summary=summ))
        assert int((c[5] != 0).sum()) == 0
        summ.rebuild()
        march_and_check(fuse(5, summary=summ))
        fuse(6)                                                             # an untracked SdfFuse ...
        summ.invalidate()                                                   # ... and what its caller owes the summary
        march_and_check(scenes.orbit_pose(6, ORBIT))
        n1 = conditional_builds(summ)
        print("conditional builds of the writers' test: built %d, early %d" % (n1[0] - n0[0], n1[1] - n0[1]))
    finally:
        roo.set_math_mode(prev)


def test_gpu_pipeline_that_stopped_tracking_for_a_while(roo):
    """FramePipeline.set_track(False) -> frames -> set_track(True): the summary went stale in between and is rebuilt from the
    volume; the next tables are the forced build's, and so are those of the tracked frames that follow."""
    from kangaroo_amd.pipeline import FramePipeline
    N, scene = 96, "room"   # (discovered over many frames: conditional builds that build, and others that return early)
    bmin, bmax, near, far = scenes.SCENES[scene]
    prev = roo.set_math_mode("fast")
    try:
        pipe = FramePipeline(roo, (N, N, N), bmin, bmax, W, H, near=near, far=far, track=True)
        assert pipe.kframe is not None
        frames = [T.upload_image(roo, scenes.render_depth(scene, W, H, scenes.orbit_pose(i, ORBIT), pipe.K)) for i in range(ORBIT)]

        class Summ:   # the frame's own summary in the shape export() takes
            pass

        def check():
            s = Summ()
            s.handle, s.vol = pipe.summary.handle, pipe.vol
            held_equal_forced(roo, s, pipe.vol, 1e-5, pipe.trunc, shift_used(s), check_classes)
            return conditional_builds(s)

        for i in range(40):
            pipe.step(scenes.orbit_pose(i % ORBIT, ORBIT), frames[i % ORBIT])
            n0 = check()
        pipe.set_track(False)
        for i in range(40, 46):
            pipe.step(scenes.orbit_pose(i % ORBIT, ORBIT), frames[i % ORBIT])
        pipe.set_track(True)
        for i in range(46, 60):
            pipe.step(scenes.orbit_pose(i % ORBIT, ORBIT), frames[i % ORBIT])
            n1 = check()
        assert n0[0] > 0 and n1[0] + n1[1] > n0[0] + n0[1], (n0, n1)
        print("pipeline: conditional builds that built / returned early: %s before the untracked frames, %s at the end" % (n0, n1))
    finally:
        roo.set_math_mode(prev)
