#!/usr/bin/env python3
"""Colour mode timings (include/kfx_color.h) at 512^3, 640x480, S_full and S_room, fast and exact numerics.  Device events around
each call, A and B alternating frame by frame in one process; medians over the frames after the warm-up.
  fuse        kfx_sdf_fuse_color_tracked against kfx_sdf_fuse_color (twin volumes, the same frames)
  pass        kfx_raycast_color_hits alone: one 640x480 image, and pyramid levels 0, 2, 3 in one launch
  raycast     RaycastSdf + pass against kfx_raycast_sdf_color (both on the plain march), and the table march + pass
  levels      RaycastSdfColorLevels (plain / tables) against three per-level kfx_raycast_sdf_color calls
  frame       FramePipeline(color=True): tracked against plain, whole frames (two pipelines, alternating)
  loop        TrackingPipeline(color=True, device_icp=True), tracked + one rendering launch, against the same loop driven with
              the operators there were before: SdfFuseColor, summary.invalidate(), three per-level RaycastSdfColor (host clock
              around step(): the pose read-back synchronises every frame)
Usage: python scripts/colour_timing.py --out profiles/colour_mode/colour_timing.jsonl [--res 512] [--frames 30] [--warm 8]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H, ORBIT = 640, 480, 30
T_CD = np.array([[1, 0, 0, 0.025], [0, 1, 0, -0.003], [0, 0, 1, 0.002]], np.float32)


def color_pose(T_cw):
    return (np.vstack([T_CD, [0, 0, 0, 1]]) @ np.vstack([T_cw, [0, 0, 0, 1]]))[:3].astype(np.float32)


def timed(fn):
    """milliseconds between device events around fn()"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def med(v):
    return round(float(np.median(v)), 5)


def stream_inputs(scene, frames):
    from kangaroo_amd import roo, scenes
    K = scenes.intrinsics(W, H)
    out = []
    for i in range(frames):
        T_wc = scenes.orbit_pose(i, ORBIT)
        T_cw = scenes.se3_inverse(T_wc)
        T_iw = color_pose(T_cw)
        raw = roo.Image(W, H).MemcpyFromHost(scenes.render_depth(scene, W, H, T_wc, K))
        rgb = roo.Image(W, H, "u8x3")
        rgb.MemcpyFromHost(scenes.render_rgb(scene, W, H, scenes.se3_inverse(T_iw), K))
        out.append(dict(T_wc=T_wc, T_cw=T_cw, T_iw=T_iw, raw=raw, rgb=rgb))
    return K, out


def operators(scene, math, N, frames, warm, K, inputs):
    import torch
    from kangaroo_amd import roo, scenes
    bmin, bmax, near, far = scenes.SCENES[scene]
    tr = scenes.trunc_dist(bmin, bmax, (N, N, N))
    roo.set_math_mode(math)
    va, vb = roo.BoundedVolume(N, N, N, bmin, bmax), roo.BoundedVolume(N, N, N, bmin, bmax)
    ca, cb = roo.BoundedVolume(N, N, N, bmin, bmax, kind="c32"), roo.BoundedVolume(N, N, N, bmin, bmax, kind="c32")
    summ = roo.SdfSummary(vb)
    roo.SdfReset(va, float("nan"))
    roo.SdfReset(vb, float("nan"), summary=summ)
    roo.ColorReset(ca)
    roo.ColorReset(cb)
    f, v, n = roo.Image(W, H), roo.Image(W, H, "f32x4"), roo.Image(W, H, "f32x4")
    levels = [0, 2, 3]
    Ks = [scenes.intrinsics_level(K, l) for l in levels]
    img = lambda l: [roo.Image(W >> l, H >> l), roo.Image(W >> l, H >> l, "f32x4"), roo.Image(W >> l, H >> l), roo.Image(W >> l, H >> l, "f32x4")]
    one, per = [img(l) for l in levels], [img(l) for l in levels]
    d0 = one[0]
    t = {k: [] for k in ("fuse_plain", "fuse_tracked", "pass_one", "pass_levels", "ray_color_kernel", "ray_plain_plus_pass", "ray_tables_plus_pass",
                         "levels_per_level_color", "levels_plain_plus_pass", "levels_tables_plus_pass")}
    for i, fr in enumerate(inputs[:frames]):
        roo.BilateralFilter(f, fr["raw"], **scenes.BILATERAL)
        roo.DepthToVbo(v, f, K)
        roo.NormalsFromVbo(n, v)
        args = (f, n, fr["T_cw"], K, fr["rgb"], fr["T_iw"], K, tr, scenes.MAX_W, scenes.MIN_COS_THETA)
        order = (("fuse_plain", lambda: roo.SdfFuseColor(va, ca, *args)), ("fuse_tracked", lambda: roo.SdfFuseColor(vb, cb, *args, summary=summ)))
        for name, fn in (order if i % 2 == 0 else order[::-1]):
            ms = timed(fn)
            if i >= warm:
                t[name].append(ms)
        T_wc = fr["T_wc"]
        ray = (T_wc, K, near, far, tr, True)
        calls = [("ray_color_kernel", lambda: roo.RaycastSdfColor(*d0[:3], vb, cb, *ray)),
                 ("ray_plain_plus_pass", lambda: (roo.RaycastSdf(*d0[:3], vb, *ray), roo.RaycastColorHits([(d0[0], d0[2])], cb, T_wc, [K]))),
                 ("ray_tables_plus_pass", lambda: roo.RaycastSdfColor(*d0[:3], vb, cb, *ray, summary=summ)),
                 ("pass_one", lambda: roo.RaycastColorHits([(d0[0], d0[2])], cb, T_wc, [K])),
                 ("levels_per_level_color", lambda: [roo.RaycastSdfColor(*o[:3], vb, cb, T_wc, Kl, near, far, tr, True) for o, Kl in zip(per, Ks)]),
                 ("levels_plain_plus_pass", lambda: roo.RaycastSdfColorLevels([tuple(o) for o in one], vb, cb, T_wc, Ks, near, far, tr, True)),
                 ("levels_tables_plus_pass", lambda: roo.RaycastSdfColorLevels([tuple(o) for o in one], vb, cb, T_wc, Ks, near, far, tr, True, summary=summ)),
                 ("pass_levels", lambda: roo.RaycastColorHits([(o[0], o[2]) for o in one], cb, T_wc, Ks))]
        if i % 2:
            calls = calls[::-1]
        for name, fn in calls:
            ms = timed(fn)
            if i >= warm:
                t[name].append(ms)
    hits = float(np.isfinite(d0[0].MemcpyToHost()).mean())
    same = bool(torch.equal(va.tensor().view(torch.int32), vb.tensor().view(torch.int32)) and torch.equal(ca.tensor().view(torch.int32), cb.tensor().view(torch.int32)))
    rec = {k + "_ms": med(x) for k, x in t.items()}
    rec.update(tracked_fuse_cost_percent=round(100.0 * (rec["fuse_tracked_ms"] / rec["fuse_plain_ms"] - 1.0), 2), hit_fraction=round(hits, 3),
               tracked_volumes_bit_equal=same)
    del va, vb, ca, cb, summ
    torch.cuda.empty_cache()
    return rec


def frame_pair(scene, math, N, frames, warm, inputs):
    import torch
    from kangaroo_amd import roo, scenes
    from kangaroo_amd.pipeline import FramePipeline
    bmin, bmax, near, far = scenes.SCENES[scene]
    roo.set_math_mode(math)
    pipes = {k: FramePipeline(roo, (N, N, N), bmin, bmax, W, H, near=near, far=far, track=(k == "tracked"), color=True, T_cd=T_CD) for k in ("tracked", "plain")}
    t = {k: [] for k in pipes}
    for i, fr in enumerate(inputs[:frames]):
        for k in (("tracked", "plain") if i % 2 == 0 else ("plain", "tracked")):
            ms = timed(lambda: pipes[k].step(fr["T_wc"], raw_image=fr["raw"], rgb_image=fr["rgb"]))
            if i >= warm:
                t[k].append(ms)
    rec = {"frame_%s_ms" % k: med(v) for k, v in t.items()}
    del pipes
    torch.cuda.empty_cache()
    return rec


def tracking_loop(scene, math, N, frames, warm, inputs):
    import torch
    from kangaroo_amd import roo, scenes
    from kangaroo_amd.pipeline import TrackingPipeline
    bmin, bmax, near, far = scenes.SCENES[scene]
    roo.set_math_mode(math)

    class Before(TrackingPipeline):
        """the colour loop with the operators there were before: the untracked writer followed by the invalidation its
        contract asks for, and one plain colour march per level"""
        def _fuse_color(self, maps_d, maps_n, T_cw):
            super()._fuse_color(maps_d, maps_n, T_cw)
            self.stale.invalidate()

    now = TrackingPipeline(roo, (N, N, N), bmin, bmax, W, H, near=near, far=far, track=True, one_raycast=True, device_icp=True, color=True, T_cd=T_CD)
    old = Before(roo, (N, N, N), bmin, bmax, W, H, near=near, far=far, track=False, one_raycast=False, device_icp=True, color=True, T_cd=T_CD)
    old.stale = roo.SdfSummary(old.vol)
    t = {"loop_tracked": [], "loop_before": []}
    good = True
    for i, fr in enumerate(inputs[:frames]):
        for k, p in ((("loop_tracked", now), ("loop_before", old)) if i % 2 == 0 else (("loop_before", old), ("loop_tracked", now))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p.step(T_wl_init=fr["T_wc"] if i == 0 else None, raw_image=fr["raw"], rgb_image=fr["rgb"])
            torch.cuda.synchronize()
            if i >= warm:
                t[k].append(1e3 * (time.perf_counter() - t0))
            good = good and p.tracking_good
    rec = {k + "_ms": med(v) for k, v in t.items()}
    rec["loop_tracking_good"] = bool(good)
    del now, old
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colour_mode", "colour_timing.jsonl"))
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warm", type=int, default=8)
    ap.add_argument("--scenes", default="full,room")
    ap.add_argument("--math", default="fast,exact")
    a = ap.parse_args()
    import torch
    from kangaroo_amd import _lib
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for scene in a.scenes.split(","):
        K, inputs = stream_inputs(scene, a.frames)
        for math in a.math.split(","):
            rec = dict(scene=scene, math=math, dims=[a.res] * 3, image=[W, H], frames=a.frames, warm=a.warm,
                       raycast_summary_env=os.environ.get("KFX_RAYCAST_SUMMARY", ""),
                       source_id=_lib.load().kfx_kernel_source_id(b"fuse").decode())
            rec.update(operators(scene, math, a.res, a.frames, a.warm, K, inputs))
            rec.update(frame_pair(scene, math, a.res, a.frames, a.warm, inputs))
            rec.update(tracking_loop(scene, math, a.res, a.frames, a.warm, inputs))
            print(json.dumps(rec), flush=True)
            with open(a.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
