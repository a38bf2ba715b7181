#!/usr/bin/env python3
"""What RaycastSdf of packed bricks costs (include/kfx_raycast_bricks.h), against the routes that existed before it, on the same
content and in the same process: 512^3 fp32 after the benchmark's S_room stream (one orbit of 30 poses at 640 x 480), every live brick
of it packed (kfx_bricks_pack, fill NaN), rendered at 640 x 480 from several poses of the orbit.  Every variant is warmed up at every
pose, the variants alternate over the rounds, each is timed with device events around a single call, and ahead of the first event the
stream is given two copies of the storage to chew on, so that the launches of the call under test are queued before the GPU gets to
them (scripts/brick_pack_timing.py's method).

  brick_plan         kfx_raycast_bricks_plan of the list: a memset and the table fill; once per list, whatever the number of views
  brick_render@k     kfx_raycast_bricks from orbit pose k
  dense_raycast@k    kfx_raycast_sdf, the plain march, on the dense volume D the list unpacks into, from the same pose
  dense_unpack       the dense route's first step: VolumeFill(D, NaN) + kfx_bricks_unpack of the list into a second 512^3 volume D

Prints one JSON object per line (ms median / min / max over the rounds), the ratio of the medians per view -- the brick render against
the plain march alone, and plan + render against the dense route unpack + march -- their best and least favourable values, and the
bytes each route allocates beside the lists and the images; --out FILE also writes the lines there."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAN = float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--views", type=int, nargs="*", default=[0, 7, 15, 22])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from kangaroo_amd import roo, scenes
    from kangaroo_amd.pipeline import FramePipeline
    assert torch.cuda.is_available(), "brick_raycast_timing needs a GPU"
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    N, w, h = args.res, 640, 480
    bmin, bmax, near, far = scenes.SCENES["room"]
    roo.set_math_mode("fast")
    pipe = FramePipeline(roo, (N, N, N), bmin, bmax, w, h, near=near, far=far, track=True)
    for i in range(args.frames):
        T_wc = scenes.orbit_pose(i, 30)
        pipe.step(T_wc, roo.Image(w, h).MemcpyFromHost(scenes.render_depth("room", w, h, T_wc, pipe.K)))
    torch.cuda.synchronize()
    vol = pipe.vol
    pad_dst = torch.empty_like(vol.storage)
    L, stream = roo._lib.load(), roo._stream(None)
    P = lambda t: C.c_void_p(t.data_ptr())

    ids, cells = roo.BrickPack(vol, NAN)
    n, nb = ids.numel(), (N // 8) ** 3
    D = roo.BoundedVolume(N, N, N, vol.boxmin, vol.boxmax)
    frame = roo._lib.KfxVolume(0, None, N, N, 0, N)
    for i in range(3):
        frame.boxmin[i], frame.boxmax[i] = float(vol.boxmin[i]), float(vol.boxmax[i])
    sbytes = roo.RaycastBricksScratchBytes(n)
    scratch = torch.empty(sbytes, dtype=torch.uint8, device="cuda")
    K = np.ascontiguousarray(pipe.K, np.float32)
    kp = K.ctypes.data_as(roo._lib.PF)
    poses = {k: np.ascontiguousarray(scenes.orbit_pose(k, 30), np.float32).reshape(-1)[:12].copy() for k in args.views}
    b_img = (roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h))
    d_img = (roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h))

    def plan():
        roo._lib.check(L.kfx_raycast_bricks_plan(C.byref(frame), P(ids), n, None, 0, P(scratch), sbytes, stream))

    def brick_render(k):
        t = poses[k].ctypes.data_as(roo._lib.PF)
        return lambda: roo._lib.check(L.kfx_raycast_bricks(b_img[0].ref(), b_img[1].ref(), b_img[2].ref(), C.byref(frame), 0, P(ids), P(cells), n, None, None, 0, 0,
                                                           P(scratch), sbytes, t, kp, near, far, pipe.trunc, 1, stream))

    def dense_raycast(k):
        t = poses[k].ctypes.data_as(roo._lib.PF)
        return lambda: roo._lib.check(L.kfx_raycast_sdf(d_img[0].ref(), d_img[1].ref(), d_img[2].ref(), D.ref(), t, kp, near, far, pipe.trunc, 1, stream))

    def dense_unpack():
        roo.VolumeFill(D, NAN)
        roo.BrickUnpack(D, ids, cells)

    dense_unpack()
    plan()
    variants = [("brick_plan", plan), ("dense_unpack", dense_unpack)]
    for k in args.views:
        variants += [("brick_render@%d" % k, brick_render(k)), ("dense_raycast@%d" % k, dense_raycast(k))]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        pad_dst.copy_(vol.storage)
        pad_dst.copy_(vol.storage)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(args.warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    # the two renderings are the same images, bit for bit (the last view's are in the buffers)
    hits = {}
    for k in args.views:
        brick_render(k)()
        dense_raycast(k)()
        torch.cuda.synchronize()
        for a, b in zip(b_img, d_img):
            assert np.array_equal(a.MemcpyToHost().view(np.int32), b.MemcpyToHost().view(np.int32)), "the brick rendering and the dense rendering differ"
        hits[k] = int((b_img[0].MemcpyToHost() > 0).sum())
    t = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            t[name].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in t.items()}
    emit({"name": "content", "res": N, "frames": args.frames, "image": [w, h], "bricks": nb, "live": n, "live_share": round(n / nb, 4),
          "packed_MiB": round(n * 4096 / 2.0 ** 20, 1), "hits": hits})
    for name, _ in variants:
        emit({"name": name, "ms": round(med[name], 4), "ms_min": round(min(t[name]), 4), "ms_max": round(max(t[name]), 4)})
    alone = {k: med["brick_render@%d" % k] / med["dense_raycast@%d" % k] for k in args.views}
    route = {k: (med["brick_plan"] + med["brick_render@%d" % k]) / (med["dense_unpack"] + med["dense_raycast@%d" % k]) for k in args.views}
    emit({"name": "ratios", "render_to_plain_march": {str(k): round(v, 3) for k, v in alone.items()},
          "render_to_plain_march_best": round(min(alone.values()), 3), "render_to_plain_march_worst": round(max(alone.values()), 3),
          "plan_and_render_to_dense_route": {str(k): round(v, 3) for k, v in route.items()},
          "plan_and_render_to_dense_route_best": round(min(route.values()), 3), "plan_and_render_to_dense_route_worst": round(max(route.values()), 3),
          "brick_route_allocates_bytes": int(sbytes), "dense_route_allocates_bytes": int(D.storage.numel())})

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for d in lines:
                fh.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
