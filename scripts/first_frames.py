#!/usr/bin/env python3
"""first_frames.py [--frames 120] [--repeat 5] [--scene full] [--res 512]: what the first frames after kfx_frame_reset cost.

While a scene is being discovered bricks change class every frame and the class tables are really rebuilt (the conditional
builds of summary.hip build): this is the stream in which the tables' change tracking has nothing to give, timed with the
frame's own device events (kfx_frame_timings) -- per repeat the sum and the median of the whole-frame times of the first
`frames` frames of the tracked pair, fast numerics.  One JSON line; compare two builds with KFX_LIB_PATH."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--scene", default="full", choices=["full", "room"])
    ap.add_argument("--res", type=int, default=512)
    a = ap.parse_args()
    import torch
    from kangaroo_amd import roo, scenes
    from kangaroo_amd.pipeline import FramePipeline
    roo.set_math_mode("fast")
    w, h, N = 640, 480, a.res
    bmin, bmax, near, far = scenes.SCENES[a.scene]
    pipe = FramePipeline(roo, (N, N, N), bmin, bmax, w, h, near=near, far=far, track=True, timing_slots=a.frames + 16)
    poses = [scenes.orbit_pose(i, 30) for i in range(30)]
    raws = []
    for T_wc in poses:
        img = roo.Image(w, h)
        img.MemcpyFromHost(scenes.render_depth(a.scene, w, h, T_wc, pipe.K))
        raws.append(img)
    pipe.set_timing(pipe.kframe.EVENTS_ALL)
    sums, meds = [], []
    for r in range(a.repeat + 1):   # (the first repeat warms the process up and is not reported)
        pipe.reset()
        first = pipe.kframe.count
        for i in range(a.frames):
            pipe.step(poses[i % 30], raws[i % 30])
        torch.cuda.synchronize()
        t = pipe.kframe.timings(first, a.frames)[:, 3].astype(np.float64)
        if r:
            sums.append(round(float(t.sum()), 4))
            meds.append(round(float(np.median(t)), 5))
    print(json.dumps(dict(scene=a.scene, res=N, frames=a.frames, lib=os.environ.get("KFX_LIB_PATH", "in-tree"),
                          whole_frames_sum_ms=sums, whole_frame_median_ms=meds)))


if __name__ == "__main__":
    main()
