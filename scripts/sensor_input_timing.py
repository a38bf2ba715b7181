#!/usr/bin/env python3
"""What the start of the frame costs (include/kfx_sensor.h): frames per second of the benchmark's default workload -- 512^3, 640 x 480,
scene S_full, fast numerics, the pipeline's own choice of kernels -- with the depth image arriving in three ways, in ONE process,
after a warm-up of every variant, in alternating blocks:

  A  the image resident in device memory, kfx_frame_step                                  (bench.py's headline loop)
  B  what a caller without this path does: hipMemcpyAsync of the float millimetre image from page-locked memory on the launch
     stream, kfx_elementwise_scale_bias_f32, kfx_frame_step
  C  a 16-bit millimetre image through the upload ring (kfx_depth_input), submitted one frame ahead, kfx_frame_step(raw = NULL)

The page-locked buffers of B and C hold a frame already (a driver's DMA target): filling them is not part of either loop.
Prints one JSON object (medians and spreads per variant, the ratios C / A and C / B); --out FILE also writes it.

  --kernels   instead: 3 x 200 launches each of BilateralFilter<float,float> on a resident metres image and of BilateralFilterDepth
              on the u16 image, 640 x 480, size 3, fast numerics -- for a separate run under `rocprofv3 --kernel-trace --stats`
  --parse CSV the kernel trace of such a run: per kernel the median and the spread of the launch durations of each block of 200
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_ORBIT = 30


def parse_trace(path):
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r["Kernel_Name"]
            if "k_bilateral" in name:
                rows.setdefault(name.split("(")[0], []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    out = {}
    for name, v in rows.items():
        v.sort()
        d = np.array([x[1] for x in v], np.float64) / 1e3
        blocks = [d[i:i + 200] for i in range(0, len(d) - len(d) % 200, 200)] or [d]
        med = [float(np.median(b)) for b in blocks]
        out[name] = {"launches": len(d), "block_median_us": [round(m, 3) for m in med], "median_us": round(float(np.median(med)), 3),
                     "spread_us": round(max(med) - min(med), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--scene", default="full")
    ap.add_argument("--block", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=400)
    ap.add_argument("--slots", type=int, default=2)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--parse", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.parse:
        print(json.dumps(parse_trace(args.parse), indent=1))
        return

    import torch
    from kangaroo_amd import roo, scenes
    from kangaroo_amd.pipeline import FramePipeline
    N, w, h = args.res, args.width, args.height
    bmin, bmax, near, far = scenes.SCENES[args.scene]
    K = scenes.intrinsics(w, h)
    roo.set_math_mode("fast")
    depth = [scenes.render_depth(args.scene, w, h, scenes.orbit_pose(i, N_ORBIT), K) for i in range(N_ORBIT)]
    with np.errstate(invalid="ignore"):
        u16 = [np.where(np.isnan(d), 0, np.clip(np.rint(1000.0 * d), 0, 65535)).astype(np.uint16) for d in depth]
    bil = scenes.BILATERAL

    if args.kernels:
        metres, raw = roo.Image(w, h), roo.Image(w, h, "u16").MemcpyFromHost(u16[0])
        roo.ElementwiseScaleBias(metres, raw, 1e-3)
        f, m = roo.Image(w, h), roo.Image(w, h)
        for _ in range(3):
            for _ in range(200):
                roo.BilateralFilter(f, metres, bil["gs"], bil["gr"], bil["size"], bil["minval"])
            torch.cuda.synchronize()
            for _ in range(200):
                roo.BilateralFilterDepth(f, m, raw, 1e-3, 0.0, bil["gs"], bil["gr"], bil["size"], bil["minval"])
            torch.cuda.synchronize()
        return

    poses = [scenes.orbit_pose(i, N_ORBIT) for i in range(N_ORBIT)]
    inv = [scenes.se3_inverse(p) for p in poses]
    pipe = FramePipeline(roo, (N, N, N), bmin, bmax, w, h, K=K, near=near, far=far, track="auto", sensor="u16", sensor_scale=1e-3, sensor_slots=args.slots)
    kf, ring = pipe.kframe, pipe.input
    resident = [roo.Image(w, h, "f32", pitch=pipe.raw.pitch).MemcpyFromHost(u.astype(np.float32) * np.float32(1e-3)) for u in u16]
    mm_dev, metres = roo.Image(w, h, "f32", pitch=pipe.raw.pitch), roo.Image(w, h, "f32", pitch=pipe.raw.pitch)
    pinned = [mm_dev.pinned_like(u.astype(np.float32)) for u in u16]
    cursor = [0]

    def step_a():
        i = cursor[0] % N_ORBIT
        cursor[0] += 1
        pipe.step(poses[i], resident[i])

    def step_b():
        i = cursor[0] % N_ORBIT
        cursor[0] += 1
        mm_dev.MemcpyFromPinned(pinned[i])
        roo.ElementwiseScaleBias(metres, mm_dev, 1e-3)
        pipe.step(poses[i], metres)

    filled = [0]

    def submit_next():
        buf = ring.acquire()
        if filled[0] < args.slots:   # every slot's buffer is written once; afterwards it holds a frame already
            buf[...] = u16[filled[0] % N_ORBIT]
            filled[0] += 1
        ring.submit()

    def step_c():
        i = cursor[0] % N_ORBIT
        cursor[0] += 1
        submit_next()   # frame k + 1, while frame k (submitted a step ago) is consumed
        pipe.step(poses[i])

    def run(step, n):
        if step is step_c:
            submit_next()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if step is step_c:   # leave the ring empty for the other variants
            ring.filter(pipe.filtered, pipe.raw, bil["gs"], bil["gr"], bil["size"], bil["minval"])
        return n / dt

    import gc
    gc.collect()
    gc.disable()
    # warm-up: the track="auto" calibration (8 + 3 x 60 frames) decides on variant A, then every variant runs
    run(step_a, max(args.warmup, pipe.cal_first + 3 * pipe.cal_block + 8))
    assert pipe.track_decision is not None
    for s in (step_b, step_c, step_a):
        run(s, args.warmup)
    fps = {"A": [], "B": [], "C": []}
    for _ in range(args.rounds):
        for name, s in (("A", step_a), ("B", step_b), ("C", step_c)):
            fps[name].append(run(s, args.block))
    gc.enable()
    med = {k: float(np.median(v)) for k, v in fps.items()}
    spread = {k: float(max(v) - min(v)) for k, v in fps.items()}
    out = {"unit": "frames/s", "workload": "%d^3, %d x %d, scene %s, fast numerics, %s" % (N, w, h, args.scene, pipe.track_decision["chosen"]),
           "block_frames": args.block, "rounds": args.rounds, "slots": args.slots,
           "blocks": {k: [round(x, 1) for x in v] for k, v in fps.items()}, "median": {k: round(v, 1) for k, v in med.items()},
           "spread": {k: round(v, 1) for k, v in spread.items()},
           "C_over_A": round(med["C"] / med["A"], 4), "B_over_A": round(med["B"] / med["A"], 4), "C_over_B": round(med["C"] / med["B"], 4),
           "C_minus_B": round(med["C"] - med["B"], 1), "C_beats_B_by_more_than_the_spread_of_A": bool(med["C"] - med["B"] > spread["A"]),
           "C_within_2_percent_of_A": bool(med["C"] >= 0.98 * med["A"])}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
