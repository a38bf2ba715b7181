#!/usr/bin/env python3
"""What a shift that spills and a shift that restores cost with the store on the host (follow=dict(spill=True): bricks.BrickStore, the
baseline) and with the store on the device (spill="device": bricks.DeviceBrickStore over include/kfx_brick_pool.h), against the
yardstick scripts/brick_pack_timing.py uses: a device-to-device copy of the volume's storage, taken in the same process.  512^3 fp32
after the benchmark's S_room stream (one orbit of 30 poses at 640 x 480), tracking; two pipelines that hold the same volume, one per
store; the variants alternate over the rounds, and the first round of every variant warms up and is dropped.

  copy                  copy_ of the volume's 1 GiB
  shift_out, _back      shift_volume((0, 0, 8)), which spills 8 planes, and shift_volume((0, 0, -8)), which restores them: host clock
                        around the call and a synchronise
  gap_out, _back        the same calls in the middle of a stream of 2 x --frames frames (step() of one pose, no synchronise in
                        between): host clock around the whole stream and a synchronise, minus the same stream without the shift --
                        what the shift adds to the stream
  world_view            world_view() while the volume is away: the live bricks packed, the store's bricks beside them, the plan of the
                        brick ray-cast -- host clock and a synchronise

Prints one JSON object per line (ms median / min / max over the rounds, host over device, the ratio of the medians to the copy's);
--out FILE also writes the lines there."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--stream-frames", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from kangaroo_amd import roo, scenes
    from kangaroo_amd.pipeline import FramePipeline
    assert torch.cuda.is_available(), "brick_pool_timing needs a GPU"
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    N, w, h = args.res, 640, 480
    bmin, bmax, near, far = scenes.SCENES["room"]
    roo.set_math_mode("fast")
    make = lambda spill: FramePipeline(roo, (N, N, N), bmin, bmax, w, h, near=near, far=far, track=True, follow=dict(quantum=8, slack=1e9, spill=spill))
    pipes = {"host": make(True), "device": make("device")}
    raw = None
    for i in range(args.frames):
        T_wc = scenes.orbit_pose(i, 30)
        raw = roo.Image(w, h).MemcpyFromHost(scenes.render_depth("room", w, h, T_wc, pipes["host"].K))
        for pipe in pipes.values():
            pipe.step(T_wc, raw)
    torch.cuda.synchronize()
    assert all(pipe.shifts == [] for pipe in pipes.values())
    assert torch.equal(pipes["host"].vol.storage, pipes["device"].vol.storage)
    before = pipes["host"].vol.storage.clone()
    dst = torch.empty_like(before)
    T_last = scenes.orbit_pose(args.frames - 1, 30)

    def clocked(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def stream(pipe, shift):
        def run():
            for _ in range(args.stream_frames):
                pipe.step(T_last, raw)
            if shift is not None:
                pipe.shift_volume(shift)
            for _ in range(args.stream_frames):
                pipe.step(T_last, raw)
        return clocked(run)

    out, back = (0, 0, 8), (0, 0, -8)
    t = {}
    add = lambda name, ms: t.setdefault(name, []).append(ms)
    facts = {}
    # ---- synchronised calls, and world_view() while away; the volumes are what they were after every round ----------------------------
    for _ in range(args.rounds + 1):
        add("copy", clocked(lambda: dst.copy_(before)))
        for name, pipe in pipes.items():
            add("shift_out/" + name, clocked(lambda: pipe.shift_volume(out)))
            facts[name] = {"bricks_stored": len(pipe.store)}
            add("world_view/" + name, clocked(lambda: pipe.world_view()))
            r0 = pipe.restored
            add("shift_back/" + name, clocked(lambda: pipe.shift_volume(back)))
            facts[name]["bricks_restored"] = pipe.restored - r0
    for name, pipe in pipes.items():
        assert torch.equal(before, pipe.vol.storage) and len(pipe.store) == 0, "%s: there and back did not restore the volume" % name
    assert pipes["device"].store.dropped == 0 and facts["host"] == facts["device"], facts
    # ---- the same calls inside a stream of frames (the frames fuse: the volumes move on, both alike) -----------------------------------
    for _ in range(args.rounds + 1):
        for name, pipe in pipes.items():
            base = stream(pipe, None)
            add("stream/" + name, base)
            add("gap_out/" + name, stream(pipe, out) - base)
            add("gap_back/" + name, stream(pipe, back) - base)
    assert torch.equal(pipes["host"].vol.storage, pipes["device"].vol.storage), "the two pipelines no longer hold the same volume"

    med = {k: (float(np.median(v[1:])), float(min(v[1:])), float(max(v[1:]))) for k, v in t.items()}
    copy_ms = med["copy"][0]
    emit({"name": "copy", "what": "torch copy_ of the %d^3 fp32 storage (%.2f GiB), host clock and a synchronise" % (N, before.numel() / 2.0 ** 30),
          "ms": round(copy_ms, 4), "ms_min": round(med["copy"][1], 4), "ms_max": round(med["copy"][2], 4), "rounds": args.rounds})
    what = {"shift_out": "shift_volume((0, 0, 8)), spilling, then a synchronise", "shift_back": "shift_volume((0, 0, -8)), restoring, then a synchronise",
            "gap_out": "what the spilling shift adds to a stream of 2 x %d frames" % args.stream_frames,
            "gap_back": "what the restoring shift adds to a stream of 2 x %d frames" % args.stream_frames,
            "world_view": "world_view() while away, then a synchronise", "stream": "2 x %d frames without a shift" % args.stream_frames}
    for key in ("shift_out", "shift_back", "gap_out", "gap_back", "world_view", "stream"):
        hm, dm = med[key + "/host"], med[key + "/device"]
        emit(dict({"name": key, "what": "%s; %d^3 fp32 after %d frames of S_room, tracking; host clock" % (what[key], N, args.frames),
                   "host_ms": round(hm[0], 4), "host_ms_min": round(hm[1], 4), "host_ms_max": round(hm[2], 4),
                   "device_ms": round(dm[0], 4), "device_ms_min": round(dm[1], 4), "device_ms_max": round(dm[2], 4),
                   "host_over_device": round(hm[0] / dm[0], 2) if dm[0] > 0 else None,
                   "device_ratio_to_copy": round(dm[0] / copy_ms, 3), "host_ratio_to_copy": round(hm[0] / copy_ms, 3)}, **facts["device"]))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for d in lines:
                fh.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
