#!/usr/bin/env python3
"""What a sparse snapshot costs (include/kfx_bricks.h), against the yardstick scripts/volume_shift_timing.py uses: a device-to-device
copy of the volume's storage (torch copy_), taken in the same process.  512^3 fp32 after the benchmark's S_room stream (one orbit
of 30 poses at 640 x 480).  Every variant is warmed up, the variants alternate over the rounds, each is timed with device events
around a single call, and ahead of the first event the stream is given two copies of the storage to chew on, so that the launches
of the call under test are queued before the GPU gets to them.

  copy          copy_ of the volume's 1 GiB (reads 1 GiB and writes 1 GiB)
  plan          kfx_bricks_plan of the whole volume: one read of the cells, the scan, and the 8-byte read-back it blocks on
  pack          kfx_bricks_pack: its own 8-byte read-back, the ids, and the live bricks' cells read and written
  unpack        kfx_bricks_unpack of those lists into the volume
  slab_z, _x    the same three for a slab of 8 planes: the z-planes shift_volume((0, 0, 8)) discards (contiguous), and 8 cells of
                every row (64 bytes per row: the shape an x-shift discards, taken at mid-volume where the scene has surfaces)
  shift_spill   FramePipeline(follow=dict(spill=True)).shift_volume((0, 0, 8)), then (0, 0, -8), which restores: host clock around
                the call and a synchronise -- the copies to and from the host and the Python store are part of it

Prints one JSON object per line (ms median / min / max over the rounds, the ratio of the medians to the copy's); --out FILE also
writes the lines there."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAN = float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shift-rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from kangaroo_amd import roo, scenes
    from kangaroo_amd.pipeline import FramePipeline
    assert torch.cuda.is_available(), "brick_pack_timing needs a GPU"
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    N, w, h = args.res, 640, 480
    bmin, bmax, near, far = scenes.SCENES["room"]
    roo.set_math_mode("fast")
    pipe = FramePipeline(roo, (N, N, N), bmin, bmax, w, h, near=near, far=far, track=True, follow=dict(quantum=8, slack=1e9, spill=True))
    for i in range(args.frames):
        T_wc = scenes.orbit_pose(i, 30)
        pipe.step(T_wc, roo.Image(w, h).MemcpyFromHost(scenes.render_depth("room", w, h, T_wc, pipe.K)))
    torch.cuda.synchronize()
    assert pipe.shifts == []
    vol = pipe.vol
    dst = torch.empty_like(vol.storage)
    L, stream = roo._lib.load(), roo._stream(None)

    def pad():
        dst.copy_(vol.storage)
        dst.copy_(vol.storage)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        pad()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def brick_calls(view, tag):
        """the three calls on one view, with buffers sized by a first plan; (variants, facts)"""
        ref, kind = view.ref(), roo.CELL_KIND[view.kind]
        need = roo.BrickScratchBytes(view)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        n = C.c_ulonglong(0)
        roo._lib.check(L.kfx_bricks_plan(ref, kind, NAN, scratch.data_ptr(), need, C.byref(n), stream))
        live, bb = n.value, roo.brick_bytes(view)
        ids = torch.empty(max(live, 1), dtype=torch.int32, device="cuda")
        cells = torch.empty(max(live, 1) * bb, dtype=torch.uint8, device="cuda")
        nb = ((view.w + 7) // 8) * ((view.h + 7) // 8) * ((view.d + 7) // 8)
        facts = {"bricks": nb, "live": live, "live_share": round(live / nb, 4), "view_MiB": round(view.w * view.h * view.d * view.ELEM / 2.0 ** 20, 2),
                 "packed_MiB": round(live * bb / 2.0 ** 20, 2), "scratch_bytes": need}
        plan = lambda: roo._lib.check(L.kfx_bricks_plan(ref, kind, NAN, scratch.data_ptr(), need, C.byref(n), stream))
        pack = lambda: roo._lib.check(L.kfx_bricks_pack(ref, kind, NAN, scratch.data_ptr(), need, live, ids.data_ptr(), cells.data_ptr(), stream))
        unpack = lambda: roo._lib.check(L.kfx_bricks_unpack(ref, kind, ids.data_ptr(), cells.data_ptr(), live, stream))
        return [(tag + "plan", plan), (tag + "pack", pack), (tag + "unpack", unpack)], facts

    whole, whole_facts = brick_calls(vol, "")
    slab_z, z_facts = brick_calls(vol.SubVolume((0, 0, 0), (N, N, 8)), "slab_z_")   # what shift_volume((0, 0, 8)) below discards
    slab_x, x_facts = brick_calls(vol.SubVolume((N // 2, 0, 0), (8, N, N)), "slab_x_")
    variants = [("copy", lambda: dst.copy_(vol.storage))] + whole + slab_z + slab_x
    before = vol.storage.clone()
    for _ in range(args.warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            t[name].append(timed(fn))
    assert torch.equal(before, vol.storage), "packing and unpacking its own bricks changed the volume"
    med = {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in t.items()}
    copy_ms = med["copy"][0]
    emit({"name": "copy", "what": "torch copy_ of the %d^3 fp32 storage (%.2f GiB)" % (N, vol.storage.numel() / 2.0 ** 30), "ms": round(copy_ms, 4),
          "ms_min": round(med["copy"][1], 4), "ms_max": round(med["copy"][2], 4), "ratio_to_copy": 1.0,
          "GBps_read_plus_write": round(2 * vol.storage.numel() / (copy_ms * 1e-3) / 1e9, 1)})
    for group, facts, what in ((whole, whole_facts, "the whole volume"), (slab_z, z_facts, "the first 8 z-planes"),
                               (slab_x, x_facts, "8 cells of every row (the shape an x-shift discards, taken at mid-volume where the scene has surfaces)")):
        for name, _ in group:
            ms = med[name]
            emit(dict({"name": name, "what": "kfx_bricks_%s, %s of %d^3 fp32 after %d frames of S_room" % (name.split("_")[-1], what, N, args.frames),
                       "ms": round(ms[0], 4), "ms_min": round(ms[1], 4), "ms_max": round(ms[2], 4), "ratio_to_copy": round(ms[0] / copy_ms, 3)}, **facts))

    # ---- a shift that spills, and the one that restores: the pipeline's own call, host and store included ------------------------------
    def clocked(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out_ms, back_ms, stored, restored = [], [], 0, 0
    for _ in range(args.shift_rounds + 1):   # (the first round warms up)
        out_ms.append(clocked(lambda: pipe.shift_volume((0, 0, 8))))
        stored = len(pipe.store)
        r0 = pipe.restored
        back_ms.append(clocked(lambda: pipe.shift_volume((0, 0, -8))))
        restored = pipe.restored - r0
    assert torch.equal(before, vol.storage) and len(pipe.store) == 0, "there and back did not restore the volume"
    for name, v, extra in (("shift_spill_out", out_ms[1:], {"bricks_stored": stored, "store_MiB": round(stored * 4096 / 2.0 ** 20, 2)}),
                           ("shift_spill_back", back_ms[1:], {"bricks_restored": restored})):
        emit(dict({"name": name, "what": "FramePipeline.shift_volume with spill, %d^3 fp32, tracking; host clock, host copies and store included" % N,
                   "ms": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                   "ratio_to_copy": round(float(np.median(v)) / copy_ms, 3)}, **extra))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for d in lines:
                fh.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
