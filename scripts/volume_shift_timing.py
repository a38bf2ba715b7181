#!/usr/bin/env python3
"""What moving the volume costs (include/kfx_shift.h), against the one yardstick that exists without it: a device-to-device copy of
the volume's storage (torch copy_).  ONE process, every variant warmed up, the variants alternating over the rounds, each timed
with device events around a single call.  Ahead of the first event the stream is given two copies of the storage to chew on, so
that the launches of the call under test are queued before the GPU gets to them: the figures are device time, not the host's
enqueue rate.

  copy              copy_ of the 512^3 fp32 volume's 1 GiB
  direct            kfx_volume_shift at 512^3 fp32 by (0, 0, 8) and (8, 0, 8): one read and one write per cell, the copy's bytes
  staged            (8, 0, 0) and (0, 8, 0) through a scratch of 16 and of 64 planes: the copy's bytes twice
  frame             kfx_frame_shift by (0, 0, 8) of a tracking frame: the shift and the summary's rebuild (one more read of the cells)
  half2048 (--big)  2048^3 half cells (32 GiB) by (0, 0, 8), against a copy of those 32 GiB

Prints one JSON object per line (ms median / min / max over the rounds, the ratio of the medians to the copy's, launches of the
plan, launches x 1.8 us as the share the launch boundaries explain); --out FILE also writes the lines there."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAN = float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--big", type=int, default=2048, help="side of the half-cell volume (0: skip)")
    ap.add_argument("--big-rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from kangaroo_amd import roo, scenes
    from kangaroo_amd.pipeline import FramePipeline
    assert torch.cuda.is_available(), "volume_shift_timing needs a GPU"
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    def timed(fn, pad):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        pad()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def measure(variants, rounds, pad):
        for _ in range(args.warmup):
            for _, fn in variants:
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name, _ in variants}
        for _ in range(rounds):
            for name, fn in variants:
                t[name].append(timed(fn, pad))
        return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in t.items()}

    def report(name, what, ms, copy_ms, vol=None, shift=None, scratch=None, extra=None):
        d = {"name": name, "what": what, "ms": round(ms[0], 4), "ms_min": round(ms[1], 4), "ms_max": round(ms[2], 4), "ratio_to_copy": round(ms[0] / copy_ms, 3)}
        if vol is not None:
            plan = roo.VolumeShiftPlan(vol, shift, scratch.numel() if scratch is not None else 0)
            d.update(shift=list(shift), launches=len(plan), boundaries_ms_at_1p8us=round(len(plan) * 1.8e-3, 4),
                     scratch_planes=(scratch.numel() // (vol.w * vol.h * vol.ELEM)) if scratch is not None else 0)
        d.update(extra or {})
        emit(d)

    # ---- 512^3 fp32: a tracking frame's volume with a few fused frames in it ----------------------------------------------------------
    N, w, h = args.res, 640, 480
    bmin, bmax, near, far = scenes.SCENES["room"]
    roo.set_math_mode("fast")
    pipe = FramePipeline(roo, (N, N, N), bmin, bmax, w, h, near=near, far=far, track=True)
    for i in range(4):
        T_wc = scenes.orbit_pose(i, 30)
        pipe.step(T_wc, roo.Image(w, h).MemcpyFromHost(scenes.render_depth("room", w, h, T_wc, pipe.K)))
    vol = pipe.vol
    dst = torch.empty_like(vol.storage)
    plane = vol.w * vol.h * vol.ELEM
    s16 = torch.empty(16 * plane, dtype=torch.uint8, device="cuda")
    s64 = torch.empty(64 * plane, dtype=torch.uint8, device="cuda")
    L, ref = roo._lib.load(), vol.ref()   # the C entry point itself: the box is left alone, every call sees the same arguments

    def shift_call(v, cell, shift, scratch):
        s3 = roo._shift3(shift)
        ptr, nb = (scratch.data_ptr(), scratch.numel()) if scratch is not None else (None, 0)
        stream = roo._stream(None)
        return lambda: roo._lib.check(L.kfx_volume_shift(v, cell, s3, NAN, ptr, nb, stream))

    def pad():
        dst.copy_(vol.storage)
        dst.copy_(vol.storage)

    fs3, fstream = roo._shift3((0, 0, 8)), roo._stream(None)
    variants = [("copy", lambda: dst.copy_(vol.storage)),
                ("direct_0_0_8", shift_call(ref, 0, (0, 0, 8), None)),
                ("direct_8_0_8", shift_call(ref, 0, (8, 0, 8), None)),
                ("staged_8_0_0_16planes", shift_call(ref, 0, (8, 0, 0), s16)),
                ("staged_8_0_0_64planes", shift_call(ref, 0, (8, 0, 0), s64)),
                ("staged_0_8_0_16planes", shift_call(ref, 0, (0, 8, 0), s16)),
                ("staged_0_8_0_64planes", shift_call(ref, 0, (0, 8, 0), s64)),
                ("frame_0_0_8_tracked", lambda: roo._lib.check(L.kfx_frame_shift(pipe.kframe.handle, fs3, None, 0, fstream))),
                ("rebuild_only", lambda: pipe.summary.rebuild())]
    t = measure(variants, args.rounds, pad)
    copy_ms = t["copy"][0]
    gib = vol.storage.numel() / 2.0 ** 30
    report("copy", "torch copy_ of the %d^3 fp32 storage (%.2f GiB)" % (N, gib), t["copy"], copy_ms,
           extra={"GBps_read_plus_write": round(2 * vol.storage.numel() / (copy_ms * 1e-3) / 1e9, 1)})
    for name, shift, scratch in (("direct_0_0_8", (0, 0, 8), None), ("direct_8_0_8", (8, 0, 8), None), ("staged_8_0_0_16planes", (8, 0, 0), s16),
                                 ("staged_8_0_0_64planes", (8, 0, 0), s64), ("staged_0_8_0_16planes", (0, 8, 0), s16), ("staged_0_8_0_64planes", (0, 8, 0), s64)):
        report(name, "kfx_volume_shift, %d^3 fp32" % N, t[name], copy_ms, vol, shift, scratch)
    report("frame_0_0_8_tracked", "kfx_frame_shift, %d^3 fp32, tracking: shift + kfx_sdf_summary_rebuild" % N, t["frame_0_0_8_tracked"], copy_ms, vol, (0, 0, 8), None)
    report("rebuild_only", "kfx_sdf_summary_rebuild alone", t["rebuild_only"], copy_ms)

    # ---- 2048^3 half cells ----------------------------------------------------------------------------------------------------------------
    if args.big:
        del pipe, dst, s16, s64
        torch.cuda.empty_cache()
        B = args.big
        big = roo.BoundedVolume(B, B, B, bmin, bmax, kind="f16")
        roo.SdfReset(big, NAN)
        bdst = torch.empty_like(big.storage)
        bref = big.ref()

        def bpad():
            bdst[:1 << 30].copy_(big.storage[:1 << 30])
            bdst[:1 << 30].copy_(big.storage[:1 << 30])

        tb = measure([("copy", lambda: bdst.copy_(big.storage)), ("half_0_0_8", shift_call(bref, 1, (0, 0, 8), None))], args.big_rounds, bpad)
        report("copy_half%d" % B, "torch copy_ of the %d^3 half-cell storage (%.1f GiB)" % (B, big.storage.numel() / 2.0 ** 30), tb["copy"], tb["copy"][0],
               extra={"GBps_read_plus_write": round(2 * big.storage.numel() / (tb["copy"][0] * 1e-3) / 1e9, 1)})
        report("half%d_0_0_8" % B, "kfx_volume_shift, %d^3 half cells" % B, tb["half_0_0_8"], tb["copy"][0], big, (0, 0, 8), None)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for d in lines:
                fh.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
