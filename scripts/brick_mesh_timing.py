#!/usr/bin/env python3
"""What the mesh of packed bricks costs (include/kfx_mesh_bricks.h), against the routes that existed before it, on the same content and
in the same process: 512^3 fp32 after the benchmark's S_room stream (one orbit of 30 poses at 640 x 480), every live brick of it packed
(kfx_bricks_pack, fill NaN).  Every variant is warmed up, the variants alternate over the rounds, each is timed with device events
around a single call, and ahead of the first event the stream is given two copies of the storage to chew on, so that the launches of
the call under test are queued before the GPU gets to them (scripts/brick_pack_timing.py's method).

  brick_plan     kfx_mesh_bricks_plan of the list: neighbour table, count, scan, and the 16-byte read-back it blocks on
  brick_emit     kfx_mesh_bricks_emit: its own 16-byte read-back, compact, emit
  dense_unpack   the dense route's first step: VolumeFill(D, NaN) + kfx_bricks_unpack of the list into a second 512^3 volume D
  dense_plan     kfx_mesh_plan of D (the same cells as the volume: the dense mesh alone costs dense_plan + dense_emit)
  dense_emit     kfx_mesh_emit of D

Prints one JSON object per line (ms median / min / max over the rounds) and the two ratios of the medians: the brick mesh against the
dense route (unpack + plan + emit) and against the dense mesh alone (plan + emit); --out FILE also writes the lines there."""
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from kangaroo_amd import mesh, roo, scenes
    from kangaroo_amd.pipeline import FramePipeline
    assert torch.cuda.is_available(), "brick_mesh_timing needs a GPU"
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
    empty = lambda n, dt: torch.empty(max(int(n), 1), dtype=dt, device="cuda")

    ids, cells = roo.BrickPack(vol, NAN)
    n, nb = ids.numel(), (N // 8) ** 3
    D = roo.BoundedVolume(N, N, N, vol.boxmin, vol.boxmax)
    frame = roo._lib.KfxVolume(0, None, N, N, 0, N)
    for i in range(3):
        frame.boxmin[i], frame.boxmax[i] = float(vol.boxmin[i]), float(vol.boxmax[i])

    # sizes from a first plan of each
    bbytes = mesh.BrickMeshScratchBytes(n)
    bscratch, btot = empty(bbytes, torch.uint8), (C.c_ulonglong * 2)()
    roo._lib.check(L.kfx_mesh_bricks_plan(C.byref(frame), 0, P(ids), P(cells), n, P(bscratch), bbytes, btot, stream))
    dargs = (D.ref(), 0, None, 0, 0)
    dbytes = L.kfx_mesh_scratch_bytes(*dargs)
    dscratch, dtot = empty(dbytes, torch.uint8), (C.c_ulonglong * 2)()
    roo.VolumeFill(D, NAN)
    roo.BrickUnpack(D, ids, cells)
    roo._lib.check(L.kfx_mesh_plan(*dargs, P(dscratch), dbytes, dtot, stream))
    assert (btot[0], btot[1]) == (dtot[0], dtot[1]), "the brick plan and the dense plan disagree"
    na, ntri = int(btot[0]), int(btot[1])
    out = [empty(na, torch.int64), empty(na, torch.int32), empty(9 * ntri, torch.float32), empty(9 * ntri, torch.float32)]
    dout = [torch.empty_like(t) for t in out]

    def dense_unpack():
        roo.VolumeFill(D, NAN)
        roo.BrickUnpack(D, ids, cells)

    variants = [
        ("brick_plan", lambda: roo._lib.check(L.kfx_mesh_bricks_plan(C.byref(frame), 0, P(ids), P(cells), n, P(bscratch), bbytes, btot, stream))),
        ("brick_emit", lambda: roo._lib.check(L.kfx_mesh_bricks_emit(C.byref(frame), 0, P(ids), P(cells), n, None, None, 0, P(bscratch), bbytes, btot,
                                                                     *[P(t) for t in out], None, stream))),
        ("dense_unpack", dense_unpack),
        ("dense_plan", lambda: roo._lib.check(L.kfx_mesh_plan(*dargs, P(dscratch), dbytes, dtot, stream))),
        ("dense_emit", lambda: roo._lib.check(L.kfx_mesh_emit(*dargs, None, P(dscratch), dbytes, dtot, *[P(t) for t in dout], None, stream))),
    ]

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
    t = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            t[name].append(timed(fn))
    # the two meshes are the same triangles (the order differs): the same multiset of cube indices, the same number of vertices
    assert torch.equal(torch.sort(out[0][:na]).values, dout[0][:na]), "the brick mesh and the dense mesh list different cubes"
    med = {k: float(np.median(v)) for k, v in t.items()}
    facts = {"res": N, "frames": args.frames, "bricks": nb, "live": n, "live_share": round(n / nb, 4), "packed_MiB": round(n * 4096 / 2.0 ** 20, 1),
             "active_cubes": na, "triangles": ntri, "brick_scratch_bytes": bbytes, "dense_scratch_bytes": int(dbytes)}
    emit(dict({"name": "content"}, **facts))
    for name, _ in variants:
        emit({"name": name, "ms": round(med[name], 4), "ms_min": round(min(t[name]), 4), "ms_max": round(max(t[name]), 4)})
    brick = med["brick_plan"] + med["brick_emit"]
    alone = med["dense_plan"] + med["dense_emit"]
    route = alone + med["dense_unpack"]
    emit({"name": "ratios", "brick_ms": round(brick, 4), "dense_route_ms": round(route, 4), "dense_alone_ms": round(alone, 4),
          "brick_to_dense_route": round(brick / route, 3), "brick_to_dense_alone": round(brick / alone, 3),
          "brick_memory_MiB": round((n * 4100 + bbytes + 16 * na + 72 * ntri) / 2.0 ** 20, 1),
          "dense_route_memory_MiB": round((n * 4100 + D.storage.numel() + dbytes + 16 * na + 72 * ntri) / 2.0 ** 20, 1)})

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for d in lines:
                fh.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
