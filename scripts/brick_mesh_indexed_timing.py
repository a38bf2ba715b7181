#!/usr/bin/env python3
"""What the indexed mesh of packed bricks costs (include/kfx_mesh_bricks_index.h), against the brick soup and against the dense indexed
route, on the same content and in the same process -- scripts/brick_mesh_timing.py's method and content: 512^3 fp32 after the
benchmark's S_room stream (one orbit of 30 poses at 640 x 480), every live brick of it packed (kfx_bricks_pack, fill NaN).  Every step
is warmed up, the steps alternate over the rounds, each is timed with device events around a single call, and ahead of the first event
the stream is given two copies of the storage to chew on, so that the launches of the call under test are queued before the GPU gets
to them.

  (a) the brick soup            brick_plan + brick_emit                          kfx_mesh_bricks_plan, kfx_mesh_bricks_emit
  (b) the brick indexed mesh    brick_plan + brick_index_plan + brick_emit_indexed   ... kfx_mesh_bricks_index_plan, kfx_mesh_bricks_emit_indexed
  (c) the dense indexed route   dense_unpack + dense_plan + dense_index_plan + dense_emit_indexed
                                VolumeFill(D, NaN) + kfx_bricks_unpack into a second 512^3 volume D, kfx_mesh_plan, kfx_mesh_index_plan,
                                kfx_mesh_emit_indexed

Prints one JSON object per line (ms median / min / max over the rounds), the output bytes of (a) and (b), the bytes (b) and (c)
allocate beside the brick lists, and the ratios of the medians (b)/(a) and (b)/(c), the least favourable one named; --out FILE also
writes the lines there."""
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
    assert torch.cuda.is_available(), "brick_mesh_indexed_timing needs a GPU"
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
    check = roo._lib.check
    P = lambda t: C.c_void_p(t.data_ptr())
    empty = lambda n, dt: torch.empty(max(int(n), 1), dtype=dt, device="cuda")

    ids, cells = roo.BrickPack(vol, NAN)
    n, nb = ids.numel(), (N // 8) ** 3
    D = roo.BoundedVolume(N, N, N, vol.boxmin, vol.boxmax)
    frame = roo._lib.KfxVolume(0, None, N, N, 0, N)
    for i in range(3):
        frame.boxmin[i], frame.boxmax[i] = float(vol.boxmin[i]), float(vol.boxmax[i])
    lists = (C.byref(frame), 0, P(ids), P(cells), n)

    # sizes from a first plan of each
    bbytes = mesh.BrickMeshScratchBytes(n)
    bscratch, btot = empty(bbytes, torch.uint8), (C.c_ulonglong * 2)()
    check(L.kfx_mesh_bricks_plan(*lists, P(bscratch), bbytes, btot, stream))
    xbytes = int(L.kfx_mesh_bricks_index_scratch_bytes(n, btot))
    xscratch, bnv = empty(xbytes, torch.uint8), C.c_ulonglong(0)
    check(L.kfx_mesh_bricks_index_plan(*lists, P(bscratch), bbytes, btot, P(xscratch), xbytes, C.byref(bnv), stream))
    dargs = (D.ref(), 0, None, 0, 0)
    dbytes = int(L.kfx_mesh_scratch_bytes(*dargs))
    dscratch, dtot = empty(dbytes, torch.uint8), (C.c_ulonglong * 2)()
    roo.VolumeFill(D, NAN)
    roo.BrickUnpack(D, ids, cells)
    check(L.kfx_mesh_plan(*dargs, P(dscratch), dbytes, dtot, stream))
    assert (btot[0], btot[1]) == (dtot[0], dtot[1]), "the brick plan and the dense plan disagree"
    dxbytes = int(L.kfx_mesh_index_scratch_bytes(*dargs, dtot))
    dxscratch, dnv = empty(dxbytes, torch.uint8), C.c_ulonglong(0)
    check(L.kfx_mesh_index_plan(*dargs, P(dscratch), dbytes, dtot, P(dxscratch), dxbytes, C.byref(dnv), stream))
    assert bnv.value == dnv.value, "the brick index and the dense index weld to different vertex counts"
    na, ntri, V = int(btot[0]), int(btot[1]), int(bnv.value)
    soup = [empty(na, torch.int64), empty(na, torch.int32), empty(9 * ntri, torch.float32), empty(9 * ntri, torch.float32)]
    bidx = [empty(3 * V, torch.float32), empty(3 * V, torch.float32), empty(3 * ntri, torch.int32)]
    didx = [torch.empty_like(t) for t in bidx]

    def dense_unpack():
        roo.VolumeFill(D, NAN)
        roo.BrickUnpack(D, ids, cells)

    variants = [
        ("brick_plan", lambda: check(L.kfx_mesh_bricks_plan(*lists, P(bscratch), bbytes, btot, stream))),
        ("brick_emit", lambda: check(L.kfx_mesh_bricks_emit(*lists, None, None, 0, P(bscratch), bbytes, btot, *[P(t) for t in soup], None, stream))),
        ("brick_index_plan", lambda: check(L.kfx_mesh_bricks_index_plan(*lists, P(bscratch), bbytes, btot, P(xscratch), xbytes, C.byref(bnv), stream))),
        ("brick_emit_indexed", lambda: check(L.kfx_mesh_bricks_emit_indexed(*lists, None, None, 0, P(bscratch), bbytes, P(xscratch), xbytes, btot, V,
                                                                           P(bidx[0]), P(bidx[1]), None, P(bidx[2]), stream))),
        ("dense_unpack", dense_unpack),
        ("dense_plan", lambda: check(L.kfx_mesh_plan(*dargs, P(dscratch), dbytes, dtot, stream))),
        ("dense_index_plan", lambda: check(L.kfx_mesh_index_plan(*dargs, P(dscratch), dbytes, dtot, P(dxscratch), dxbytes, C.byref(dnv), stream))),
        ("dense_emit_indexed", lambda: check(L.kfx_mesh_emit_indexed(*dargs, None, P(dxscratch), dxbytes, dtot, V, P(didx[0]), P(didx[1]), None,
                                                                     P(didx[2]), stream))),
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
    # the two indexed meshes are the same welded vertices in another numbering: the same count, and every id below it
    assert int(bidx[2].view(torch.int32).max()) == V - 1 == int(didx[2].max()) and int(bidx[2].min()) == 0
    med = {k: float(np.median(v)) for k, v in t.items()}
    facts = {"res": N, "frames": args.frames, "bricks": nb, "live": n, "live_share": round(n / nb, 4), "packed_MiB": round(n * 4096 / 2.0 ** 20, 1),
             "active_cubes": na, "triangles": ntri, "vertices": V, "brick_scratch_bytes": bbytes, "brick_index_scratch_bytes": xbytes,
             "dense_scratch_bytes": dbytes, "dense_index_scratch_bytes": dxbytes}
    emit(dict({"name": "content"}, **facts))
    for name, _ in variants:
        emit({"name": name, "ms": round(med[name], 4), "ms_min": round(min(t[name]), 4), "ms_max": round(max(t[name]), 4)})
    a = med["brick_plan"] + med["brick_emit"]
    b = med["brick_plan"] + med["brick_index_plan"] + med["brick_emit_indexed"]
    c = med["dense_unpack"] + med["dense_plan"] + med["dense_index_plan"] + med["dense_emit_indexed"]
    out_a, out_b = 16 * na + 72 * ntri, 24 * V + 12 * ntri
    alloc_b = bbytes + xbytes + out_b
    alloc_c = D.storage.numel() * D.storage.element_size() + dbytes + dxbytes + out_b
    ratios = {"indexed_to_soup": round(b / a, 3), "indexed_to_dense_indexed_route": round(b / c, 3)}
    emit(dict({"name": "ratios", "a_brick_soup_ms": round(a, 4), "b_brick_indexed_ms": round(b, 4), "c_dense_indexed_route_ms": round(c, 4),
               "least_favourable": max(ratios, key=ratios.get),
               "a_output_bytes": out_a, "b_output_bytes": out_b, "b_output_to_a_output": round(out_b / out_a, 3),
               "b_allocated_MiB": round(alloc_b / 2.0 ** 20, 1), "c_allocated_MiB": round(alloc_c / 2.0 ** 20, 1)}, **ratios))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for d in lines:
                fh.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
