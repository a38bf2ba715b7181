#!/usr/bin/env python3
"""What colour mode costs a slab rank's frame (include/kfx_slab_color.h), by device events, warm frames, A and B alternating in blocks,
medians with the spread of the block medians.

  (a) rank 3 of 8 over the loop-back transport (512^3, 640 x 480, S_room, fast numerics, kfx_slab_frame_step, exact raycast in 4
      row-tiles): the colour frame's parts beside the grey frame's parts from the same run.  Expectation: SdfFuse differs by about the
      24 B / 16 B traffic ratio per updated voxel, the march by one 8-corner gather per hit.
  (b) a one-rank colour slab frame (kfx_slab_frame_step) against FramePipeline(color=True), 256^3: the kernels are the same, so a gap
      is host cost -- one library call against the operators issued from Python.
  (c) the grey slab frame of (a) with this build against another build of the library (--ab OTHER/libkfx.so, e.g. the parent commit's,
      scripts/build_ab.sh), interleaved processes, and the other build against itself for the run-to-run spread.

Usage: python scripts/colour_slab_timing.py [--ab build_ab/<name>/libkfx.so] [out.json]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

BLOCK, BLOCKS, WARM = 60, 5, 300


def stats(blocks):
    import numpy as np
    med = [float(np.median(b)) for b in blocks]
    return {"median_ms": round(float(np.median(med)), 5), "block_medians_min_max_ms": [round(min(med), 5), round(max(med), 5)]}


def slab_rank(color, N=512, world=8, rank=3, w=640, h=480):
    import numpy as np  # noqa: F401
    from kangaroo_amd import roo, scenes, slab
    from kangaroo_amd.pipeline import SlabPipeline
    from slab_host_floor import LoopbackDist
    bmin, bmax, near, far = scenes.SCENES["room"]
    K = scenes.intrinsics(w, h)
    pipe = SlabPipeline(roo, LoopbackDist(rank, world), (N, N, N), bmin, bmax, w, h, halo="recompute", raycast="exact", K=K, near=near, far=far,
                        driver="c", comm=slab.Comm.loopback(rank, world), timing_slots=BLOCK + 64, unchecked=True, tiles=4, color=color)
    pipe.sframe.set_timing(31)
    poses = [scenes.orbit_pose(i, 30) for i in range(30)]
    frames = []
    for T in poses:
        im = roo.Image(w, h, "f32", pitch=pipe.raw.pitch)
        im.MemcpyFromHost(scenes.render_depth("room", w, h, T, K))
        frames.append(im)
    if color:
        pipe.rgb.MemcpyFromHost(scenes.render_rgb("room", w, h, poses[0], pipe.Kimg))
    return pipe, poses, frames


def run_block(pipe, poses, frames, n):
    import torch
    first = pipe.sframe.count
    for s in range(n):
        pipe.step(poses[s % 30], frames[s % 30])
    try:
        pipe.sframe.sync()
    except Exception:   # noqa: BLE001  (unchecked exact march of one rank of eight)
        pass
    torch.cuda.synchronize()
    return pipe.sframe.timings(first, n)


def part_a():
    pipes = {"grey": slab_rank(False), "colour": slab_rank(True)}
    for p in pipes.values():
        for _ in range(WARM // BLOCK):
            run_block(*p, BLOCK)
    cols = {"sdf_fuse_ms": 1, "raycast_ms": 2, "frame_events_ms": 4, "period_events_ms": 5}
    blocks = {k: {c: [] for c in cols} for k in pipes}
    for _ in range(BLOCKS):
        for k, p in pipes.items():
            t = run_block(*p, BLOCK)
            for c, i in cols.items():
                blocks[k][c].append(t[:-1, i] if c == "period_events_ms" else t[:, i])
    out = {k: {c: stats(v) for c, v in blocks[k].items()} for k in pipes}
    out["colour_over_grey"] = {c: round(out["colour"][c]["median_ms"] / out["grey"][c]["median_ms"], 4) for c in cols}
    return out


def part_b(N=256, w=640, h=480):
    import numpy as np
    import torch
    from kangaroo_amd import roo, scenes, slab
    from kangaroo_amd.pipeline import FramePipeline, SlabPipeline
    from slab_host_floor import LoopbackDist
    bmin, bmax, near, far = scenes.SCENES["room"]
    K = scenes.intrinsics(w, h)
    sp = SlabPipeline(roo, LoopbackDist(0, 1), (N, N, N), bmin, bmax, w, h, raycast="exact", K=K, near=near, far=far, driver="c",
                      comm=slab.Comm.threads(1)[0], tiles=1, color=True)
    sp.sframe.set_timing(0)
    mono = FramePipeline(roo, (N, N, N), bmin, bmax, w, h, K=K, near=near, far=far, color=True, track=False)
    poses = [scenes.orbit_pose(i, 30) for i in range(30)]
    depth = [scenes.render_depth("room", w, h, T, K) for T in poses]
    rgb = scenes.render_rgb("room", w, h, poses[0], sp.Kimg)
    for p in (sp, mono):
        p.rgb.MemcpyFromHost(rgb)
    frames = {id(p): [roo.Image(w, h, "f32", pitch=p.raw.pitch).MemcpyFromHost(d) for d in depth] for p in (sp, mono)}

    def block(p, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        for s in range(n):
            ev[s].record()
            p.step(poses[s % 30], frames[id(p)][s % 30])
        ev[n].record()
        torch.cuda.synchronize()
        return np.array([ev[s].elapsed_time(ev[s + 1]) for s in range(n)])
    for p in (sp, mono):
        for _ in range(WARM // BLOCK):
            block(p, BLOCK)
    got = {"slab_frame_one_rank": [], "frame_pipeline": []}
    for _ in range(BLOCKS):
        got["slab_frame_one_rank"].append(block(sp, BLOCK))
        got["frame_pipeline"].append(block(mono, BLOCK))
    out = {k: stats(v) for k, v in got.items()}
    out["note"] = "frame period by device events, start of step to start of the next; %d^3, %d x %d; same kernels: the difference is host cost" % (N, w, h)
    return out


def grey_frame_child():
    """(c): one process, one library: the grey slab frame's period and parts"""
    import ctypes
    from kangaroo_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in list(_lib.SIGNATURES):   # an older build lacks the entry points added since: the grey frame does not call them
        if not hasattr(lib, name):
            del _lib.SIGNATURES[name]
    from kangaroo_amd import roo
    roo.set_math_mode("fast")
    p = slab_rank(False)
    for _ in range(WARM // BLOCK):
        run_block(*p, BLOCK)
    per, fuse, ray = [], [], []
    for _ in range(BLOCKS):
        t = run_block(*p, BLOCK)
        per.append(t[:-1, 5]); fuse.append(t[:, 1]); ray.append(t[:, 2])
    print("CHILD " + json.dumps({"period_events_ms": stats(per), "sdf_fuse_ms": stats(fuse), "raycast_ms": stats(ray)}), flush=True)


def part_c(other):
    def child(lib):
        env = dict(os.environ)
        if lib:
            env["KFX_LIB_PATH"] = os.path.abspath(lib)
        else:
            env.pop("KFX_LIB_PATH", None)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--grey-frame-child"], capture_output=True, text=True, env=env, timeout=600)
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("CHILD ")]
        assert out.returncode == 0 and line, out.stdout[-2000:] + out.stderr[-2000:]
        return json.loads(line[0][6:])
    runs = {"other": [], "this": []}
    for _ in range(2):   # interleaved: other, this, other, this
        runs["other"].append(child(other))
        runs["this"].append(child(None))
    out = {"other_library": other, "runs": runs}
    for part in ("period_events_ms", "sdf_fuse_ms", "raycast_ms"):
        o = [r[part]["median_ms"] for r in runs["other"]]
        t = [r[part]["median_ms"] for r in runs["this"]]
        out[part] = {"other_vs_other_spread": round(abs(o[0] - o[1]) / min(o), 4), "this_over_other": round((sum(t) / 2) / (sum(o) / 2), 4)}
    return out


def main():
    args = sys.argv[1:]
    if "--grey-frame-child" in args:
        grey_frame_child()
        return
    other = None
    if "--ab" in args:
        i = args.index("--ab")
        other = args[i + 1]
        del args[i:i + 2]
    from kangaroo_amd import roo
    roo.set_math_mode("fast")
    res = {"note": "fast numerics, S_room; %d warm frames, then %d blocks of %d frames per variant, variants alternating; medians of the block medians" % (WARM, BLOCKS, BLOCK)}
    res["a_rank3_of_8_loopback_512"] = part_a()
    print("a", json.dumps(res["a_rank3_of_8_loopback_512"]), flush=True)
    res["b_one_rank_slab_frame_vs_frame_pipeline"] = part_b()
    print("b", json.dumps(res["b_one_rank_slab_frame_vs_frame_pipeline"]), flush=True)
    if other:
        res["c_grey_slab_frame_this_vs_other"] = part_c(other)
        print("c", json.dumps(res["c_grey_slab_frame_this_vs_other"]), flush=True)
    if args:
        json.dump(res, open(args[0], "w"), indent=1)


if __name__ == "__main__":
    main()
