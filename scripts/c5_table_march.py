#!/usr/bin/env python3
"""Config C5 (2048^3 half cells, one MI355X): the class-table march of a half-cell brick summary against the plain half march,
and what tracking costs the half SdfFuse.

Steps (each runs in a child process under its own time limit; results as JSON lines in --out):
  raycast K   fuse K frames of the S_room orbit (fast numerics, 640x480, tracked) into a 2048^3 half volume, then time
              kfx_raycast_sdf_h against kfx_raycast_sdf_tracked_h (device events, alternating, after warm-up), the tracked
              frame pair (fuse_tracked_h + raycast_tracked_h: the table build after every fuse included) against the plain pair,
              and report both count entry points (samples per ray, table look-ups, unique voxels U), the share of 32^3-cell
              entries of class != 0 and the unique-bytes fraction (4 B x U + table bytes + 24 B x w h) / t / 8 TB/s.
  fuse N      kfx_sdf_fuse_h against kfx_sdf_fuse_tracked_h on an N^3 half volume (after 10 frames), alternating.
The table march is forced (KFX_RAYCAST_SUMMARY=1) so that what is timed is the march, not the quarter rule's choice; the share
of skippable entries says what the rule would choose.

Usage: python scripts/c5_table_march.py --out profiles/r07_c5_tables/c5_table_march.jsonl [--steps raycast:30,raycast:300,fuse:512,fuse:2048]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_TBPS = 8.0
W, H = 640, 480
ORBIT = 30


def _setup(N):
    import numpy as np  # noqa: F401
    import torch
    from kangaroo_amd import roo, scenes
    roo.set_math_mode("fast")
    bmin, bmax, near, far = scenes.SCENES["room"]
    K = scenes.intrinsics(W, H)
    tr = scenes.trunc_dist(bmin, bmax, (N, N, N))
    frames = []   # the orbit's preprocessed images, made once: a step times kernels, not the host renderer
    for i in range(ORBIT):
        T_wc = scenes.orbit_pose(i, ORBIT)
        raw = roo.Image(W, H).MemcpyFromHost(scenes.render_depth("room", W, H, T_wc, K))
        f, v, n = roo.Image(W, H), roo.Image(W, H, "f32x4"), roo.Image(W, H, "f32x4")
        roo.BilateralFilter(f, raw, **scenes.BILATERAL)
        roo.DepthToVbo(v, f, K)
        roo.NormalsFromVbo(n, v)
        frames.append((T_wc, scenes.se3_inverse(T_wc), f, n))
    torch.cuda.synchronize()
    return roo, scenes, torch, bmin, bmax, near, far, K, tr, frames


def _alternate(torch, fns, reps, warmup=3):
    """Median device time (ms) of each callable, calls interleaved A B A B ..."""
    import numpy as np
    for _ in range(warmup):
        for f in fns:
            f()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return [dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), n=len(t)) for t in times]


def step_raycast(K_frames):
    import ctypes as C
    roo, scenes, torch, bmin, bmax, near, far, K, tr, frames = _setup(2048)
    from kangaroo_amd import _lib
    N = 2048
    vol = roo.BoundedVolume(N, N, N, bmin, bmax, kind="f16")
    summ = roo.SdfSummary(vol)
    roo.SdfReset(vol, float("nan"), summary=summ)
    fuse = lambda i, s: roo.SdfFuse(vol, frames[i % ORBIT][2], frames[i % ORBIT][3], frames[i % ORBIT][1], K, tr, scenes.MAX_W,
                                    scenes.MIN_COS_THETA, summary=s)
    t0 = time.time()
    for i in range(K_frames):
        fuse(i, summ)
    torch.cuda.synchronize()
    fuse_s = time.time() - t0
    T_wc = frames[(K_frames - 1) % ORBIT][0]
    img = [roo.Image(W, H), roo.Image(W, H, "f32x4"), roo.Image(W, H)]
    plain = lambda: roo.RaycastSdf(*img, vol, T_wc, K, near, far, tr, True)
    tracked = lambda: roo.RaycastSdf(*img, vol, T_wc, K, near, far, tr, True, summary=summ)
    rt = _alternate(torch, [plain, tracked], 20)
    # the frame pair: each tracked fuse dirties the tables, the tracked raycast rebuilds them (the volume keeps changing: the
    # comparison is of the same frames in both arms, the summary rebuilt from the volume before the tracked arm's turn)
    k = [K_frames]

    def pair_plain():
        i = k[0]; k[0] += 1
        roo.SdfFuse(vol, frames[i % ORBIT][2], frames[i % ORBIT][3], frames[i % ORBIT][1], K, tr, scenes.MAX_W, scenes.MIN_COS_THETA)
        roo.RaycastSdf(*img, vol, frames[i % ORBIT][0], K, near, far, tr, True)

    def pair_tracked():
        i = k[0]; k[0] += 1
        fuse(i, summ)
        roo.RaycastSdf(*img, vol, frames[i % ORBIT][0], K, near, far, tr, True, summary=summ)

    # (the plain arm leaves the summary stale: rebuild it outside the timed window before each tracked frame)
    times_p, times_t = [], []
    import numpy as np
    for r in range(13):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); pair_plain(); b.record(); b.synchronize()
        if r >= 3:
            times_p.append(a.elapsed_time(b))
        summ.rebuild()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); pair_tracked(); b.record(); b.synchronize()
        if r >= 3:
            times_t.append(a.elapsed_time(b))
    summ.rebuild()
    cp = roo.RaycastSdfCount(vol, W, H, T_wc, K, near, far, tr)
    ct = roo.RaycastSdfCount(vol, W, H, T_wc, K, near, far, tr, summary=summ)
    torch.cuda.synchronize()
    f = _lib.load_debug().kfx_debug_summary_export
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
    dims = (C.c_int * 12)()
    assert f(summ.handle, 0.0, 1.0, 5, None, None, dims, None) == 0
    skippable, n_coarse = dims[11], dims[10]
    out = dict(step="raycast", N=N, frames=K_frames, w=W, h=H, numerics="fast", fuse_wall_s=round(fuse_s, 3),
               raycast_plain=rt[0], raycast_tracked=rt[1], frame_pair_plain_median_ms=float(np.median(times_p)),
               frame_pair_tracked_median_ms=float(np.median(times_t)), count_plain=cp, count_tracked=ct,
               samples_per_ray_plain=cp["samples"] / max(cp["rays"], 1), samples_per_ray_tracked=ct["samples"] / max(ct["rays"], 1),
               skippable_32cube_entries=skippable, n_32cube_entries=n_coarse,
               skippable_share=(skippable / n_coarse) if skippable >= 0 else None)
    for name, c, t in (("plain", cp, rt[0]["median_ms"]), ("tracked", ct, rt[1]["median_ms"])):
        bytes_ = 4.0 * c["U"] + c.get("table_bytes", 0) + 24.0 * W * H
        out["unique_bytes_fraction_" + name] = bytes_ / (t * 1e-3) / (HBM_TBPS * 1e12)
    return out


def step_fuse(N):
    roo, scenes, torch, bmin, bmax, near, far, K, tr, frames = _setup(N)
    va, vb = roo.BoundedVolume(N, N, N, bmin, bmax, kind="f16"), roo.BoundedVolume(N, N, N, bmin, bmax, kind="f16")
    summ = roo.SdfSummary(vb)
    roo.SdfReset(va, float("nan"))
    roo.SdfReset(vb, float("nan"), summary=summ)
    k = [0]

    def plain():
        i = k[0] % ORBIT
        roo.SdfFuse(va, frames[i][2], frames[i][3], frames[i][1], K, tr, scenes.MAX_W, scenes.MIN_COS_THETA)

    def tracked():
        i = k[0] % ORBIT
        k[0] += 1
        roo.SdfFuse(vb, frames[i][2], frames[i][3], frames[i][1], K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, summary=summ)

    for _ in range(10):
        plain(); tracked()
    r = _alternate(torch, [plain, tracked], 30, warmup=0)
    return dict(step="fuse", N=N, w=W, h=H, numerics="fast", fuse_h=r[0], fuse_tracked_h=r[1],
                overhead=r[1]["median_ms"] / r[0]["median_ms"] - 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--steps", default="raycast:30,raycast:300,fuse:512,fuse:2048")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        kind, arg = a.child.split(":")
        res = step_raycast(int(arg)) if kind == "raycast" else step_fuse(int(arg))
        print("RESULT " + json.dumps(res))
        return 0
    env = dict(os.environ, KFX_RAYCAST_SUMMARY="1")
    rc = 0
    with open(a.out, "a") as fh:
        for st in a.steps.split(","):
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--out", a.out, "--child", st], env=env,
                                   capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print("%s: time limit (%d s); stopping" % (st, a.timeout))
                return 124
            lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                print("%s: exit %d\n%s" % (st, p.returncode, (p.stdout + p.stderr)[-2000:]))
                return p.returncode or 1   # (a failed GPU step ends the run)
            fh.write(lines[-1][7:] + "\n")
            fh.flush()
            print(st, lines[-1][7:])
    return rc


if __name__ == "__main__":
    sys.exit(main())
