#!/usr/bin/env python3
"""Derivation of KFX_SUMMARY_HALF_BAND (include/kfx_summary_h.h): how far observed free space of a half-cell volume drifts
from vref = (half) trunc_dist under the reference's half running average (Sdf.h:52-58: every intermediate rounded to half).

CPU only: the oracle's half fuse (kfo_sdf_fuse_h, the GPU's bit-exact counterpart) and, next to it, its fp32 fuse of the
same frames.  A cell counts as free space where the fp32 volume holds trunc_dist within the fp32 tables' own 1e-5 -- every
observation it took was +trunc -- and its half value is then compared with vref.  Reported per checkpoint: the largest
relative deviation |v - vref| / vref over those cells (and in half ulps of vref), the largest seen so far (excursions), and
how many free cells there are.  The band the library uses must cover the largest deviation with margin.

Usage: python scripts/half_free_band.py [--frames 600] [--N 64] [--scenes room,full] [--out path.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import oracle  # noqa: E402  (a measurement script: the CPU oracle is the reference arithmetic)
from kangaroo_amd import scenes  # noqa: E402


def library_band():
    """KFX_SUMMARY_HALF_BAND as the library header defines it."""
    for line in open(os.path.join(ROOT, "include", "kfx_summary_h.h")):
        if line.startswith("#define KFX_SUMMARY_HALF_BAND"):
            return float(line.split()[2].rstrip("f"))
    raise RuntimeError("KFX_SUMMARY_HALF_BAND not found")


def _preprocess(depth_np, K):
    h, w = depth_np.shape
    d = oracle.Image.from_numpy(depth_np)
    f, vbo, nrm = oracle.Image(w, h), oracle.Image(w, h, channels=4), oracle.Image(w, h, channels=4)
    b = scenes.BILATERAL
    oracle.bilateral(f, d, b["gs"], b["gr"], b["size"], b["minval"])
    oracle.depth_to_vbo(vbo, f, K)
    oracle.normals_from_vbo(nrm, vbo)
    return f, nrm


def simulate(scene, N, frames, w=160, h=120, orbit=120, every=None, nthreads=None):
    """Fuse `frames` frames of the orbit (orbit_pose(i, orbit)) into an fp32 and a half oracle volume; returns the list of
    checkpoints {frame, free, max_rel, max_ulps} (every `every` frames and at the end) and the overall maximum."""
    bmin, bmax, near, far = scenes.SCENES[scene]
    K = scenes.intrinsics(w, h)
    tr = scenes.trunc_dist(bmin, bmax, (N, N, N))
    vref = float(np.float16(tr))
    ulp = float(np.spacing(np.float16(vref)))
    nthreads = nthreads or min(16, oracle.max_threads())
    v32, v16 = oracle.Volume(N, N, N, bmin, bmax), oracle.VolumeH(N, N, N, bmin, bmax)
    oracle.sdf_reset(v32, float("nan"))
    oracle.sdf_reset(v16, float("nan"))
    every = every or max(1, frames // 10)
    rows, worst = [], 0.0
    for i in range(frames):
        T_wc = scenes.orbit_pose(i, orbit)
        f, nrm = _preprocess(scenes.render_depth(scene, w, h, T_wc, K), K)
        T_cw = scenes.se3_inverse(T_wc)
        oracle.sdf_fuse(v32, f, nrm, T_cw, K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, nthreads=nthreads)
        oracle.sdf_fuse(v16, f, nrm, T_cw, K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, nthreads=nthreads)
        a = np.asarray(v32.data[..., 0], np.float32)
        free = np.abs(a - np.float32(tr)) <= np.float32(1e-5) * np.float32(tr)
        hv = np.asarray(v16.data[..., 0], np.float32)[free]
        dev = float(np.abs(hv - vref).max()) if hv.size else 0.0
        worst = max(worst, dev / vref)
        if (i + 1) % every == 0 or i + 1 == frames:
            rows.append(dict(frame=i + 1, free=int(free.sum()), max_rel=dev / vref, max_ulps=dev / ulp, worst_rel_so_far=worst))
    return dict(scene=scene, N=N, frames=frames, w=w, h=h, trunc=tr, vref=vref, ulp=ulp, checkpoints=rows, max_rel=worst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--scenes", default="room,full")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    band = library_band()
    res = [simulate(s, a.N, a.frames) for s in a.scenes.split(",")]
    for r in res:
        print("%s %d^3, %d frames: trunc %.6g, vref %.6g (half ulp %.3g)" % (r["scene"], r["N"], r["frames"], r["trunc"], r["vref"], r["ulp"]))
        for c in r["checkpoints"]:
            print("  frame %4d  free cells %7d  max |v - vref| %.5f rel (%5.1f ulps)  worst so far %.5f" %
                  (c["frame"], c["free"], c["max_rel"], c["max_ulps"], c["worst_rel_so_far"]))
    worst = max(r["max_rel"] for r in res)
    print("largest relative deviation of free space: %.5f; KFX_SUMMARY_HALF_BAND = %.6f (margin x%.2f)" % (worst, band, band / max(worst, 1e-30)))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(dict(band=band, worst=worst, runs=res), fh, indent=1)
    return 0 if worst <= band else 1


if __name__ == "__main__":
    sys.exit(main())
