#!/usr/bin/env python3
"""Mesh extraction timings (include/kfx_mesh.h): the planned path's calls and the whole host-visible ExtractMesh, against the
byte-per-cube path it replaces (kfx_mc_count + torch.nonzero / torch.cumsum + kfx_mc_emit, still callable through the ABI).
Volumes:
  512    512^3 fp32 after the S_room stream (30 orbit frames, 640x480, fast numerics)
  1024   1024^3 fp32, the same stream
  2048h  2048^3 half cells with S_room fused in (the old path cannot take half cells)
Each case reports the median wall time of kfx_mesh_plan (count + reduce + scan + the 16-byte read-back), kfx_mesh_emit (compact +
emit + the totals check) and the whole ExtractMesh call, interleaved with the old path; the count pass's fraction of 8 TB/s by
unique volume bytes comes from the kernel time of a rocprofv3 --kernel-trace run of this script (pass --count-ms to fold it in).
The indexed output (include/kfx_mesh_index.h) is timed in the same process, so that the soup figures beside it are this build's own:
indexed_ms is the whole ExtractMesh(indexed=True) call (plan + index plan + indexed emit, to set against extract_ms), index_plan_ms
and emit_indexed_ms its two added calls alone; ply_bytes / ply_bytes_indexed are the sizes of the binary files of either mesh.
Usage: python scripts/mesh_timing.py --out profiles/r07_mesh/mesh_timing.jsonl [--cases 512,1024,2048h] [--reps 7]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, ORBIT = 640, 480, 30


def fused_volume(N, kind):
    import torch
    from kangaroo_amd import roo, scenes
    roo.set_math_mode("fast")
    bmin, bmax, near, far = scenes.SCENES["room"]
    K = scenes.intrinsics(W, H)
    tr = scenes.trunc_dist(bmin, bmax, (N, N, N))
    vol = roo.BoundedVolume(N, N, N, bmin, bmax, kind=kind)
    roo.SdfReset(vol, float("nan"))
    f, v, n = roo.Image(W, H), roo.Image(W, H, "f32x4"), roo.Image(W, H, "f32x4")
    for i in range(ORBIT):
        T_wc = scenes.orbit_pose(i, ORBIT)
        raw = roo.Image(W, H).MemcpyFromHost(scenes.render_depth("room", W, H, T_wc, K))
        roo.BilateralFilter(f, raw, **scenes.BILATERAL)
        roo.DepthToVbo(v, f, K)
        roo.NormalsFromVbo(n, v)
        roo.SdfFuse(vol, f, n, scenes.se3_inverse(T_wc), K, tr, scenes.MAX_W, scenes.MIN_COS_THETA)
    roo.set_math_mode("exact")
    torch.cuda.synchronize()
    return vol


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def run_case(name, reps):
    import numpy as np
    import torch
    from kangaroo_amd import _lib, mesh
    from test_gpu_mesh_volumes import old_path
    N, kind = {"512": (512, "f32"), "1024": (1024, "f32"), "2048h": (2048, "f16")}[name]
    vol = fused_volume(N, kind)
    L = _lib.load()
    cell = mesh.CELL[kind]
    nbytes = L.kfx_mesh_scratch_bytes(vol.ref(), cell, None, 0, 0)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    totals = (C.c_ulonglong * 2)()
    _lib.check(L.kfx_mesh_plan(vol.ref(), cell, None, 0, 0, C.c_void_p(scratch.data_ptr()), nbytes, totals, None))
    na, nt = int(totals[0]), int(totals[1])
    ci = torch.empty(na, dtype=torch.int64, device="cuda")
    to = torch.empty(na, dtype=torch.int32, device="cuda")
    vv = torch.empty((3 * nt, 3), dtype=torch.float32, device="cuda")
    nn = torch.empty((3 * nt, 3), dtype=torch.float32, device="cuda")
    plan = lambda: _lib.check(L.kfx_mesh_plan(vol.ref(), cell, None, 0, 0, C.c_void_p(scratch.data_ptr()), nbytes, totals, None))
    emit = lambda: _lib.check(L.kfx_mesh_emit(vol.ref(), cell, None, 0, 0, None, C.c_void_p(scratch.data_ptr()), nbytes, totals,
                                              C.c_void_p(ci.data_ptr()), C.c_void_p(to.data_ptr()), C.c_void_p(vv.data_ptr()),
                                              C.c_void_p(nn.data_ptr()), None, None))
    xbytes = L.kfx_mesh_index_scratch_bytes(vol.ref(), cell, None, 0, 0, totals)
    xscratch = torch.empty(xbytes, dtype=torch.uint8, device="cuda")
    nvert = C.c_ulonglong(0)
    index_plan = lambda: _lib.check(L.kfx_mesh_index_plan(vol.ref(), cell, None, 0, 0, C.c_void_p(scratch.data_ptr()), nbytes, totals,
                                                          C.c_void_p(xscratch.data_ptr()), xbytes, C.byref(nvert), None))
    index_plan()
    nv = int(nvert.value)
    ff = torch.empty((nt, 3), dtype=torch.int32, device="cuda")
    emit_indexed = lambda: _lib.check(L.kfx_mesh_emit_indexed(vol.ref(), cell, None, 0, 0, None, C.c_void_p(xscratch.data_ptr()), xbytes, totals, nv,
                                                              C.c_void_p(vv.data_ptr()), C.c_void_p(nn.data_ptr()), None, C.c_void_p(ff.data_ptr()), None))
    fns = {"plan_ms": plan, "emit_ms": emit, "extract_ms": lambda: mesh.ExtractMesh(vol), "index_plan_ms": index_plan,
           "emit_indexed_ms": emit_indexed, "indexed_ms": lambda: mesh.ExtractMesh(vol, indexed=True)}
    if kind == "f32":
        fns["old_path_ms"] = lambda: old_path(vol)
    for f in fns.values():   # warm-up
        wall(f)
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            times[k].append(wall(f))
    rec = dict(case=name, dims=[N, N, N], cell=kind, active_cubes=na, triangles=nt, scratch_bytes=int(nbytes),
               volume_bytes=int(vol.img_pitch * N), reps=reps, vertices=nv, index_scratch_bytes=int(xbytes),
               ply_bytes=(72 + 13) * nt, ply_bytes_indexed=24 * nv + 13 * nt)   # (without the ~300-byte header)
    rec.update({k: round(float(np.median(v)), 4) for k, v in times.items()})
    rec.update({k.replace("_ms", "_spread_ms"): [round(float(min(v)), 4), round(float(max(v)), 4)] for k, v in times.items()})
    if kind == "f32":
        ov = old_path(vol)
        nv = mesh.ExtractMesh(vol)
        rec["same_as_old_path"] = bool(torch.equal(ov[0].view(torch.int32), nv[0].view(torch.int32)) and
                                       torch.equal(ov[1].view(torch.int32), nv[1].view(torch.int32)))
    del vol, scratch
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_mesh", "mesh_timing.jsonl"))
    ap.add_argument("--cases", default="512,1024,2048h")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for name in a.cases.split(","):
        rec = run_case(name, a.reps)
        print(json.dumps(rec), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
