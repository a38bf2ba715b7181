#!/usr/bin/env python3
"""Mesh clean-up timings (include/kfx_mesh_clean.h) on the 512^3 fp32 S_room orbit mesh of the other mesh rows (scripts/mesh_timing.py's
volume: 30 orbit frames, 640x480, fast numerics).  One process, interleaved repeats; every sample is the wall time of INNER back-to-back
calls ending in a device synchronise, divided by INNER:
  extract_ms          kfx_mesh_plan + kfx_mesh_index_plan + kfx_mesh_emit_indexed, the extraction that produces the input (unchanged code)
  components_plan_ms  kfx_mesh_components_plan: validate, init, unite, flatten, count, roots, scan, and its one read-back
  filter_plan_ms      kfx_mesh_filter_plan at min_faces (the scratch check's read-back, count, two scans, remap, the totals' read-back)
  filter_emit_ms      kfx_mesh_filter_emit: the scratch check's read-back, the gather and the face rewrite
  clean_ms            the three in a row: what FilterMesh costs on top of the extraction
  host_route_ms       what a user does today: download the faces, label them with numpy on the CPU (min-label propagation with pointer
                      jumping: tests/mesh_components.py), upload a keep mask per vertex; host_download_ms is its first step alone
The device's labels, counts and filtered faces are compared with the host route's at this size before anything is timed.
--kernels: only the device calls, a few times, for a rocprofv3 --kernel-trace --stats run (kernel times; the tracer slows the host).
Usage: python scripts/mesh_clean_timing.py --out profiles/mesh_clean/timing.jsonl [--reps 9] [--inner 10] [--min-faces 200]"""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_clean", "timing.jsonl"))
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--min-faces", type=int, default=200)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    from kangaroo_amd import _lib, mesh
    import mesh_components as MC
    from mesh_timing import fused_volume, wall

    N = a.res
    vol = fused_volume(N, "f32")
    L = _lib.load()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    U2 = C.c_ulonglong * 2

    # the extraction, call by call, into buffers allocated once
    nbytes = L.kfx_mesh_scratch_bytes(vol.ref(), 0, None, 0, 0)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    totals, nvert = U2(), C.c_ulonglong(0)
    _lib.check(L.kfx_mesh_plan(vol.ref(), 0, None, 0, 0, ptr(scratch), nbytes, totals, None))
    xbytes = L.kfx_mesh_index_scratch_bytes(vol.ref(), 0, None, 0, 0, totals)
    xscratch = torch.empty(xbytes, dtype=torch.uint8, device="cuda")
    _lib.check(L.kfx_mesh_index_plan(vol.ref(), 0, None, 0, 0, ptr(scratch), nbytes, totals, ptr(xscratch), xbytes, C.byref(nvert), None))
    V, T = int(nvert.value), int(totals[1])
    verts, norms = (torch.empty((V, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    faces = torch.empty((T, 3), dtype=torch.int32, device="cuda")

    def extract():
        _lib.check(L.kfx_mesh_plan(vol.ref(), 0, None, 0, 0, ptr(scratch), nbytes, totals, None))
        _lib.check(L.kfx_mesh_index_plan(vol.ref(), 0, None, 0, 0, ptr(scratch), nbytes, totals, ptr(xscratch), xbytes, C.byref(nvert), None))
        _lib.check(L.kfx_mesh_emit_indexed(vol.ref(), 0, None, 0, 0, None, ptr(xscratch), xbytes, totals, V, ptr(verts), ptr(norms), None, ptr(faces), None))

    extract()
    cbytes = L.kfx_mesh_components_scratch_bytes(V, T)
    cscratch = torch.empty(cbytes, dtype=torch.uint8, device="cuda")
    counts, kept = U2(), U2()
    components_plan = lambda: _lib.check(L.kfx_mesh_components_plan(ptr(faces), T, V, ptr(cscratch), cbytes, counts, None))
    filter_plan = lambda: _lib.check(L.kfx_mesh_filter_plan(ptr(cscratch), cbytes, V, T, ptr(faces), a.min_faces, 0, kept, None))
    components_plan()
    filter_plan()
    kv, kt = int(kept[0]), int(kept[1])
    overts, onorms = (torch.empty((kv, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    ofaces = torch.empty((kt, 3), dtype=torch.int32, device="cuda")
    filter_emit = lambda: _lib.check(L.kfx_mesh_filter_emit(ptr(cscratch), cbytes, V, T, kept, ptr(verts), ptr(norms), None, ptr(faces), ptr(overts),
                                                            ptr(onorms), None, ptr(ofaces), None))
    filter_emit()

    def clean():
        components_plan()
        filter_plan()
        filter_emit()

    if a.kernels:
        for _ in range(3):
            extract()
            clean()
        torch.cuda.synchronize()
        print(json.dumps(dict(kernels_only=True, vertices=V, triangles=T, components=int(counts[0]))))
        return

    def host_download():
        return faces.cpu().numpy().view(np.uint32)

    def host_route():
        f = host_download()
        vc, cf = MC.components(f, V)
        keep = MC.kept_components(cf, a.min_faces)[vc]
        return torch.from_numpy(keep).cuda(), vc, cf

    # the same answer, at this size, before anything is timed
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mask, vc, cf = host_route()
    torch.cuda.synchronize()
    first_host_ms = 1e3 * (time.perf_counter() - t0)   # (the first of the host route's samples: it takes seconds, so it is not repeated often)
    dvc = torch.empty(V, dtype=torch.int32, device="cuda")
    dcf = torch.empty(int(counts[0]), dtype=torch.int32, device="cuda")
    _lib.check(L.kfx_mesh_components_emit(ptr(cscratch), cbytes, V, T, counts, ptr(dvc), ptr(dcf), None))
    same = bool(np.array_equal(dvc.cpu().numpy().view(np.uint32), vc) and np.array_equal(dcf.cpu().numpy().view(np.uint32), cf))
    host_mask, host_faces = mask.cpu().numpy(), host_download().astype(np.int64)
    want_faces = (np.cumsum(host_mask) - 1)[host_faces[host_mask[host_faces[:, 0]]]]
    same = same and int(mask.sum()) == kv and np.array_equal(ofaces.cpu().numpy().view(np.uint32), want_faces)
    same = same and bool(torch.equal(overts.view(torch.int32), verts[mask].view(torch.int32)))

    fns = {"extract_ms": extract, "components_plan_ms": components_plan, "filter_plan_ms": filter_plan, "filter_emit_ms": filter_emit, "clean_ms": clean}

    def sample(fn):
        def many():
            for _ in range(a.inner):
                fn()
        return wall(many) / a.inner

    for fn in fns.values():
        sample(fn)
    times = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, fn in fns.items():
            times[k].append(sample(fn))
    host = {"host_route_ms": [first_host_ms], "host_download_ms": [wall(host_download)]}
    for _ in range(a.host_reps - 1 if first_host_ms < 30e3 else 0):
        host["host_route_ms"].append(wall(host_route))
        host["host_download_ms"].append(wall(host_download))
    times.update(host)
    rec = dict(case=str(N), dims=[N, N, N], cell="f32", vertices=V, triangles=T, components=int(counts[0]), largest_faces=int(counts[1]),
               min_faces=a.min_faces, kept_vertices=kv, kept_triangles=kt, clean_scratch_bytes=int(cbytes), mesh_bytes=24 * V + 12 * T,
               reps=a.reps, inner=a.inner, host_reps=len(host["host_route_ms"]), same_as_host_route=same)
    rec.update({k: round(float(np.median(v)), 4) for k, v in times.items()})
    rec.update({k.replace("_ms", "_spread_ms"): [round(float(min(v)), 4), round(float(max(v)), 4)] for k, v in times.items()})
    rec["clean_over_extract"] = round(rec["clean_ms"] / rec["extract_ms"], 3)
    rec["host_route_over_clean"] = round(rec["host_route_ms"] / rec["clean_ms"], 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    print(json.dumps(rec), flush=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
