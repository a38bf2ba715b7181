#!/usr/bin/env python3
"""Mesh simplification timings (include/kfx_mesh_simplify.h) on the 512^3 fp32 S_room orbit mesh of the other mesh rows
(scripts/mesh_timing.py's volume: 30 orbit frames, 640x480, fast numerics), after the clean-up's min_faces filter, at cells of 2, 4 and 8
voxel sizes anchored at the world origin.  One process, interleaved repeats; every sample is the wall time of INNER back-to-back calls
ending in a device synchronise, divided by INNER.  One JSON line per cell size:
  extract_ms          kfx_mesh_plan + kfx_mesh_index_plan + kfx_mesh_emit_indexed, the extraction that produces the mesh (unchanged code)
  plan_ms             kfx_mesh_simplify_plan: validate, init, the two table builds and their look-up passes, counts, scans, remap, and its
                      one read-back
  emit_ms             kfx_mesh_simplify_emit: the scratch check's read-back, the gather and the face rewrite
  simplify_ms         the two in a row: what SimplifyMesh costs on top of the extraction and the filter
  host_route_ms       what a user does today: download the mesh, cluster it with numpy on the CPU (tests/mesh_simplify.py), upload the
                      result; host_download_ms is its first step alone
The device's output is compared with the host route's, bit for bit, at every cell size before anything is timed.
--kernels: only the device calls, a few times, for a rocprofv3 --kernel-trace --stats run (kernel times; the tracer slows the host).
Usage: python scripts/mesh_simplify_timing.py --out profiles/mesh_simplify/timing.jsonl [--reps 7] [--inner 5] [--min-faces 200]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_simplify", "timing.jsonl"))
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--min-faces", type=int, default=200)
    ap.add_argument("--cells", default="2,4,8")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    from kangaroo_amd import _lib, mesh
    import mesh_simplify as MS
    from mesh_timing import fused_volume, wall

    N = a.res
    vol = fused_volume(N, "f32")
    voxel = float(np.float32((float(vol.boxmax[0]) - float(vol.boxmin[0])) / N))
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
    V0, T0 = int(nvert.value), int(totals[1])
    verts0, norms0 = (torch.empty((V0, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    faces0 = torch.empty((T0, 3), dtype=torch.int32, device="cuda")

    def extract():
        _lib.check(L.kfx_mesh_plan(vol.ref(), 0, None, 0, 0, ptr(scratch), nbytes, totals, None))
        _lib.check(L.kfx_mesh_index_plan(vol.ref(), 0, None, 0, 0, ptr(scratch), nbytes, totals, ptr(xscratch), xbytes, C.byref(nvert), None))
        _lib.check(L.kfx_mesh_emit_indexed(vol.ref(), 0, None, 0, 0, None, ptr(xscratch), xbytes, totals, V0, ptr(verts0), ptr(norms0), None, ptr(faces0), None))

    extract()
    verts, norms, _, faces = mesh.FilterMesh(verts0, norms0, None, faces0, min_faces=a.min_faces)   # floaters go first
    V, T = len(verts), len(faces)
    sbytes = L.kfx_mesh_simplify_scratch_bytes(V, T)
    sscratch = torch.empty(sbytes, dtype=torch.uint8, device="cuda")
    origin = (C.c_float * 3)(0, 0, 0)
    overts, onorms = (torch.empty((V, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    ofaces = torch.empty((T, 3), dtype=torch.int32, device="cuda")
    kept = U2()

    def calls(cell):
        plan = lambda: _lib.check(L.kfx_mesh_simplify_plan(ptr(verts), ptr(faces), T, V, origin, cell, ptr(sscratch), sbytes, kept, None))
        emit = lambda: _lib.check(L.kfx_mesh_simplify_emit(ptr(sscratch), sbytes, V, T, kept, ptr(verts), ptr(norms), None, ptr(faces), ptr(overts),
                                                           ptr(onorms), None, ptr(ofaces), None, None))

        def both():
            plan()
            emit()
        return plan, emit, both

    cells = [float(np.float32(float(k) * voxel)) for k in a.cells.split(",")]
    if a.kernels:
        for cell in cells:
            for _ in range(3):
                extract()
                calls(cell)[2]()
        torch.cuda.synchronize()
        print(json.dumps(dict(kernels_only=True, vertices=V, triangles=T, cells=cells)))
        return

    def host_download():
        return verts.cpu().numpy(), norms.cpu().numpy(), faces.cpu().numpy().view(np.uint32)

    def sample(fn):
        def many():
            for _ in range(a.inner):
                fn()
        return wall(many) / a.inner

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for name, cell in zip(a.cells.split(","), cells):
        plan, emit, both = calls(cell)
        both()
        kv, kt = int(kept[0]), int(kept[1])

        def host_route():
            v, n, f = host_download()
            out = MS.simplify(v, n, None, f, cell)
            return out, [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (out[0], out[1], out[3].view(np.int32))]

        # the same answer, at this size, before anything is timed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want, _ = host_route()
        torch.cuda.synchronize()
        host_ms = 1e3 * (time.perf_counter() - t0)   # (it takes seconds: one sample)
        same = (kv, kt) == (len(want[0]), len(want[3]))
        same = same and np.array_equal(overts[:kv].cpu().numpy().view(np.uint32), want[0].view(np.uint32))
        same = same and np.array_equal(onorms[:kv].cpu().numpy().view(np.uint32), want[1].view(np.uint32))
        same = same and np.array_equal(ofaces[:kt].cpu().numpy().view(np.uint32), want[3])

        fns = {"extract_ms": extract, "plan_ms": plan, "emit_ms": emit, "simplify_ms": both}
        for fn in fns.values():
            sample(fn)
        times = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, fn in fns.items():
                times[k].append(sample(fn))
        times["host_route_ms"] = [host_ms]
        times["host_download_ms"] = [wall(host_download)]
        rec = dict(case=str(N), dims=[N, N, N], cell="f32", min_faces=a.min_faces, extracted_vertices=V0, extracted_triangles=T0, vertices=V, triangles=T,
                   cell_voxels=float(name), cell_size=cell, kept_vertices=kv, kept_triangles=kt, vertex_ratio=round(kv / V, 4), triangle_ratio=round(kt / T, 4),
                   simplify_scratch_bytes=int(sbytes), mesh_bytes=24 * V + 12 * T, output_bytes=24 * kv + 12 * kt, reps=a.reps, inner=a.inner,
                   same_as_host_route=bool(same))
        rec.update({k: round(float(np.median(v)), 4) for k, v in times.items()})
        rec.update({k.replace("_ms", "_spread_ms"): [round(float(min(v)), 4), round(float(max(v)), 4)] for k, v in times.items()})
        rec["simplify_over_extract"] = round(rec["simplify_ms"] / rec["extract_ms"], 3)
        rec["host_route_over_simplify"] = round(rec["host_route_ms"] / rec["simplify_ms"], 1)
        print(json.dumps(rec), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
