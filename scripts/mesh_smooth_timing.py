#!/usr/bin/env python3
"""Mesh smoothing timings (include/kfx_mesh_smooth.h) on the 512^3 fp32 S_room orbit mesh of the other mesh rows (scripts/mesh_timing.py's
volume: 30 orbit frames, 640x480, fast numerics), after the clean-up's min_faces filter -- the input of scripts/mesh_simplify_timing.py.
One process, interleaved repeats; every sample is the wall time of INNER back-to-back calls ending in a device synchronise, divided by
INNER.  One JSON line per operation:
  adjacency     kfx_mesh_adjacency with the flags: validate, count, scan, fill, rank, flags, and its one read-back
  taubin_1      kfx_mesh_smooth, one iteration (lambda 0.5, mu -0.53, the boundary pinned) on that adjacency: the two validations, the
                neighbour table, two passes, one read-back
  taubin_5      ... five iterations: ten passes
  normals       kfx_mesh_vertex_normals on that adjacency
  smooth_mesh_5 the three in a row -- adjacency, five iterations, normals of the result: what smooth=5 costs on top of the extraction
each with
  device_ms        the call(s)
  extract_ms       kfx_mesh_plan + kfx_mesh_index_plan + kfx_mesh_emit_indexed, the extraction that produces the mesh (unchanged code)
  host_route_ms    what a user does without it: download the arrays the call reads, run the numpy oracle (tests/mesh_smooth.py) on the
                   CPU, upload the result (one sample: it takes seconds)
The device's output is compared with the host route's, bit for bit, for every operation before anything is timed (same_as_host_route).
--kernels: only the device calls, a few times, for a rocprofv3 --kernel-trace --stats run (kernel times; the tracer slows the host).
Usage: python scripts/mesh_smooth_timing.py --out profiles/mesh_smooth/timing.jsonl [--reps 7] [--inner 5] [--min-faces 200]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_smooth", "timing.jsonl"))
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--min-faces", type=int, default=200)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    from kangaroo_amd import _lib, mesh
    import mesh_smooth as SM
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
    abytes, sbytes = L.kfx_mesh_adjacency_scratch_bytes(V, T), L.kfx_mesh_smooth_scratch_bytes(V, T)
    ascratch, sscratch = (torch.empty(n, dtype=torch.uint8, device="cuda") for n in (abytes, sbytes))
    nscratch = torch.empty(256, dtype=torch.uint8, device="cuda")
    start = torch.empty(V + 1, dtype=torch.int32, device="cuda")
    inc = torch.empty(3 * T, dtype=torch.int32, device="cuda")
    flags = torch.empty(V, dtype=torch.int32, device="cuda")
    overts, onorms = (torch.empty((V, 3), dtype=torch.float32, device="cuda") for _ in range(2))

    def adjacency():
        _lib.check(L.kfx_mesh_adjacency(ptr(faces), T, V, ptr(start), ptr(inc), ptr(flags), ptr(ascratch), abytes, None))

    def taubin(iterations):
        return lambda: _lib.check(L.kfx_mesh_smooth(ptr(verts), ptr(faces), T, V, ptr(start), ptr(inc), ptr(flags), iterations, 0.5, -0.53, 1, ptr(overts),
                                                    ptr(sscratch), sbytes, None))

    def normals(of=verts):
        return lambda: _lib.check(L.kfx_mesh_vertex_normals(ptr(of), ptr(faces), T, V, ptr(start), ptr(inc), ptr(onorms), ptr(nscratch), 256, None))

    def smooth_mesh():
        adjacency()
        taubin(5)()
        normals(overts)()

    device = {"adjacency": adjacency, "taubin_1": taubin(1), "taubin_5": taubin(5), "normals": normals(), "smooth_mesh_5": smooth_mesh}
    adjacency()
    if a.kernels:
        for _ in range(3):
            extract()
            for fn in device.values():
                fn()
        torch.cuda.synchronize()
        print(json.dumps(dict(kernels_only=True, vertices=V, triangles=T)))
        return

    down = lambda t: t.cpu().numpy()
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    words = lambda t: down(t).view(np.uint32)

    # the host routes: (what is downloaded, the oracle on it, what is uploaded) and the device arrays that must equal the upload
    def host_adjacency():
        f = down(faces).view(np.uint32)
        return [up(x.view(np.int32)) for x in SM.adjacency(V, f)]

    def host_taubin(iterations):
        def route():
            v, f = down(verts), down(faces).view(np.uint32)
            adj = tuple(words(t) for t in (start, inc, flags))
            return [up(SM.smooth(v, f, iterations=iterations, pin_mask=1, adj=adj))]
        return route

    def host_normals():
        v, f = down(verts), down(faces).view(np.uint32)
        return [up(SM.vertex_normals(v, f, adj=(words(start), words(inc))))]

    def host_smooth_mesh():
        v, f = down(verts), down(faces).view(np.uint32)
        adj = SM.adjacency(V, f)
        out = SM.smooth(v, f, iterations=5, pin_mask=1, adj=adj)
        return [up(out), up(SM.vertex_normals(out, f, adj=adj))]

    host = {"adjacency": (host_adjacency, lambda: (start, inc, flags)), "taubin_1": (host_taubin(1), lambda: (overts,)),
            "taubin_5": (host_taubin(5), lambda: (overts,)), "normals": (host_normals, lambda: (onorms,)),
            "smooth_mesh_5": (host_smooth_mesh, lambda: (overts, onorms))}

    def sample(fn):
        def many():
            for _ in range(a.inner):
                fn()
        return wall(many) / a.inner

    # the same answer, for every operation, before anything is timed; the host route is timed here: one sample
    same, host_ms = {}, {}
    for name, (route, outputs) in host.items():
        device[name]()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = route()
        torch.cuda.synchronize()
        host_ms[name] = 1e3 * (time.perf_counter() - t0)
        same[name] = all(torch.equal(g.view(torch.int32), w.view(torch.int32)) for g, w in zip(outputs(), want))
        print("# %s: host route %.0f ms, same %s" % (name, host_ms[name], same[name]), flush=True)

    fns = dict(device, extract=extract)
    for fn in fns.values():
        sample(fn)
    times = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, fn in fns.items():
            times[k].append(sample(fn))
    med = {k: float(np.median(v)) for k, v in times.items()}
    flag_counts = {name: int(((words(flags) & bit) != 0).sum()) for name, bit in (("boundary", 1), ("nonmanifold", 2), ("degenerate", 4), ("isolated", 8))}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for name in device:
        rec = dict(case=str(N), dims=[N, N, N], cell="f32", min_faces=a.min_faces, extracted_vertices=V0, extracted_triangles=T0, vertices=V, triangles=T,
                   op=name, adjacency_scratch_bytes=int(abytes), smooth_scratch_bytes=int(sbytes), mesh_bytes=24 * V + 12 * T, flagged=flag_counts,
                   reps=a.reps, inner=a.inner, same_as_host_route=bool(same[name]),
                   device_ms=round(med[name], 4), device_spread_ms=[round(float(min(times[name])), 4), round(float(max(times[name])), 4)],
                   extract_ms=round(med["extract"], 4), extract_spread_ms=[round(float(min(times["extract"])), 4), round(float(max(times["extract"])), 4)],
                   host_route_ms=round(host_ms[name], 1))
        rec["device_over_extract"] = round(rec["device_ms"] / rec["extract_ms"], 3)
        rec["host_route_over_device"] = round(rec["host_route_ms"] / rec["device_ms"], 1)
        print(json.dumps(rec), flush=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
