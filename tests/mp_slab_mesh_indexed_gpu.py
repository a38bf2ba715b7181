"""Ranks of the Z-slab pipeline on ONE GPU (gloo collectives, as tests/mp_slab_mesh_gpu.py) meshing their slabs with indexed=True:
every rank's SlabPipeline.ExtractMesh(indexed=True) is the sequential first-occurrence weld of its own ExtractMesh() soup -- ids in
first-occurrence order, first occurrences bit for bit, later copies within 4 ulp of the largest box coordinate -- and
SaveMesh(prefix, indexed=True) writes those V vertices and T faces.  Launched by tests/test_gpu_mesh_indexed.py; prints MESH_OK per rank.

    python -m torch.distributed.run --nproc-per-node 3 tests/mp_slab_mesh_indexed_gpu.py <prefix>
"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kangaroo_amd import roo, scenes  # noqa: E402
from kangaroo_amd.pipeline import SlabPipeline  # noqa: E402

prefix = sys.argv[1]
torch.cuda.set_device(0)
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
N, W, H, FRAMES, scene = 72, 160, 120, 3, "room"
bmin, bmax, near, far = scenes.SCENES[scene]

pipe = SlabPipeline(roo, dist, (N, N, N), bmin, bmax, W, H, halo="exchange", raycast="exact", near=near, far=far)
for i in range(FRAMES):
    T_wc = scenes.orbit_pose(i, 8)
    pipe.raw.MemcpyFromHost(scenes.render_depth(scene, W, H, T_wc, pipe.K))
    pipe.preprocess()
    pipe.fuse(T_wc)
sv, sn = pipe.ExtractMesh()
v, n, f = pipe.ExtractMesh(indexed=True)
nt = pipe.SaveMesh(prefix, indexed=True)
torch.cuda.synchronize()
sv, sn, v, n = (x.cpu().numpy() for x in (sv, sn, v, n))
f = f.cpu().numpy().view(np.uint32)
V = len(v)
assert nt == len(f) == len(sv) // 3 > 500 and V < len(sv) // 3 * 2, (nt, len(f), len(sv), V)
flat = f.reshape(-1).astype(np.int64)
run = np.maximum.accumulate(flat)
assert flat[0] == 0 and run[-1] == V - 1 and (np.diff(run) <= 1).all(), "rank %d: ids are not in first-occurrence order" % rank
firsts = np.r_[0, np.flatnonzero(np.diff(run) > 0) + 1]
assert np.array_equal(v.view(np.uint32), sv[firsts].view(np.uint32)) and np.array_equal(n.view(np.uint32), sn[firsts].view(np.uint32)), \
    "rank %d: a vertex is not its first soup copy" % rank
M = max(abs(float(x)) for x in tuple(bmin) + tuple(bmax))
err = float(np.abs(v[flat].astype(np.float64) - sv.astype(np.float64)).max())
assert err <= 4 * float(np.spacing(np.float32(M))), (rank, err)
raw = open("%s.r%d.ply" % (prefix, rank), "rb").read()
head, body = raw.split(b"end_header\n", 1)
assert b"element vertex %d\n" % V in head and b"element face %d\n" % nt in head and len(body) == 24 * V + 13 * nt
assert np.array_equal(np.frombuffer(body, "<u4", 6 * V), np.concatenate([v, n], 1).reshape(-1).view(np.uint32))
dist.barrier()
print("MESH_OK rank %d triangles %d vertices %d" % (rank, nt, V), flush=True)
dist.destroy_process_group()
