"""Ranks of the Z-slab pipeline on ONE GPU (gloo collectives, as tests/mp_slab_gpu.py) meshing their slabs: after a few fused frames
every rank's SlabPipeline.ExtractMesh() equals, in order, the triangles of the single-volume mesh whose cubes it owns, and the rank
meshes together equal that mesh as a multiset of triangles.  Launched by tests/test_gpu_mesh_volumes.py; prints MESH_OK per rank.

    python -m torch.distributed.run --nproc-per-node 3 tests/mp_slab_mesh_gpu.py <halo> <prefix>
"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kangaroo_amd import mesh, roo, scenes  # noqa: E402
from kangaroo_amd.pipeline import FramePipeline, SlabPipeline  # noqa: E402

halo, prefix = sys.argv[1], sys.argv[2]
torch.cuda.set_device(0)
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
N, W, H, FRAMES, scene = 72, 160, 120, 3, "room"
bmin, bmax, near, far = scenes.SCENES[scene]

pipe = SlabPipeline(roo, dist, (N, N, N), bmin, bmax, W, H, halo=halo, raycast="exact", near=near, far=far)
ref = FramePipeline(roo, (N, N, N), bmin, bmax, W, H, near=near, far=far)
for i in range(FRAMES):
    T_wc = scenes.orbit_pose(i, 8)
    depth = scenes.render_depth(scene, W, H, T_wc, pipe.K)
    pipe.raw.MemcpyFromHost(depth)
    pipe.preprocess()
    pipe.fuse(T_wc)
    ref.raw.MemcpyFromHost(depth)
    ref.preprocess()
    roo.SdfFuse(ref.vol, ref.filtered, ref.normals, scenes.se3_inverse(T_wc), ref.K, ref.trunc, ref.max_w, ref.mincostheta)
v, n = pipe.ExtractMesh()
nt = pipe.SaveMesh(prefix)
wv, wn, _, ci, to = mesh.ExtractMesh(ref.vol, with_index=True)
torch.cuda.synchronize()
v, n, wv, wn = (x.cpu().numpy() for x in (v, n, wv, wn))
ci, to = ci.cpu().numpy(), to.cpu().numpy().view(np.uint32).astype(np.int64)
ntri = np.diff(np.append(to, len(wv) // 3))
cube_z = np.repeat(ci % (N - 1), ntri)                         # the cube of every triangle of the whole mesh
mine = np.repeat((cube_z >= pipe.z0) & (cube_z < min(pipe.z1, N - 1)), 3)
assert len(wv) > 3000 and len(v) == mine.sum() and nt == len(v) // 3, (len(v), int(mine.sum()))
assert np.array_equal(v.view(np.uint32), wv[mine].view(np.uint32)) and np.array_equal(n.view(np.uint32), wn[mine].view(np.uint32)), \
    "rank %d: slab mesh differs from its part of the single-volume mesh" % rank
ply = open("%s.r%d.ply" % (prefix, rank), "rb").read()
assert b"element face %d\n" % nt in ply[:400]
# the rank meshes together = the whole mesh as a multiset of triangles
parts = [None] * world
dist.all_gather_object(parts, np.concatenate([v, n], 1).reshape(-1, 18).view(np.uint32))
if rank == 0:
    allt = np.concatenate(parts)
    whole = np.concatenate([wv, wn], 1).reshape(-1, 18).view(np.uint32)
    key = lambda a: a[np.lexsort(a.T[::-1])]
    assert allt.shape == whole.shape and np.array_equal(key(allt), key(whole)), "rank meshes do not partition the whole mesh"
dist.barrier()
print("MESH_OK rank %d triangles %d" % (rank, nt), flush=True)
dist.destroy_process_group()
