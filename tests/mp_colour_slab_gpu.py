"""Two or three ranks of the COLOUR Z-slab pipeline on ONE GPU, real HIP operators, collectives over gloo (tests/mp_slab_gpu.py's
set-up).  Launched by tests/test_gpu_colour_multi_rank.py through torch.distributed.run:

    python -m torch.distributed.run --nproc-per-node 3 tests/mp_colour_slab_gpu.py <halo> <raycast>

Every rank steps SlabPipeline(color=True) with the Python driver and with the C driver (kfx_slab_frame_step after
kfx_slab_frame_set_color; exact raycast: plain and pipelined) next to the single-volume FramePipeline(color=True) it runs itself.
Rank 0 gathers every frame's colour image and the final volumes of all ranks and compares them with the single-GPU pipeline's, bit for
bit (exact raycast; the composite's images are compared between the two drivers, its volumes with the single volume)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kangaroo_amd import roo, scenes  # noqa: E402
from kangaroo_amd.pipeline import FramePipeline, SlabPipeline  # noqa: E402
import kfx_testlib as T  # noqa: E402

halo, raycast = sys.argv[1], sys.argv[2]
torch.cuda.set_device(0)
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
N, W, H, FRAMES, scene = 96, 160, 120, 5, "room"
bmin, bmax, near, far = scenes.SCENES[scene]

variants = [dict(driver="python"), dict(driver="c", tiles=4)]
if raycast == "exact":
    variants.append(dict(driver="c", tiles=1, overlap=True, pipeline=2))
pipes = [SlabPipeline(roo, dist, (N, N, N), bmin, bmax, W, H, halo=halo, raycast=raycast, near=near, far=far, color=True, **v) for v in variants]
ref = FramePipeline(roo, (N, N, N), bmin, bmax, W, H, near=near, far=far, color=True, track=False)


def gather(arr):
    """every rank's array on rank 0 (a list), through an all-gather of the bit patterns"""
    t = torch.from_numpy(np.ascontiguousarray(arr).view(np.int32).reshape(-1).copy())
    n = torch.tensor([t.numel()])
    sizes = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(sizes, n)
    m = int(max(int(s) for s in sizes))
    pad = torch.zeros(m, dtype=torch.int32)
    pad[:t.numel()] = t
    parts = [torch.zeros(m, dtype=torch.int32) for _ in range(world)]
    dist.all_gather(parts, pad)
    return [p[:int(s)].numpy() for p, s in zip(parts, sizes)]


failures = []
for i in range(FRAMES):
    T_wc = scenes.orbit_pose(i, 8)
    depth = scenes.render_depth(scene, W, H, T_wc, ref.K)
    rgb = scenes.render_rgb(scene, W, H, T_wc, ref.Kimg)
    for p_ in pipes + [ref]:
        p_.raw.MemcpyFromHost(depth)
        p_.rgb.MemcpyFromHost(rgb)
        p_.step(T_wc)
    for p_ in pipes:
        p_.wait_composite()
        if p_.sframe is not None:
            p_.sframe.sync()
    torch.cuda.synchronize()
    want = [x.MemcpyToHost() for x in (ref.ray_d, ref.ray_n, ref.ray_i)]
    if raycast != "exact":   # the composite restarts the march at each slab: the Python driver's images are the yardstick of the C driver's
        want = [x.MemcpyToHost() for x in (pipes[0].ray_d, pipes[0].ray_n, pipes[0].ray_i)]
    for v, p_ in zip(variants, pipes):
        got = [x.MemcpyToHost() for x in (p_.ray_d, p_.ray_n, p_.ray_i)]
        all_imgs = gather(got[2])                      # every rank's colour image of this frame, on rank 0
        for r, im in enumerate(all_imgs):
            if not np.array_equal(im, want[2].view(np.int32).reshape(-1)):
                failures.append("frame %d %r: rank %d's colour image differs" % (i, v, r))
        for name, a, b in zip(("depth", "normals"), got, want):
            if not T.nan_equal(a, b):
                failures.append("frame %d %r: rank %d's %s differ" % (i, v, rank, name))
    hit = np.isfinite(want[0])
    assert hit.mean() > 0.3 and np.ptp(want[2][hit]) > 0.2

full, cfull = ref.vol.MemcpyToHost(), ref.cvol.MemcpyToHost()
assert (cfull != 0.5).mean() > 0.2
for v, p_ in zip(variants, pipes):
    vols, cols = gather(p_.vol.MemcpyToHost()), gather(p_.cvol.MemcpyToHost())
    spans = gather(np.array([p_.s0, p_.s1], np.int32))
    for r in range(world):
        s0, s1 = int(spans[r][0]), int(spans[r][1])
        # NaN cells: compare as floats (any NaN equals any NaN)
        if not T.nan_equal(vols[r].view(np.float32).reshape(full[s0:s1].shape), full[s0:s1]):
            failures.append("%r: rank %d's SDF slab differs from the single volume" % (v, r))
        if not T.nan_equal(cols[r].view(np.float32).reshape(cfull[s0:s1].shape), cfull[s0:s1]):
            failures.append("%r: rank %d's colour slab differs from the single volume" % (v, r))
assert not failures, failures[:8]   # (the gathered comparisons are every rank's; depth and normals are each rank's own)
# meshes: this rank's part carries colours
vt, nm, cl = pipes[0].ExtractMesh()
assert cl is not None and len(cl) == len(vt)
dist.barrier()
print("MP_OK rank %d of %d (colour, %s, %s)" % (rank, world, halo, raycast), flush=True)
for p_ in pipes:
    p_.sframe = None
dist.destroy_process_group()
