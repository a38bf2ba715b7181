"""The planned mesh extraction (include/kfx_mesh.h: kfx_mesh_plan / kfx_mesh_emit) on every volume the fuser writes:
  * fp32, whole volume: the cube lists are nonzero / cumsum of kfx_mc_count's bytes and the arrays kfx_mc_emit's, bit for bit;
  * half cells: the mesh of the exactly widened volume -- the oracle's marching cubes of it, bit for bit, in emission order;
  * Z-slab views (ghost 2; 1 is refused) and SlabPipeline ranks: every rank's mesh is, in order, the single-volume mesh's triangles
    of the cubes it owns, and the ranks together hold every triangle once;
  * scale: 1024^3 fp32 against the byte-per-cube path, 2048^3 half cells with cube indices beyond 2^32."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import oracle, scenes

pytestmark = pytest.mark.gpu


def old_path(vol, cvol=None):
    """kfx_mc_count -> torch.nonzero / torch.cumsum -> kfx_mc_emit: the compaction this change replaces."""
    import torch
    from kangaroo_amd import _lib
    L = _lib.load()
    dev = vol.storage.device
    counts = torch.empty((vol.w - 1) * (vol.h - 1) * (vol.d - 1), dtype=torch.uint8, device=dev)
    _lib.check(L.kfx_mc_count(vol.ref(), C.c_void_p(counts.data_ptr()), None))
    active = torch.nonzero(counts).reshape(-1)
    ca = counts[active].to(torch.int64)
    incl = torch.cumsum(ca, 0)
    ntri = int(incl[-1].item()) if incl.numel() else 0
    tri_offset = (incl - ca).to(torch.int32)
    verts = torch.empty((3 * ntri, 3), dtype=torch.float32, device=dev)
    norms = torch.empty((3 * ntri, 3), dtype=torch.float32, device=dev)
    colors = torch.empty((3 * ntri, 4), dtype=torch.float32, device=dev) if cvol is not None else None
    if ntri:
        _lib.check(L.kfx_mc_emit(vol.ref(), cvol.ref() if cvol is not None else None, C.c_void_p(active.data_ptr()),
                                 C.c_void_p(tri_offset.data_ptr()), int(active.numel()), C.c_void_p(verts.data_ptr()),
                                 C.c_void_p(norms.data_ptr()), C.c_void_p(colors.data_ptr()) if cvol is not None else None, None))
    return verts, norms, colors, active, tri_offset, counts


def bits_equal(a, b):
    import torch
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def volume_case(roo, case):
    import test_color_cpu as TC
    import test_mesh_cpu as TM
    ocvol = None
    if case == "sphere":
        ovol = TM.sphere_volume(48, 0.7)
    elif case == "fused_room_colour":
        ovol, ocvol, K, Kimg, tr, near, far, inputs = TC.color_setup(0, 160, 120, 160, 120, dims=(64, 64, 64))
        for fr in inputs:
            oracle.sdf_fuse_color(ovol, ocvol, fr["f"], fr["nrm"], fr["T_cw"], K, fr["rgb"], fr["T_iw"], Kimg, tr, 1000.0, 0.1, nthreads=0)
    else:
        ovol = oracle.Volume(21, 13, 34, (-1, -0.5, -1), (1, 0.7, 1.5), pitch_bytes=21 * 8 + 40)
        oracle.sdf_sphere(ovol, (0.1, 0.0, 0.2), 0.45)
        ovol.data[:, :, :, 0][(np.add.outer(np.add.outer(np.arange(34), np.arange(13)), np.arange(21)) % 7) == 0] = np.nan
    vol = roo.BoundedVolume(ovol.w, ovol.h, ovol.d, ovol.boxmin, ovol.boxmax, pitch=ovol.pitch if case == "ragged_unobserved" else None)
    vol.MemcpyFromHost(ovol.data)
    cvol = None
    if ocvol is not None:
        cvol = roo.BoundedVolume(ocvol.w, ocvol.h, ocvol.d, ocvol.boxmin, ocvol.boxmax, kind="c32")
        cvol.MemcpyFromHost(ocvol.data)
    return vol, cvol


@pytest.mark.parametrize("case", ["sphere", "fused_room_colour", "ragged_unobserved"])
def test_gpu_mesh_f32_whole_volume_equals_the_byte_per_cube_path(roo, case):
    from kangaroo_amd import mesh
    vol, cvol = volume_case(roo, case)
    v, n, c, ci, to = mesh.ExtractMesh(vol, cvol, with_index=True)
    ov, on, oc, oa, oto, counts = old_path(vol, cvol)
    assert len(v) > 300 and bits_equal(ci, oa) and bits_equal(to, oto)
    assert bits_equal(v, ov) and bits_equal(n, on) and bits_equal(c, oc)
    assert (cvol is None) == (c is None)


def widened(ovh):
    ov = oracle.Volume(ovh.w, ovh.h, ovh.d, ovh.boxmin, ovh.boxmax)
    ov.data[...] = ovh.data.astype(np.float32)
    return ov


@pytest.mark.parametrize("case", ["room_96", "ragged_nan_80x64x72", "full_64_colour"])
def test_gpu_mesh_half_cells_equal_the_oracle_of_the_widened_volume(roo, case):
    import test_mesh_cpu as TM
    from kangaroo_amd import mesh
    ntri, mask, tri = TM.tables()
    scene, dims, pitch = {"room_96": ("room", (96, 96, 96), None), "ragged_nan_80x64x72": ("room", (80, 64, 72), 80 * 4 + 52),
                          "full_64_colour": ("full", (64, 64, 64), None)}[case]
    bmin, bmax, near, far = scenes.SCENES[scene]
    w, h = 160, 120
    K = scenes.intrinsics(w, h)
    tr = scenes.trunc_dist(bmin, bmax, dims)
    ovh = oracle.VolumeH(*dims, bmin, bmax, pitch_bytes=pitch)
    oracle.sdf_reset(ovh, float("nan"))
    vol = roo.BoundedVolume(*dims, bmin, bmax, kind="f16", pitch=pitch)
    roo.SdfReset(vol, float("nan"))
    for i in range(3):
        T_wc = scenes.orbit_pose(i, 8)
        f, vbo, nrm = T.preprocess_oracle(scenes.render_depth(scene, w, h, T_wc, K), K)
        T_cw = scenes.se3_inverse(T_wc)
        oracle.sdf_fuse(ovh, f, nrm, T_cw, K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, nthreads=0)
        roo.SdfFuse(vol, T.upload_image(roo, f.data), T.upload_image(roo, nrm.data), T_cw, K, tr, scenes.MAX_W, scenes.MIN_COS_THETA)
    if pitch:   # unobserved cells scattered through the surface band
        cells = ovh.data[:, :, :, 0]
        cells[(np.add.outer(np.add.outer(np.arange(dims[2]), np.arange(dims[1])), np.arange(dims[0])) % 11) == 0] = np.nan
        vol.MemcpyFromHost(ovh.data)
    assert T.nan_equal(vol.MemcpyToHost(), ovh.data)
    ocvol = cvol = None
    if case.endswith("colour"):
        ocvol = oracle.ColorVolume(*dims, bmin, bmax)
        ocvol.data[...] = np.random.default_rng(5).random(ocvol.data.shape, dtype=np.float32)
        cvol = roo.BoundedVolume(*dims, bmin, bmax, kind="c32")
        cvol.MemcpyFromHost(ocvol.data)
    want_v, want_n, want_c = oracle.marching_cubes(widened(ovh), ocvol, ntri, mask, tri)
    assert len(want_v) > 1000
    v, n, c = mesh.ExtractMesh(vol, cvol)
    assert T.nan_equal(v.cpu().numpy(), want_v) and T.nan_equal(n.cpu().numpy(), want_n)
    if ocvol is not None:
        assert T.nan_equal(c.cpu().numpy(), want_c)


def slab_bounds(D, world, ghost):
    from kangaroo_amd.pipeline import slab_range
    for r in range(world):
        z0, z1 = slab_range(D, r, world)
        yield z0, z1, max(z0 - ghost, 0), min(z1 + ghost, D)


def check_slab_views(vol, world, ghost=2):
    """Each rank's view (planes [s0, s1) of `vol`) meshes, in order, the whole mesh's triangles of its cubes; together every triangle once."""
    import torch
    from kangaroo_amd import mesh
    D = vol.d
    zmin, zmax = float(vol.boxmin[2]), float(vol.boxmax[2])
    wv, wn, _, ci, to = mesh.ExtractMesh(vol, with_index=True)
    ntri = torch.diff(torch.cat([to.to(torch.int64) & 0xffffffff, torch.tensor([len(wv) // 3], device=to.device)]))
    cube_z = torch.repeat_interleave(ci % (D - 1), ntri)
    seen = 0
    for z0, z1, s0, s1 in slab_bounds(D, world, ghost):
        v, n, _ = mesh.ExtractMesh(vol.ZSlab(s0, s1), slab=(D, s0, zmin, zmax, z0, z1))
        mine = torch.repeat_interleave((cube_z >= z0) & (cube_z < min(z1, D - 1)), 3)
        assert bits_equal(v, wv[mine]) and bits_equal(n, wn[mine]), (world, z0, z1)
        seen += len(v)
    assert seen == len(wv) and len(wv) > 0
    return len(wv) // 3


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_gpu_mesh_slab_views_partition_the_whole_mesh(roo, kind):
    from kangaroo_amd import _lib, mesh
    D = 88
    bmin, bmax = (-1.0, -0.8, -1.1), (1.0, 0.9, 1.2)
    vol = roo.BoundedVolume(70, 60, D, bmin, bmax, kind=kind)
    roo.SdfSphere(vol, (0.1, -0.05, 0.15), 0.8)
    t = vol.tensor()
    t[..., 0][(torch_arange3(t.shape[:3]) % 13) == 0] = float("nan")
    for world in (2, 3, 5, 8):
        check_slab_views(vol, world)
    # a ghost of one plane does not cover the normals' stencil
    z0, z1, s0, s1 = list(slab_bounds(D, 3, 1))[1]
    with pytest.raises(_lib.KfxError) as e:
        mesh.ExtractMesh(vol.ZSlab(s0, s1), slab=(D, s0, bmin[2], bmax[2], z0, z1))
    assert e.value.code == -4


def torch_arange3(shape):
    import torch
    d, h, w = shape
    return (torch.arange(d, device="cuda")[:, None, None] * 7 + torch.arange(h, device="cuda")[None, :, None] * 3 +
            torch.arange(w, device="cuda")[None, None, :])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("halo", ["exchange", "recompute"])
def test_gpu_slab_pipeline_rank_meshes(halo, tmp_path):
    world = 3
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(T.ROOT, "tests", "mp_slab_mesh_gpu.py"), halo, str(tmp_path / "m")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=T.ROOT)
    assert out.returncode == 0 and out.stdout.count("MESH_OK") == world, out.stdout[-3000:] + out.stderr[-3000:]
    for r in range(world):
        assert (tmp_path / ("m.r%d.ply" % r)).exists()


def test_gpu_mesh_scan_carries_across_chunks_of_block_sums(roo):
    """k_mesh_scan_partials walks the block sums in chunks of 1024 x 8 = 8192 blocks and carries the running totals from chunk to
    chunk.  2050 x 2050 x 3 fp32 (101 MB): cz = 2, one segment per column, 2049^2 = 4 198 401 segments = 8201 blocks of 512, nine of
    them in the second chunk.  All NaN but the columns x < 10 and x >= 2040, which the plane z = 0.5 voxels crosses: active cubes in the
    first blocks and, from segment 2040 * 2049 (block 8164) on, up to the last, whose offsets are right only if the carry is."""
    import torch
    from kangaroo_amd import mesh
    N = 2050
    vol = roo.BoundedVolume(N, N, 3, (-1, -1, 0), (1, 1, 0.002))
    t = vol.tensor()
    t[...] = float("nan")
    for xs in (slice(0, 10), slice(N - 10, N)):
        t[:, :, xs, 0] = (torch.arange(3, device=t.device, dtype=torch.float32) - 0.5)[:, None, None] * 0.25
        t[:, :, xs, 1] = 1.0
    v, n, _, ci, to = mesh.ExtractMesh(vol, with_index=True)
    ov, on, _, oa, oto, counts = old_path(vol)
    assert len(ci) == 2 * 9 * (N - 1) and int(ci[0]) == 0 and int(ci[-1]) == ((N - 2) * (N - 1) + N - 2) * 2
    assert int((ci // 2 >= 8192 * 512).sum()) == 2 * (N - 1) - 1   # cubes whose segment (ci / cz) lies in the second chunk
    assert bits_equal(ci, oa) and bits_equal(to, oto) and bits_equal(v, ov) and bits_equal(n, on)
    del vol, t, v, n, ov, on, counts
    torch.cuda.empty_cache()


def test_gpu_mesh_1024_f32_equals_the_byte_per_cube_path(roo):
    import torch
    from kangaroo_amd import mesh
    N = 1024
    vol = roo.BoundedVolume(N, N, N, (-1, -1, -1), (1, 1, 1))
    roo.SdfSphere(vol, (0.05, -0.1, 0.02), 0.6)
    v, n, _, ci, to = mesh.ExtractMesh(vol, with_index=True)
    ov, on, _, oa, oto, counts = old_path(vol)
    assert int(counts.sum(dtype=torch.int64)) == len(v) // 3 and int((counts != 0).sum()) == len(ci)
    assert bits_equal(ci, oa) and bits_equal(to, oto) and bits_equal(v, ov) and bits_equal(n, on)
    del vol, v, n, ov, on, counts
    torch.cuda.empty_cache()


def test_gpu_mesh_2048_half_cells_beyond_32_bit_cube_indices(roo):
    import torch
    from kangaroo_amd import mesh
    N = 2048
    vol = roo.BoundedVolume(N, N, N, (-1, -1, -1), (1, 1, 1), kind="f16")
    roo.SdfSphere(vol, (0.45, 0.0, 0.0), 0.4)      # x in [~1075, ~1893]: cube indices (x*2047 + y)*2047 + z above 2^32
    v, n, _, ci, to = mesh.ExtractMesh(vol, with_index=True)
    assert len(v) > 3_000_000 and int(ci.max()) >= 2 ** 32 and int(ci.min()) >= 2 ** 32
    assert bool(torch.isfinite(v).all()) and bool((ci[1:] > ci[:-1]).all())
    whole = len(v) // 3
    del v, n, ci, to
    torch.cuda.empty_cache()
    parts = 0
    for z0, z1, s0, s1 in slab_bounds(N, 4, 2):
        pv, _, _ = mesh.ExtractMesh(vol.ZSlab(s0, s1), slab=(N, s0, -1.0, 1.0, z0, z1))
        parts += len(pv) // 3
        del pv
    assert parts == whole
    # one 64-plane window through the sphere, widened into an fp32 slab: the same triangles as the half slab call
    s0 = 1000
    win = roo.BoundedVolume(N, N, 64, (-1, -1, float(vol.VoxelPositionInUnits(0, 0, s0)[2])),
                            (1, 1, float(vol.VoxelPositionInUnits(0, 0, s0 + 63)[2])))
    win.tensor().copy_(vol.tensor()[s0:s0 + 64].float())
    sl = (N, s0, -1.0, 1.0, s0 + 2, s0 + 62)
    hv, hn, _ = mesh.ExtractMesh(vol.ZSlab(s0, s0 + 64), slab=sl)
    fv, fn, _ = mesh.ExtractMesh(win, slab=sl)
    assert len(hv) > 10000 and bits_equal(hv, fv) and bits_equal(hn, fn)
    del vol, win, hv, hn, fv, fn
    torch.cuda.empty_cache()
