"""The scenes of the brick ray-cast's tests (include/kfx_raycast_bricks.h), defined once for the CPU test of the scenes themselves
(test_brick_raycast_cases_cpu.py, on the oracle) and the GPU test of the kernel (test_gpu_brick_raycast.py).  A plain module.

Every scene: voxel 1/16, so the box is (0, 0, 0) .. (dim - 1) / 16; near 0.1, trunc 0.25, subpix on unless a test says otherwise;
K = (f, f, (w - 1) / 2, (h - 1) / 2); T_wc = [R | cam] with R the identity or rot_y(a) = [[cos a, 0, sin a], [0, 1, 0], [-sin a, 0, cos a]].
"drop5": brick (bx, by, bz) is removed from the list when (bx + 2 by + 3 bz) % 5 == 0.

counts: what oracle.raycast_sdf gives on the dense comparator D (NaN, then the listed bricks): (hits with every brick, hits with drop5,
pixels whose depth or normal bits differ between the two); dropped: (bricks drop5 removes, bricks of the frame)."""
import numpy as np

VOXEL = 1.0 / 16
NEAR, TRUNC = 0.1, 0.25
NAN = float("nan")
# what keeps a GPU comparison from passing vacuously: the comparator hits on at least this share of the pixels and misses on at least
# this share, and (drop5) differs from the all-bricks image on at least DIFFER_FLOOR of them
HIT_FLOOR = MISS_FLOOR = 0.15
DIFFER_FLOOR = 0.10

CASES = {
    # a sphere centred on a brick corner (cell (16, 8, 16)); 96 x 72: sparse lanes
    "A": dict(dims=(40, 24, 32), center=(1.0, 0.5, 1.0), r=0.4, rot=0.0, cam=(1.0, 0.5, -1.5), f=200.0, size=(96, 72), far=10.0,
              counts=(3268, 2259, 1233), dropped=(12, 60)),
    # the same at 200 x 150: dense lanes
    "A2": dict(dims=(40, 24, 32), center=(1.0, 0.5, 1.0), r=0.4, rot=0.0, cam=(1.0, 0.5, -1.5), f=400.0, size=(200, 150), far=10.0,
               counts=(13080, 9041, 4930), dropped=(12, 60)),
    "B": dict(dims=(40, 24, 32), center=(1.0, 0.5, 1.0), r=0.4, rot=np.deg2rad(35.0), cam=(-0.6, 0.4, -1.2), f=200.0, size=(96, 72), far=10.0,
              counts=(2737, 2325, 1737), dropped=(12, 60)),
    # partial bricks on all axes, a surface that leaves through the frame's faces, NaN where (x + y + z) % 7 == 0, a ragged image
    "C": dict(dims=(44, 29, 35), center=(0.5, 0.9, 1.0), r=1.15, rot=-1.0, cam=(2.4, 0.9, 0.2), f=120.0, size=(67, 45), far=10.0,
              counts=(955, 582, 532), dropped=(24, 120), nan7=True),
    # the camera inside the frame
    "D": dict(dims=(40, 24, 32), center=(1.0, 0.5, 1.0), r=0.4, rot=0.0, cam=(1.0, 0.6, 0.1), f=60.0, size=(96, 72), far=10.0,
              counts=(2734, 1966, 1027), dropped=(12, 60)),
    # the shell: of a 128^3 frame only the bricks near the surface (min |val| < 0.3) are listed -- most samples are in absent bricks
    "S": dict(dims=(128, 128, 128), center=(4.0, 4.0, 4.0), r=2.5, rot=0.0, cam=(4.0, 4.0, -3.0), f=120.0, size=(160, 120), far=20.0,
              counts=(6616, 6616, None), kept=(832, 4096), steps_k=(122, 328)),
}


def box(dims):
    return (0.0, 0.0, 0.0), tuple((int(d) - 1) * VOXEL for d in dims)


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)


def pose(case):
    """T_wc, 3 x 4 float32"""
    c = CASES[case] if isinstance(case, str) else case
    return np.hstack([rot_y(c["rot"]), np.asarray(c["cam"], np.float64).reshape(3, 1)]).astype(np.float32)


def intrinsics(case, size=None):
    c = CASES[case] if isinstance(case, str) else case
    w, h = c["size"] if size is None else size
    return np.array([c["f"], c["f"], (w - 1) / 2.0, (h - 1) / 2.0], np.float32)


def brick_grid(dims):
    return tuple((int(d) + 7) // 8 for d in dims)


def brick_coords(ids, dims):
    nbx, nby, _ = brick_grid(dims)
    ids = np.asarray(ids).astype(np.int64)
    return ids % nbx, (ids // nbx) % nby, ids // (nbx * nby)


def drop5(ids, dims):
    """which of the bricks `ids` the drop rule removes (bool array)"""
    bx, by, bz = brick_coords(ids, dims)
    return (bx + 2 * by + 3 * bz) % 5 == 0


def nan7_mask(dims):
    """(d, h, w) bool: the cells case C leaves unobserved"""
    w, h, d = [int(v) for v in dims]
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    return (x + y + z) % 7 == 0


def brick_min_abs(val, dims):
    """min |val| over each brick's cells inside the frame, by brick id; val: (d, h, w), NaN cells ignored"""
    w, h, d = [int(v) for v in dims]
    nbx, nby, nbz = brick_grid(dims)
    pad = np.full((nbz * 8, nby * 8, nbx * 8), np.inf, np.float64)
    a = np.abs(np.asarray(val, np.float64))
    pad[:d, :h, :w] = np.where(np.isnan(a), np.inf, a)
    return pad.reshape(nbz, 8, nby, 8, nbx, 8).min(axis=(1, 3, 5)).reshape(-1)


def shell_keep(val, dims):
    """case S: the ids of the bricks whose min |val| < 0.3"""
    return np.nonzero(brick_min_abs(val, dims) < 0.3)[0].astype(np.uint32)


def brick_cell_mask(ids, dims):
    """(d, h, w) bool: the cells of the frame that lie in the bricks `ids`"""
    w, h, d = [int(v) for v in dims]
    nbx, nby, nbz = brick_grid(dims)
    listed = np.zeros(nbx * nby * nbz, bool)
    listed[np.asarray(ids).astype(np.int64)] = True
    m = np.repeat(np.repeat(np.repeat(listed.reshape(nbz, nby, nbx), 8, 0), 8, 1), 8, 2)
    return m[:d, :h, :w]


# ---- the scenes on the CPU oracle -------------------------------------------------------------------------------------------------

def oracle_volume(oracle, case):
    """the scene's volume on the host (oracle.Volume): the sphere, case C's unobserved cells"""
    c = CASES[case]
    vol = oracle.Volume(*c["dims"], *box(c["dims"]))
    oracle.sdf_sphere(vol, c["center"], c["r"])
    if c.get("nan7"):
        vol.data[..., 0][nan7_mask(c["dims"])] = np.nan
    return vol


def oracle_dense(oracle, case, vol, ids):
    """the comparator D on the host: NaN, then the bricks `ids` of vol"""
    c = CASES[case]
    D = oracle.Volume(*c["dims"], *box(c["dims"]))
    oracle.sdf_reset(D, NAN)
    m = brick_cell_mask(ids, c["dims"])
    D.data[m] = vol.data[m]
    return D


def oracle_render(oracle, case, D, subpix=True):
    """(depth, normals, shade, stats) of oracle.raycast_sdf on D at the case's camera"""
    c = CASES[case]
    w, h = c["size"]
    d, n, i = oracle.Image(w, h), oracle.Image(w, h, channels=4), oracle.Image(w, h)
    st = oracle.raycast_sdf(d, n, i, D, pose(case), intrinsics(case), NEAR, c["far"], TRUNC, subpix, nthreads=0)
    return d.data.copy(), n.data.copy(), i.data.copy(), st


def differing_pixels(a, b):
    """pixels whose depth or normal bits differ between two renderings (depth, normals, ...)"""
    dd = a[0].view(np.int32) != b[0].view(np.int32)
    dn = np.any(a[1].view(np.int32) != b[1].view(np.int32), axis=-1)
    return int(np.count_nonzero(dd | dn))
