"""The kept set of the tracked SdfFuse (KFX_FUSE_KEEP_MB, fuse.hip): the workgroups of every stride-th row of y-bricks -- 8 voxel
rows, counted in the parent volume -- read their cells with ordinary loads so that the lines stay in the memory-side cache;
stride = ceil(volume bytes / kept bytes).  Which loads a brick uses must never show in the results:
  * the tracked volume equals the untracked one bit for bit after four orbit frames (both sweep directions), and the summary
    stays conservative, with all, a quarter and none of the rows kept, on a ragged volume and on a view that starts at 8 cells;
  * the set is a function of the parent's rows alone: the same in every launch, and in a view the rows of the parent.
The knob is read once per process, so every case runs in a fresh child process."""
import json
import os
import subprocess
import sys

import pytest

import kfx_testlib as T

pytestmark = pytest.mark.gpu

CHILD = r'''
import ctypes as C, json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import kfx_testlib as T
from kfx_testlib import scenes
from kangaroo_amd import roo, _lib
from test_gpu_summary import export, check_conservative

case = json.loads(sys.argv[1])
dims, w, h, view = tuple(case["dims"]), case["w"], case["h"], case["view"]
keep = _lib.load_debug().kfx_debug_fuse_keep
keep.restype, keep.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_ubyte), C.c_int]
bmin, bmax, near, far = scenes.SCENES["room"]
K = scenes.intrinsics(w, h)
tr = scenes.trunc_dist(bmin, bmax, dims)
roo.set_math_mode("fast")
va, vb = roo.BoundedVolume(*dims, bmin, bmax), roo.BoundedVolume(*dims, bmin, bmax)
summ = roo.SdfSummary(vb)
roo.SdfReset(va, float("nan"))
roo.SdfReset(vb, float("nan"), summary=summ)
wa, wb = (va.SubVolume(*view), vb.SubVolume(*view)) if view else (va, vb)
f, vbo, nrm = roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h, "f32x4")
n_rows = -(-dims[1] // 8)
launches = []
for i in range(4):
    T_wc = scenes.orbit_pose(i, 30)
    roo.BilateralFilter(f, T.upload_image(roo, scenes.render_depth("room", w, h, T_wc, K)), **scenes.BILATERAL)
    roo.DepthToVbo(vbo, f, K)
    roo.NormalsFromVbo(nrm, vbo)
    T_cw = scenes.se3_inverse(T_wc)
    roo.SdfFuse(wa, f, nrm, T_cw, K, tr, scenes.MAX_W, scenes.MIN_COS_THETA)
    roo.SdfFuse(wb, f, nrm, T_cw, K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, summary=summ)
    out, kept = (C.c_int * 3)(), (C.c_ubyte * n_rows)()
    assert keep(summ.handle, out, kept, n_rows) == 0
    launches.append({"stride": out[0], "row0": out[1], "rows": out[2], "kept": [r for r in range(n_rows) if kept[r]]})
a, b = va.MemcpyToHost(), vb.MemcpyToHost()
assert np.isfinite(b[..., 0]).any(), "nothing was fused"
assert T.nan_equal(a, b), "the tracked volume differs from the untracked one"
R, classes = export(roo, summ, 1e-5, tr, fine_shift=4)
check_conservative(vb, R)
print("RESULT " + json.dumps({"launches": launches, "volume_bytes": int(vb.img_pitch) * dims[2]}))
'''


def run_case(keep_mb, dims, w, h, view=None):
    code = CHILD % (T.ROOT, os.path.join(T.ROOT, "tests"))
    env = dict(os.environ)
    env["KFX_FUSE_KEEP_MB"] = str(keep_mb)
    case = {"dims": dims, "w": w, "h": h, "view": view}
    out = subprocess.run([sys.executable, "-c", code, json.dumps(case)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
    assert lines, out.stdout + out.stderr
    return json.loads(lines[-1][7:])


def check_kept_set(res, keep_mb, first_row, rows):
    """Every launch decided the same: the stride of the budget, and of the rows it covered those the parent's index selects."""
    budget = keep_mb << 20
    stride = -(-res["volume_bytes"] // budget) if keep_mb else 0
    want = {"stride": stride, "row0": first_row, "rows": rows,
            "kept": [r for r in range(first_row, first_row + rows) if stride and r % stride == 0]}
    assert res["launches"][0] == want, (res["launches"][0], want)
    for a, b in zip(res["launches"], res["launches"][1:]):
        assert a == b, "the kept set changed between two consecutive launches: %r / %r" % (a, b)
    return want


@pytest.mark.parametrize("keep_mb,n_kept", [(4, 4), (16, 16), (0, 0)])
def test_gpu_keep_quarter_all_and_none_of_the_rows(keep_mb, n_kept):
    """128^3 (16 MiB, sixteen rows of y-bricks): 4 MB keeps every fourth row, 16 MB all of them, 0 none."""
    res = run_case(keep_mb, (128, 128, 128), 160, 120)
    assert res["volume_bytes"] == 16 << 20
    want = check_kept_set(res, keep_mb, 0, 16)
    assert len(want["kept"]) == n_kept and want["stride"] == {4: 4, 16: 1, 0: 0}[keep_mb]


def test_gpu_keep_on_a_ragged_volume():
    """(100, 84, 92): the extents 96 x 80 x 88 end inside an x-brick and inside a z-layer; ten rows of y-bricks are launched."""
    res = run_case(2, (100, 84, 92), 200, 150)
    want = check_kept_set(res, 2, 0, 10)
    assert want["stride"] >= 3 and 0 < len(want["kept"]) < 10   # (6.2 MB of cells, more with a padded pitch, against 2 MB)


def test_gpu_keep_follows_the_parent_rows_in_a_view():
    """A view of a 128^3 parent from (8, 8, 8) -- z a multiple of 8, not of 16: its first row of y-bricks is the parent's row 1,
    so the kept rows are the parent's 4, 8 and 12 (the view's own 3, 7 and 11), not the view's own multiples of four."""
    res = run_case(4, (128, 128, 128), 160, 120, view=[[8, 8, 8], [112, 112, 112]])
    want = check_kept_set(res, 4, 1, 14)
    assert want["kept"] == [4, 8, 12]
