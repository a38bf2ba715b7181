"""The brick summary of half-cell volumes (kfx_sdf_summary_create_h and the _h tracked calls, include/kfx_summary_h.h), and the
global-table mode of the class-table march (fp32 and half).
  * tracking never changes the half volume; the summary covers its contents; the class tables hold against them with
    vref = (half) trunc and KFX_SUMMARY_HALF_BAND;
  * exact numerics: tracked images bit-identical to kfx_raycast_sdf_h and to the oracle; fast: within the fast tolerances;
  * rebuild, views, invalidate, reset; kind mismatches are refused;
  * global-table mode: the same images and counts as the LDS tables, with only the two top levels staged."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import oracle, scenes
from test_gpu_summary import export

pytestmark = pytest.mark.gpu


def band():
    for line in open(os.path.join(T.ROOT, "include", "kfx_summary_h.h")):
        if line.startswith("#define KFX_SUMMARY_HALF_BAND"):
            return float(line.split()[2].rstrip("f"))
    raise AssertionError("KFX_SUMMARY_HALF_BAND")


def vref_of(tr):
    return float(np.float16(np.float32(tr)))


def check_classes(vol, classes, tol, vref):
    """Class 1 / 2 / 3 entries hold -- in their cells and the +1 cells -- only vref (within tol) / NaN / either, in the half volume."""
    import torch
    import torch.nn.functional as F
    v = vol.tensor()[..., 0].float()
    d, h, w = v.shape
    flags = {1: (v - vref).abs() <= tol * vref, 2: torch.isnan(v)}
    flags[3] = flags[1] | flags[2]
    out = {}
    for shift, cls in classes.items():
        m = 1 << shift
        nz, ny, nx = cls.shape
        for k, fl in flags.items():
            bad = F.pad((~fl).float()[None, None], (0, nx * m + 1 - w, 0, ny * m + 1 - h, 0, nz * m + 1 - d), value=0.0)
            holds = F.max_pool3d(bad, kernel_size=m + 1, stride=m)[0, 0] == 0
            wrong = (cls == k) & ~holds
            assert not bool(wrong.any()), "class %d entries of the 2^%d level that the volume contradicts: %d" % (k, shift, int(wrong.sum()))
        out[shift] = {k: int((cls == k).sum()) for k in range(4)}
    return out


def check_conservative(vol, R):
    import torch
    v = vol.tensor()[..., 0].float()
    d, h, w = v.shape
    nbz, nby, nbx = R.shape[:3]
    pad = torch.full((nbz * 8, nby * 8, nbx * 8), float("nan"), device=v.device)
    known = torch.zeros_like(pad, dtype=torch.bool)
    pad[:d, :h, :w] = v
    known[:d, :h, :w] = True
    br = pad.view(nbz, 8, nby, 8, nbx, 8).permute(0, 2, 4, 1, 3, 5).reshape(nbz, nby, nbx, 512)
    kn = known.view(nbz, 8, nby, 8, nbx, 8).permute(0, 2, 4, 1, 3, 5).reshape(nbz, nby, nbx, 512)
    has = ~torch.isnan(br) & kn
    isn = torch.isnan(br) & kn
    tmin = torch.where(has, br, torch.full_like(br, float("inf"))).amin(-1)
    tmax = torch.where(has, br, torch.full_like(br, float("-inf"))).amax(-1)
    state = R[..., 2].contiguous().view(torch.int32)
    assert not bool(((state == 1) & has.any(-1)).any()), "brick marked all-NaN holds values"
    assert not bool(((state == 0) & isn.any(-1)).any()), "brick marked all-values holds NaN"
    for s in (state == 0, (state == 2) & has.any(-1)):
        assert bool((R[..., 0][s] <= tmin[s]).all()) and bool((R[..., 1][s] >= tmax[s]).all()), "range does not cover the brick"
    return dict(uniform=int((state == 0).sum()), all_nan=int((state == 1).sum()), mixed=int((state == 2).sum()))


def check_rebuild_exact(vol, R):
    """kfx_sdf_summary_rebuild: every brick's state and the exact lo / hi of its valued cells (cells beyond the volume do not count)."""
    import torch
    v = vol.tensor()[..., 0].float()
    d, h, w = v.shape
    nbz, nby, nbx = R.shape[:3]
    pad = torch.full((nbz * 8, nby * 8, nbx * 8), float("nan"), device=v.device)
    known = torch.zeros_like(pad, dtype=torch.bool)
    pad[:d, :h, :w] = v
    known[:d, :h, :w] = True
    br = pad.view(nbz, 8, nby, 8, nbx, 8).permute(0, 2, 4, 1, 3, 5).reshape(nbz, nby, nbx, 512)
    kn = known.view(nbz, 8, nby, 8, nbx, 8).permute(0, 2, 4, 1, 3, 5).reshape(nbz, nby, nbx, 512)
    has = ~torch.isnan(br) & kn
    nan = torch.isnan(br) & kn
    want = torch.where(has.any(-1), torch.where(nan.any(-1), 2, 0), 1)
    assert bool((R[..., 2].contiguous().view(torch.int32) == want).all()), "rebuilt states"
    some = has.any(-1)
    lo = torch.where(has, br, torch.full_like(br, float("inf"))).amin(-1)
    hi = torch.where(has, br, torch.full_like(br, float("-inf"))).amax(-1)
    assert bool((R[..., 0][some] == lo[some]).all()) and bool((R[..., 1][some] == hi[some]).all()), "rebuilt ranges"
    assert int(some.sum()) > 0 and int((~some).sum()) > 0


def fast_close(a, b, w, h, normal_tol=2e-3):
    da, db = a[0].MemcpyToHost(), b[0].MemcpyToHost()
    na, nb = a[1].MemcpyToHost(), b[1].MemcpyToHost()
    hit_a, hit_b = np.isfinite(da), np.isfinite(db)
    flips = int((hit_a != hit_b).sum())
    assert flips <= max(3, 2e-4 * w * h), flips
    both = hit_a & hit_b
    assert both.sum() > 0.03 * w * h
    assert np.abs(da[both] - db[both]).max() < 1e-4, np.abs(da[both] - db[both]).max()
    cosang = np.clip(np.sum(na[both][:, :3].astype(np.float64) * nb[both][:, :3], axis=1), -1, 1)
    assert np.arccos(cosang).max() < normal_tol, np.arccos(cosang).max()


def images(roo, w, h):
    return [roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h)]


def bit_equal(a, b):
    return all(T.nan_equal(x.MemcpyToHost(), y.MemcpyToHost()) for x, y in zip(a, b))


def frame_inputs(roo, scene, w, h, K, i, n=30):
    T_wc = scenes.orbit_pose(i, n)
    f, vbo, nrm = roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h, "f32x4")
    roo.BilateralFilter(f, T.upload_image(roo, scenes.render_depth(scene, w, h, T_wc, K)), **scenes.BILATERAL)
    roo.DepthToVbo(vbo, f, K)
    roo.NormalsFromVbo(nrm, vbo)
    return T_wc, f, nrm


@pytest.mark.parametrize("scene,N,w,h,dims", [("room", 128, 320, 240, None), ("full", 96, 160, 120, None), ("room", 0, 200, 150, (100, 84, 92))])
@pytest.mark.parametrize("math", ["exact", "fast"])
def test_gpu_half_tracked_fuse_and_raycast(roo, scene, N, w, h, dims, math):
    dims = dims or (N, N, N)
    bmin, bmax, near, far = scenes.SCENES[scene]
    K = scenes.intrinsics(w, h)
    tr = scenes.trunc_dist(bmin, bmax, dims)
    vref, tol = vref_of(tr), (band() if math == "fast" else 0.0)
    prev = roo.set_math_mode(math)
    try:
        va, vb = roo.BoundedVolume(*dims, bmin, bmax, kind="f16"), roo.BoundedVolume(*dims, bmin, bmax, kind="f16")
        summ = roo.SdfSummary(vb)
        roo.SdfReset(va, float("nan"))
        roo.SdfReset(vb, float("nan"), summary=summ)
        ovol = oracle.VolumeH(*dims, bmin, bmax)
        oracle.sdf_reset(ovol, float("nan"))
        for i in range(4):
            T_wc, f, nrm = frame_inputs(roo, scene, w, h, K, i)
            T_cw = scenes.se3_inverse(T_wc)
            roo.SdfFuse(va, f, nrm, T_cw, K, tr, scenes.MAX_W, scenes.MIN_COS_THETA)
            roo.SdfFuse(vb, f, nrm, T_cw, K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, summary=summ)
            assert T.nan_equal(va.MemcpyToHost(), vb.MemcpyToHost())          # tracking only observes
            R, classes = export(roo, summ, tol, vref, fine_shift=4)
            check_conservative(vb, R)
            counts = check_classes(vb, classes, tol, vref)
            a, b = images(roo, w, h), images(roo, w, h)
            roo.set_math_mode("exact")
            roo.RaycastSdf(*a, va, T_wc, K, near, far, tr, True)                # the plain half march
            roo.set_math_mode(math)
            roo.RaycastSdf(*b, vb, T_wc, K, near, far, tr, True, summary=summ)
            if math == "exact":
                assert bit_equal(a, b)
                # and the oracle's half march on the same cells
                ovol.data[...] = vb.MemcpyToHost()
                od, on, oi = oracle.Image(w, h), oracle.Image(w, h, channels=4), oracle.Image(w, h)
                oracle.raycast_sdf(od, on, oi, ovol, T_wc, K, near, far, tr, True)
                assert T.nan_equal(od.data, b[0].MemcpyToHost()) and T.nan_equal(oi.data, b[2].MemcpyToHost())
                if i == 0:
                    assert sum(counts[4][k] for k in (1, 2, 3)) > 0, counts
            else:
                fast_close(a, b, w, h)
    finally:
        roo.set_math_mode(prev)


def _fused_half(roo, scene, N, w, h, frames, math="exact", summ=True, n=30):
    bmin, bmax, near, far = scenes.SCENES[scene]
    K = scenes.intrinsics(w, h)
    tr = scenes.trunc_dist(bmin, bmax, (N, N, N))
    vol = roo.BoundedVolume(N, N, N, bmin, bmax, kind="f16")
    s = roo.SdfSummary(vol) if summ else None
    roo.SdfReset(vol, float("nan"), summary=s)
    prev = roo.set_math_mode(math)
    try:
        for i in range(frames):
            T_wc, f, nrm = frame_inputs(roo, scene, w, h, K, i, n)
            roo.SdfFuse(vol, f, nrm, scenes.se3_inverse(T_wc), K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, summary=s)
    finally:
        roo.set_math_mode(prev)
    return vol, s, K, tr, T_wc, near, far


def test_gpu_half_rebuild_views_invalidate_and_reset(roo):
    import torch
    vol, summ, K, tr, T_wc, near, far = _fused_half(roo, "room", 96, 160, 120, 2)
    R0, _ = export(roo, summ, 0.0, vref_of(tr))
    summ.rebuild()
    R1, _ = export(roo, summ, 0.0, vref_of(tr))
    check_conservative(vol, R1)
    check_rebuild_exact(vol, R1)
    # a ragged parent (90 x 84 x 92: the last bricks along every axis are cut, x takes the per-cell path of the rebuild kernel)
    bmin, bmax, _, _ = scenes.SCENES["room"]
    vu = roo.BoundedVolume(90, 84, 92, bmin, bmax, kind="f16")
    su = roo.SdfSummary(vu)
    roo.SdfReset(vu, float("nan"))
    roo.SdfSphere(vu, (0.0, 0.0, 2.0), 0.5)
    su.rebuild()
    check_rebuild_exact(vu, export(roo, su, 0.0, 1.0)[0])
    # a parent whose row pitch is not a multiple of 16 bytes (4 B cells, 90 per row, pitch 364 B): every row takes the per-cell path
    vp = roo.BoundedVolume(90, 40, 48, bmin, bmax, kind="f16", pitch=364)
    sp = roo.SdfSummary(vp)
    roo.SdfReset(vp, float("nan"))
    roo.SdfSphere(vp, (0.0, 0.0, 2.0), 0.5)
    sp.rebuild()
    check_rebuild_exact(vp, export(roo, sp, 0.0, 1.0)[0])
    # a view at multiples of 8 cells tracks: the summary keeps covering the parent volume
    sub = vol.SubVolume((8, 16, 8), (64, 64, 64))
    T_wc2, f, nrm = frame_inputs(roo, "room", 160, 120, K, 3)
    roo.SdfFuse(sub, f, nrm, scenes.se3_inverse(T_wc2), K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, summary=summ)
    check_conservative(vol, export(roo, summ, 0.0, vref_of(tr))[0])
    # untracked writer + invalidate(): every brick unknown, images still equal
    roo.SdfSphere(vol, (0.0, 0.0, 2.0), 0.3)
    summ.invalidate()
    Ri, _ = export(roo, summ, 0.0, vref_of(tr))
    assert bool((Ri[..., 2].contiguous().view(torch.int32) == 2).all())
    a, b = images(roo, 160, 120), images(roo, 160, 120)
    roo.RaycastSdf(*a, vol, T_wc, K, near, far, tr, True)
    roo.RaycastSdf(*b, vol, T_wc, K, near, far, tr, True, summary=summ)
    assert bit_equal(a, b)
    # reset_tracked_h: every brick {vref, vref, state 0}
    roo.SdfReset(vol, tr, summary=summ)
    Rr, _ = export(roo, summ, 0.0, vref_of(tr))
    assert bool((Rr[..., 0] == vref_of(tr)).all()) and bool((Rr[..., 1] == vref_of(tr)).all())
    assert bool((Rr[..., 2].contiguous().view(torch.int32) == 0).all())
    check_conservative(vol, Rr)


def test_gpu_summary_kind_mismatch_is_refused(roo):
    from kangaroo_amd._lib import KfxError
    bmin, bmax, near, far = scenes.SCENES["room"]
    w, h = 160, 120
    K = scenes.intrinsics(w, h)
    tr = scenes.trunc_dist(bmin, bmax, (64, 64, 64))
    v16, v32 = roo.BoundedVolume(64, 64, 64, bmin, bmax, kind="f16"), roo.BoundedVolume(64, 64, 64, bmin, bmax)
    s16, s32 = roo.SdfSummary(v16), roo.SdfSummary(v32)
    roo.SdfReset(v16, float("nan"), summary=s16)
    roo.SdfReset(v32, float("nan"), summary=s32)
    T_wc, f, nrm = frame_inputs(roo, "room", w, h, K, 0)
    T_cw = scenes.se3_inverse(T_wc)
    roo.SdfFuse(v16, f, nrm, T_cw, K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, summary=s16)
    roo.SdfFuse(v32, f, nrm, T_cw, K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, summary=s32)
    before16, before32 = v16.MemcpyToHost(), v32.MemcpyToHost()
    img = images(roo, w, h)
    for x in img:
        x.storage.fill_(7)
    for vol, s in ((v16, s32), (v32, s16)):
        for call in (lambda: roo.SdfFuse(vol, f, nrm, T_cw, K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, summary=s),
                     lambda: roo.RaycastSdf(*img, vol, T_wc, K, near, far, tr, True, summary=s),
                     lambda: roo.RaycastSdfCount(vol, w, h, T_wc, K, near, far, tr, summary=s),
                     lambda: roo.RaycastSdfLevels([tuple(img)], vol, T_wc, [K], near, far, tr, True, summary=s),
                     lambda: roo.SdfReset(vol, tr, summary=s)):
            with pytest.raises(KfxError) as e:
                call()
            assert e.value.code == -2, str(e.value)   # KFX_E_SHAPE
    assert T.nan_equal(v16.MemcpyToHost(), before16) and T.nan_equal(v32.MemcpyToHost(), before32)
    assert all(bool((x.storage == 7).all()) for x in img)


@pytest.mark.parametrize("scene", ["room", "full"])
def test_gpu_half_long_fast_stream_keeps_free_space(roo, scene):
    """~600 fast-mode frames at 64^3: the free space the tables recognise at frame 60 is still class 1 at the end."""
    N, w, h = 64, 160, 120
    bmin, bmax, near, far = scenes.SCENES[scene]
    K = scenes.intrinsics(w, h)
    tr = scenes.trunc_dist(bmin, bmax, (N, N, N))
    vref, tol = vref_of(tr), band()
    vol = roo.BoundedVolume(N, N, N, bmin, bmax, kind="f16")
    summ = roo.SdfSummary(vol)
    roo.SdfReset(vol, float("nan"), summary=summ)
    prev = roo.set_math_mode("fast")
    try:
        frames = []
        for i in range(120):
            T_wc, f, nrm = frame_inputs(roo, scene, w, h, K, i, 120)
            frames.append((scenes.se3_inverse(T_wc), f, nrm))
        free60 = None
        for i in range(600):
            T_cw, f, nrm = frames[i % 120]
            roo.SdfFuse(vol, f, nrm, T_cw, K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, summary=summ)
            if i + 1 == 60:
                free60 = export(roo, summ, tol, vref, fine_shift=3)[1][3] == 1
        R, classes = export(roo, summ, tol, vref, fine_shift=3)
        check_classes(vol, classes, tol, vref)
        kept = classes[3][free60] == 1
        assert int(free60.sum()) > 0
        assert bool(kept.all()), "free entries of frame 60 that left class 1 by frame 600: %d of %d" % (int((~kept).sum()), int(free60.sum()))
    finally:
        roo.set_math_mode(prev)


_GLOBAL_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import numpy as np, torch
import kfx_testlib as T
from kfx_testlib import scenes
from kangaroo_amd import roo
kind, math = sys.argv[2], sys.argv[3]
N, w, h, scene = 256, 320, 240, 'full'
bmin, bmax, near, far = scenes.SCENES[scene]
K = scenes.intrinsics(w, h)
tr = scenes.trunc_dist(bmin, bmax, (N, N, N))
vol = roo.BoundedVolume(N, N, N, bmin, bmax, kind=kind)
s = roo.SdfSummary(vol)
roo.SdfReset(vol, float('nan'), summary=s)
roo.set_math_mode(math)
for i in range(2):
    T_wc = scenes.orbit_pose(i, 30)
    f, vbo, nrm = roo.Image(w, h), roo.Image(w, h, 'f32x4'), roo.Image(w, h, 'f32x4')
    roo.BilateralFilter(f, T.upload_image(roo, scenes.render_depth(scene, w, h, T_wc, K)), **scenes.BILATERAL)
    roo.DepthToVbo(vbo, f, K); roo.NormalsFromVbo(nrm, vbo)
    roo.SdfFuse(vol, f, nrm, scenes.se3_inverse(T_wc), K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, summary=s)
img = [roo.Image(w, h), roo.Image(w, h, 'f32x4'), roo.Image(w, h)]
roo.RaycastSdf(*img, vol, T_wc, K, near, far, tr, True, summary=s)
c = roo.RaycastSdfCount(vol, w, h, T_wc, K, near, far, tr, summary=s)
torch.cuda.synchronize()
np.savez(sys.argv[4], d=img[0].MemcpyToHost(), n=img[1].MemcpyToHost(), i=img[2].MemcpyToHost())
print(json.dumps(c))
"""


@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("math", ["exact", "fast"])
def test_gpu_global_table_mode_matches_lds_tables(roo, kind, math, tmp_path):
    """KFX_RAYCAST_GLOBAL_TABLES=1 at 256^3 (where the LDS tables fit): same images and counts, smaller staged bytes."""
    out = {}
    for mode in ("lds", "global"):
        # (KFX_RAYCAST_CLASS_KB=4: the LDS mode then stages the 16^3-cell fine level the global mode uses -- the same tables)
        env = dict(os.environ, KFX_RAYCAST_SUMMARY="1", KFX_RAYCAST_CLASS_KB="4")
        if mode == "global":
            env["KFX_RAYCAST_GLOBAL_TABLES"] = "1"
        path = str(tmp_path / (mode + ".npz"))
        r = subprocess.run([sys.executable, "-c", _GLOBAL_CHILD, T.ROOT, kind, math, path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        out[mode] = (json.loads(r.stdout.strip().splitlines()[-1]), np.load(path))
    (cl, il), (cg, ig) = out["lds"], out["global"]
    for k in ("d", "n", "i"):
        assert T.nan_equal(il[k], ig[k]), k
    assert cl["samples"] == cg["samples"] and cl["lookups"] == cg["lookups"] and cl["hits"] == cg["hits"], (cl, cg)
    assert cl["lookups"] > 0 and 0 < cg["table_bytes"] < cl["table_bytes"], (cl, cg)


_C5_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import numpy as np, torch
import kfx_testlib as T
from kfx_testlib import scenes
from kangaroo_amd import roo
math, frames = sys.argv[2], int(sys.argv[3])
N, w, h, scene = 2048, 320, 240, 'room'
bmin, bmax, near, far = scenes.SCENES[scene]
K = scenes.intrinsics(w, h)
tr = scenes.trunc_dist(bmin, bmax, (N, N, N))
vol = roo.BoundedVolume(N, N, N, bmin, bmax, kind='f16')
s = roo.SdfSummary(vol)
roo.SdfReset(vol, float('nan'), summary=s)
roo.set_math_mode(math)
for i in range(frames):
    T_wc = scenes.orbit_pose(i, 30)
    f, vbo, nrm = roo.Image(w, h), roo.Image(w, h, 'f32x4'), roo.Image(w, h, 'f32x4')
    roo.BilateralFilter(f, T.upload_image(roo, scenes.render_depth(scene, w, h, T_wc, K)), **scenes.BILATERAL)
    roo.DepthToVbo(vbo, f, K); roo.NormalsFromVbo(nrm, vbo)
    roo.SdfFuse(vol, f, nrm, scenes.se3_inverse(T_wc), K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, summary=s)
a = [roo.Image(w, h), roo.Image(w, h, 'f32x4'), roo.Image(w, h)]
b = [roo.Image(w, h), roo.Image(w, h, 'f32x4'), roo.Image(w, h)]
roo.RaycastSdf(*a, vol, T_wc, K, near, far, tr, True)
roo.RaycastSdf(*b, vol, T_wc, K, near, far, tr, True, summary=s)
ct = roo.RaycastSdfCount(vol, w, h, T_wc, K, near, far, tr, summary=s)
cp = roo.RaycastSdfCount(vol, w, h, T_wc, K, near, far, tr)
torch.cuda.synchronize()
np.savez(sys.argv[4], ad=a[0].MemcpyToHost(), an=a[1].MemcpyToHost(), ai=a[2].MemcpyToHost(), bd=b[0].MemcpyToHost(), bn=b[1].MemcpyToHost(), bi=b[2].MemcpyToHost())
print(json.dumps(dict(tracked=ct, plain=cp)))
"""


@pytest.mark.parametrize("math,frames", [("exact", 1), ("fast", 3)])
def test_gpu_c5_2048_half_tracked_raycast(roo, math, frames, tmp_path):
    """2048^3 half cells (C5, 32 GiB), tracked, KFX_RAYCAST_SUMMARY=1: the global-table march against the plain half march in the
    same numerics.  Fast: the difference is the table march's own -- runs through the wide half band (KFX_SUMMARY_HALF_BAND) place
    the samples near a surface differently from the plain march, and the normal of 2.4 mm half cells follows its stencil's base
    cell: 2.01e-3 rad at one pixel of 60 676 (depth within the usual 1e-4 m).  The normal limit is 4e-3 here, 2e-3 elsewhere."""
    import torch
    if torch.cuda.get_device_properties(0).total_memory < 24 << 30:
        pytest.skip("needs a 2048^3 half volume")
    path = str(tmp_path / "c5.npz")
    env = dict(os.environ, KFX_RAYCAST_SUMMARY="1")
    r = subprocess.run([sys.executable, "-c", _C5_CHILD, T.ROOT, math, str(frames), path], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    c = json.loads(r.stdout.strip().splitlines()[-1])
    z = np.load(path)
    if math == "exact":
        for k in ("d", "n", "i"):
            assert T.nan_equal(z["a" + k], z["b" + k]), k
    else:
        class Img:
            def __init__(self, x): self.x = x
            def MemcpyToHost(self): return self.x
        fast_close([Img(z["ad"]), Img(z["an"])], [Img(z["bd"]), Img(z["bn"])], 320, 240, normal_tol=4e-3)
    ratio = c["tracked"]["samples"] / max(c["plain"]["samples"], 1)
    assert c["tracked"]["lookups"] > 0 and c["tracked"]["samples"] < c["plain"]["samples"], "sample ratio %.3f: %s" % (ratio, c)
    print("C5 %s: samples tracked / plain = %.3f (%s)" % (math, ratio, c))


@pytest.mark.parametrize("scene", ["room", "full"])
def test_gpu_half_tracked_levels(roo, scene):
    N, w, h = 128, 320, 240
    vol, summ, K, tr, T_wc, near, far = _fused_half(roo, scene, N, w, h, 2)
    levels = [0, 2, 3]
    Ks = [scenes.intrinsics_level(K, l) for l in levels]
    one = [images(roo, w >> l, h >> l) + [roo.Image(w >> l, h >> l, "f32x4")] for l in levels]
    prev = roo.set_math_mode("exact")
    try:
        roo.RaycastSdfLevels([tuple(o) for o in one], vol, T_wc, Ks, near, far, tr, True, summary=summ)
        for l, Kl, o in zip(levels, Ks, one):
            p = images(roo, w >> l, h >> l)
            roo.RaycastSdf(*p, vol, T_wc, Kl, near, far, tr, True)
            assert bit_equal(p, o[:3]), l
    finally:
        roo.set_math_mode(prev)


def test_gpu_frame_pipeline_half_tracked(roo):
    from kangaroo_amd import pipeline
    N, w, h = 96, 160, 120
    bmin, bmax, near, far = scenes.SCENES["room"]
    K = scenes.intrinsics(w, h)
    prev = roo.set_math_mode("exact")
    try:
        pa = pipeline.FramePipeline(roo, (N, N, N), bmin, bmax, w, h, near=near, far=far, kind="f16", track=True)
        pb = pipeline.FramePipeline(roo, (N, N, N), bmin, bmax, w, h, near=near, far=far, kind="f16", track=False)
        assert pa.vol.kind == "f16" and pa.summary is not None and pa.kframe is None
        for i in range(10):
            T_wc = scenes.orbit_pose(i, 30)
            raw = scenes.render_depth("room", w, h, T_wc, K)
            for p in (pa, pb):
                p.raw.MemcpyFromHost(raw)
                p.step(T_wc)
            assert T.nan_equal(pa.vol.MemcpyToHost(), pb.vol.MemcpyToHost())
            for x, y in ((pa.ray_d, pb.ray_d), (pa.ray_n, pb.ray_n), (pa.ray_i, pb.ray_i)):
                assert T.nan_equal(x.MemcpyToHost(), y.MemcpyToHost()), i
    finally:
        roo.set_math_mode(prev)
    with pytest.raises(ValueError):
        pipeline.FramePipeline(roo, (N, N, N), bmin, bmax, w, h, kind="f16", track="auto")
