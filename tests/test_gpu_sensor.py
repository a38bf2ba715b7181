"""The sensor input path (include/kfx_sensor.h) on the GPU: every comparison is bit for bit, because both sides run the same
arithmetic -- s * raw + offset (one __device__ function) and the bilateral window of kfx_bilateral_f32.

  * kfx_bilateral_depth against ElementwiseScaleBias followed by BilateralFilter(minval 0.2): u16 and f32 sensor images, both
    numerics modes, the fast / LDS / global kernels, a padded pitch, an output smaller than the input, no metres image;
  * the same under every KFX_BILATERAL_TILE (read once per process: one fresh interpreter per value);
  * the upload ring: order, slot reuse with and without synchronisation in between, "ring full", the pending count;
  * kfx_frame_step fed by the ring against the separate operators; FramePipeline / TrackingPipeline(sensor="u16") against the
    pipelines given the converted images."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import scenes

pytestmark = pytest.mark.gpu

W, H = 83, 61          # a multiple of no tile size: partial tiles on both edges, clamped aprons on all four
SCALE = 1e-3
BIL = scenes.BILATERAL
E_RANGE = -4
_CACHE = {}


def sensor_frame(k=0, w=W, h=H, pose=1):
    """(u16 millimetres, f32 millimetres) of a room depth: NaN -> 0 in u16 and kept in f32, a block of invalid pixels in the
    interior and one touching a corner, one saturated pixel; frame k is k mm further away"""
    key = (k, w, h, pose)
    if key not in _CACHE:
        K = scenes.intrinsics(w, h)
        d = np.array(scenes.render_depth("room", w, h, scenes.orbit_pose(pose, 8), K), np.float32)
        d[h // 3: h // 3 + 7, w // 3: w // 3 + 11] = np.nan
        d[:5, :6] = np.nan
        mm = np.float32(1000.0) * d + np.float32(k)
        with np.errstate(invalid="ignore"):
            u16 = np.clip(np.rint(mm), 0, 65535)
        u16 = np.where(np.isnan(mm), 0, u16).astype(np.uint16)
        f32 = mm.astype(np.float32)
        u16[h - 3, 5], f32[h - 3, 5] = 65535, 65535.0
        _CACHE[key] = (u16, f32)
    return _CACHE[key]


def upload(roo, arr, pitch=None):
    kind = "u16" if arr.dtype == np.uint16 else "f32"
    return roo.Image(arr.shape[1], arr.shape[0], kind, pitch=pitch).MemcpyFromHost(arr)


def separate_calls(roo, raw, size, ow=None, oh=None):
    """ElementwiseScaleBias + BilateralFilter(minval): (filtered, metres) as numpy, filtered of ow x oh (default: the input's size)"""
    m = roo.Image(raw.w, raw.h)
    f = roo.Image(raw.w if ow is None else ow, raw.h if oh is None else oh)
    roo.ElementwiseScaleBias(m, raw, SCALE, 0.0)
    roo.BilateralFilter(f, m, BIL["gs"], BIL["gr"], size, BIL["minval"])
    return f.MemcpyToHost(), m.MemcpyToHost()


def check_kernel(roo, fmt, size, variant=None):
    arr = sensor_frame()[0 if fmt == "u16" else 1]
    elem = arr.dtype.itemsize
    raw = upload(roo, arr, pitch=(W * elem + 255) // 256 * 256 + 48 * elem if variant == "pitch" else None)
    ow, oh = (50, 37) if variant == "sub" else (W, H)
    f, m = roo.Image(ow, oh), (None if variant == "no_metres" else roo.Image(ow, oh))
    roo.BilateralFilterDepth(f, m, raw, SCALE, 0.0, BIL["gs"], BIL["gr"], size, BIL["minval"])
    rf, rm = separate_calls(roo, raw, size, ow, oh)
    got = f.MemcpyToHost()
    assert T.nan_equal(got, rf), (fmt, size, variant, T.mismatch_report(got, rf))
    if m is not None:
        assert T.nan_equal(m.MemcpyToHost(), rm[:oh, :ow]), (fmt, size, variant)
    # the comparison means something: valid and invalid pixels, and the saturated reading is in range
    assert 0.5 * got.size < np.isfinite(got).sum() < got.size
    return got


@pytest.mark.parametrize("size", [1, 3, 5, 17])
@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("fmt", ["u16", "f32"])
def test_gpu_bilateral_depth_equals_scale_bias_then_bilateral(roo, fmt, math, size):
    prev = roo.set_math_mode(math)
    try:
        check_kernel(roo, fmt, size)
    finally:
        roo.set_math_mode(prev)


@pytest.mark.parametrize("variant", ["pitch", "sub", "no_metres"])
def test_gpu_bilateral_depth_views(roo, variant):
    """a padded-pitch input; an output that is a sub-rectangle smaller than the input; no metres image"""
    for math in ("exact", "fast"):
        prev = roo.set_math_mode(math)
        try:
            for fmt in ("u16", "f32"):
                check_kernel(roo, fmt, 3, variant)
        finally:
            roo.set_math_mode(prev)


def test_gpu_scale_bias_u16_is_the_reference_expression(roo):
    u16 = sensor_frame()[0]
    out = roo.Image(W, H)
    roo.ElementwiseScaleBias(out, upload(roo, u16), SCALE, 0.25)
    want = (np.float32(SCALE) * u16.astype(np.float32)).astype(np.float32) + np.float32(0.25)   # no contraction: two roundings
    assert T.nan_equal(out.MemcpyToHost(), want)


def _tile_child():
    """Run in a fresh interpreter per KFX_BILATERAL_TILE: the LDS kernel's shapes (size 5 in both modes, 3 in exact mode).  Both sides
    of check_kernel's equality go through one dispatch, so a grid or an LDS size that is wrong for a shape would cancel there: plain
    BilateralFilter is also held against the oracle in exact numerics (test_gpu_bilateral_variants' inputs, comparison and tolerance)."""
    import torch
    from kangaroo_amd import roo
    from test_gpu_parity import check_bilateral_variant
    assert torch.cuda.is_available()
    for math in ("exact", "fast"):
        roo.set_math_mode(math)
        for fmt in ("u16", "f32"):
            for size in (3, 5):
                check_kernel(roo, fmt, size)
            check_kernel(roo, fmt, 5, "sub")
    roo.set_math_mode("exact")
    for kind, minval in (("f32", 0.2), ("u8", None)):
        for size in (3, 5):
            check_bilateral_variant(roo, kind, minval, size)
    print("tile child ok", os.environ.get("KFX_BILATERAL_TILE"))


def test_gpu_bilateral_depth_under_every_tile_shape(roo):
    for tile in range(6):
        env = dict(os.environ, KFX_BILATERAL_TILE=str(tile))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--tile-child"], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "tile child ok %d" % tile in out.stdout, (tile, out.stdout[-2000:] + out.stderr[-2000:])


def test_gpu_depth_input_ring_order_and_reuse(roo):
    import torch
    n = 7
    frames = [sensor_frame(k)[0] for k in range(n)]
    want = []
    for k in range(n):   # the stateless operator on frame k
        f, m = roo.Image(W, H), roo.Image(W, H)
        roo.BilateralFilterDepth(f, m, upload(roo, frames[k]), SCALE, 0.0, BIL["gs"], BIL["gr"], BIL["size"], BIL["minval"])
        want.append((f.MemcpyToHost(), m.MemcpyToHost()))
    assert not T.nan_equal(want[0][0], want[1][0])   # a stale or overwritten slot would show

    def filt(inp, f, m):
        inp.filter(f, m, BIL["gs"], BIL["gr"], BIL["size"], BIL["minval"])

    # pass A: frame k + 1 submitted before frame k is filtered; every result read back
    inp = roo.DepthInput(W, H, "u16", SCALE, 0.0, slots=2)
    assert inp.pending == 0
    with pytest.raises(roo.KfxError) as e:
        filt(inp, roo.Image(W, H), None)   # nothing pending
    assert e.value.code == E_RANGE
    f, m = roo.Image(W, H), roo.Image(W, H)
    buf = inp.acquire()
    assert buf.shape == (H, W) and buf.dtype == np.uint16
    buf[...] = frames[0]
    inp.submit()
    assert inp.pending == 1
    for k in range(n):
        if k + 1 < n:
            inp.submit(frames[k + 1])
        assert inp.pending == (2 if k + 1 < n else 1)
        if k == 2:   # two images pending in two slots: ring full, and nothing changes
            with pytest.raises(roo.KfxError) as e:
                inp.acquire()
            assert e.value.code == E_RANGE and inp.pending == 2
        filt(inp, f, m)
        assert inp.pending == (1 if k + 1 < n else 0)
        if k == 2:   # after one filter the third acquire succeeds (the next submit fills the same buffer)
            assert inp.acquire().shape == (H, W) and inp.pending == 1
        torch.cuda.synchronize()
        assert T.nan_equal(f.MemcpyToHost(), want[k][0]), k
        assert T.nan_equal(m.MemcpyToHost(), want[k][1]), k
    with pytest.raises(roo.KfxError):
        inp.submit()   # no acquired buffer

    # pass B: the same with no read-back and no synchronisation until the end
    inp = roo.DepthInput(W, H, "u16", SCALE, 0.0, slots=2)
    outs = [(roo.Image(W, H), roo.Image(W, H)) for _ in range(n)]
    inp.submit(frames[0])
    for k in range(n):
        if k + 1 < n:
            inp.submit(frames[k + 1])
        filt(inp, *outs[k])
    assert inp.pending == 0
    torch.cuda.synchronize()
    for k in range(n):
        assert T.nan_equal(outs[k][0].MemcpyToHost(), want[k][0]), k
        assert T.nan_equal(outs[k][1].MemcpyToHost(), want[k][1]), k
    # an f32 ring of three slots, filled before the first filter
    inp = roo.DepthInput(W, H, "f32", SCALE, 0.0, slots=3)
    for k in range(3):
        inp.submit(sensor_frame(k)[1])
    assert inp.pending == 3
    for k in range(3):
        filt(inp, f, m)
        rf, rm = separate_calls(roo, upload(roo, sensor_frame(k)[1]), BIL["size"])
        assert T.nan_equal(f.MemcpyToHost(), rf) and T.nan_equal(m.MemcpyToHost(), rm), k


@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("track", [False, True])
def test_gpu_frame_step_takes_its_image_from_the_ring(roo, math, track):
    """tests/test_gpu_frame.py's set-up at 64^3 and 83 x 61: five frames through Frame.set_input, submitted one frame ahead."""
    import torch
    N, n = 64, 5
    bmin, bmax, near, far = scenes.SCENES["room"]
    K = scenes.intrinsics(W, H)
    tr = scenes.trunc_dist(bmin, bmax, (N, N, N))
    frames = [sensor_frame(0, pose=i)[0] for i in range(n)]
    prev = roo.set_math_mode(math)
    try:
        va, vb = roo.BoundedVolume(N, N, N, bmin, bmax), roo.BoundedVolume(N, N, N, bmin, bmax)
        mk = lambda: [roo.Image(W, H), roo.Image(W, H), roo.Image(W, H, "f32x4"), roo.Image(W, H, "f32x4"), roo.Image(W, H), roo.Image(W, H, "f32x4"),
                      roo.Image(W, H)]   # metres, filtered, vbo, normals, ray depth / normals / image
        ia, ib = mk(), mk()
        fr = roo.Frame(vb, ib[0], ib[1], ib[2], ib[3], ib[4], ib[5], ib[6], K, BIL, near, far, tr, scenes.MAX_W, scenes.MIN_COS_THETA, timing_slots=16)
        inp = roo.DepthInput(W, H, "u16", SCALE, 0.0, slots=2)
        fr.set_input(inp)
        summ = roo.SdfSummary(va) if track else None
        roo.SdfReset(va, float("nan"), summary=summ)
        fr.set_track(track)
        fr.reset()
        kw = {"summary": summ} if track else {}
        inp.submit(frames[0])
        fr.reset()   # leaves the pending image pending
        assert inp.pending == 1
        for i in range(n):
            T_wc = scenes.orbit_pose(i, 30)
            if i + 1 < n:
                inp.submit(frames[i + 1])
            # the separate operators fed the quantised image
            roo.ElementwiseScaleBias(ia[0], upload(roo, frames[i]), SCALE, 0.0)
            roo.BilateralFilter(ia[1], ia[0], **BIL)
            roo.DepthToVbo(ia[2], ia[1], K)
            roo.NormalsFromVbo(ia[3], ia[2])
            roo.SdfFuse(va, ia[1], ia[3], scenes.se3_inverse(T_wc), K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, **kw)
            roo.RaycastSdf(ia[4], ia[5], ia[6], va, T_wc, K, near, far, tr, True, **kw)
            if i == 3:   # an explicit raw, or a step without the preprocess, leaves the ring alone
                before = inp.pending
                fr.step(T_wc, None, ia[0], fr.PREPROCESS)
                fr.step(T_wc, None, None, fr.RAYCAST)
                assert inp.pending == before
            fr.step(T_wc, scenes.se3_inverse(T_wc), None)
            assert inp.pending == (1 if i + 1 < n else 0)
            torch.cuda.synchronize()
            for j, (a, b) in enumerate(zip(ia, ib)):
                assert T.nan_equal(a.MemcpyToHost(), b.MemcpyToHost()), (i, j)
            assert T.nan_equal(va.MemcpyToHost(), vb.MemcpyToHost()), i
        with pytest.raises(roo.KfxError) as e:
            fr.step(scenes.orbit_pose(0, 30), None, None)   # nothing pending
        assert e.value.code == E_RANGE and fr.count == n + 2
        t = fr.timings(0, n + 2)
        assert t.shape == (n + 2, 5) and np.all(np.isfinite(t[:, :3])) and np.all(t[:, :3] >= 0)
        assert np.all(t[[0, 1, 2, 6], 0] > 0) and np.all(t[[0, 1, 2, 6], 1] > 0) and np.all(t[[0, 1, 2, 6], 2] > 0)
        fr.set_input(None)   # detached: a step without raw filters cfg.raw again
        fr.step(scenes.orbit_pose(0, 30), None, None, fr.PREPROCESS)
        torch.cuda.synchronize()
        assert T.nan_equal(ia[1].MemcpyToHost(), ib[1].MemcpyToHost())
    finally:
        roo.set_math_mode(prev)


def _metres(roo, u16):
    m = roo.Image(u16.shape[1], u16.shape[0])
    roo.ElementwiseScaleBias(m, upload(roo, u16), SCALE, 0.0)
    return m


@pytest.mark.parametrize("kw", [{}, {"color": True}], ids=["one-call frame", "separate operators (colour)"])
def test_gpu_frame_pipeline_with_a_sensor_equals_the_pipeline_given_metres(roo, kw):
    import torch
    from kangaroo_amd.pipeline import FramePipeline, SlabPipeline
    N, n = 64, 4
    bmin, bmax, near, far = scenes.SCENES["room"]
    a = FramePipeline(roo, (N, N, N), bmin, bmax, W, H, near=near, far=far, sensor="u16", sensor_scale=SCALE, sensor_slots=2, **kw)
    b = FramePipeline(roo, (N, N, N), bmin, bmax, W, H, near=near, far=far, **kw)
    assert (a.kframe is not None) == (not kw) and a.input is not None and b.input is None
    frames = [sensor_frame(0, pose=i)[0] for i in range(n)]
    a.submit(frames[0])
    for i in range(n):
        T_wc = scenes.orbit_pose(i, 30)
        if i + 1 < n:
            a.submit(frames[i + 1])
        a.step(T_wc)
        m = _metres(roo, frames[i])
        b.step(T_wc, m)
        torch.cuda.synchronize()
        assert T.nan_equal(a.raw.MemcpyToHost(), m.MemcpyToHost()), i
        for name in ("filtered", "vbo", "normals", "ray_d", "ray_n", "ray_i"):
            assert T.nan_equal(getattr(a, name).MemcpyToHost(), getattr(b, name).MemcpyToHost()), (i, name)
        assert T.nan_equal(a.vol.MemcpyToHost(), b.vol.MemcpyToHost()), i
    assert a.input.pending == 0
    with pytest.raises(ValueError, match="sensor"):
        SlabPipeline(roo, None, (N, N, N), bmin, bmax, W, H, sensor="u16")


def test_gpu_tracking_pipeline_with_a_sensor_equals_the_pipeline_given_metres(roo):
    from kangaroo_amd.pipeline import FROM_SENSOR, TrackingPipeline
    N, w, h, n = 64, 160, 120, 4
    bmin, bmax, near, far = scenes.SCENES["room"]
    K = scenes.intrinsics(w, h)
    frames = []
    for i in range(n):
        d = scenes.render_depth("room", w, h, scenes.orbit_pose(i, 30), K)
        with np.errstate(invalid="ignore"):
            frames.append(np.where(np.isnan(d), 0, np.clip(np.rint(1000.0 * d), 0, 65535)).astype(np.uint16))
    a = TrackingPipeline(roo, (N, N, N), bmin, bmax, w, h, K=K, near=near, far=far, device_icp=True, track=False, sensor="u16", sensor_scale=SCALE)
    b = TrackingPipeline(roo, (N, N, N), bmin, bmax, w, h, K=K, near=near, far=far, device_icp=True, track=False)
    metres = [_metres(roo, f) for f in frames]
    a.submit(frames[0])
    for i in range(n):
        init = scenes.orbit_pose(0, 30) if i == 0 else None
        if i + 1 < n:
            a.submit(frames[i + 1])
        Ta = a.step(init, next_image=FROM_SENSOR if i + 1 < n else None)
        Tb = b.step(init, metres[i], next_image=metres[i + 1] if i + 1 < n else None)
        assert np.asarray(Ta, np.float64).tobytes() == np.asarray(Tb, np.float64).tobytes(), i
        assert (a.rmse == b.rmse or (np.isnan(a.rmse) and np.isnan(b.rmse))) and a.tracking_good == b.tracking_good, i
    assert a.input.pending == 0 and a.resets == b.resets == 0 and a.tracking_good
    assert T.nan_equal(a.vol.MemcpyToHost(), b.vol.MemcpyToHost())


if __name__ == "__main__":
    if sys.argv[1:] == ["--tile-child"]:
        _tile_child()
