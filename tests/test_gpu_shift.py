"""The moving volume on the GPU (include/kfx_shift.h, roo.VolumeShift, roo.Frame.shift, FramePipeline(follow=)).

  * a shift equals numpy, every BYTE of the storage compared: retained cells verbatim, exposed cells the bytes of the matching
    reset, everything outside the view's cells -- pitch padding, the neighbours of a sub-view -- untouched; the box is
    kfx_volume_shift_box's;
  * on a lattice whose voxel positions are exact in fp32, shifting commutes with SdfFuse bit for bit: the oracle fused into a
    fresh volume with the shifted box is the reference;
  * a summary rebuilt after the shift is one the table march can trust;
  * kfx_frame_shift between frame steps equals the separate entry points; FramePipeline(follow=) equals a manual loop."""
import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import oracle, scenes

pytestmark = pytest.mark.gpu

NAN = float("nan")
LO, HI = (-1.0, -1.0, 2.0), (1.0, 1.0, 4.0)
SHIFTS = [(1, 0, 0), (-1, 0, 0), (0, 3, 0), (0, 0, -5), (3, -2, 5), (-7, 5, -1), (39, 23, 15), (40, 0, 0), (0, 0, -16)]
# (name, cell kind, dims, pitch, view (start, size) or None, fill, shifts)
CASES = [
    ("f32", "f32", (40, 24, 16), None, None, NAN, SHIFTS),
    ("f32-finite-fill", "f32", (40, 24, 16), None, None, 1.25, [(3, -2, 5), (0, 3, 0)]),
    # rows that start 8-byte aligned only; the neighbours of the view are part of the storage that must not change
    ("f32-subview", "f32", (40, 24, 16), None, ((3, 2, 1), (32, 16, 12)), NAN, SHIFTS + [(31, 15, 11), (-2, 1, 0), (5, 0, -3)]),
    ("f16", "f16", (72, 16, 24), None, None, NAN, SHIFTS + [(71, 0, 0), (-4, 0, 0), (0, 0, 23)]),
    ("f16-subview", "f16", (72, 16, 24), None, ((1, 2, 1), (66, 9, 20)), NAN, [(1, 0, 0), (-3, 2, 0), (2, -1, 4), (0, 0, -7), (65, 8, 19)]),
    # a pitch that is no multiple of 16: every row has its own distance to the 16-byte boundary below it
    ("f16-odd-pitch", "f16", (41, 5, 6), 41 * 4 + 4, None, NAN, [(1, 0, 0), (-2, 1, 0), (3, -1, 2), (0, 0, -1)]),
    ("colour", "c32", (40, 24, 16), None, None, 0.5, SHIFTS),
    ("colour-odd-pitch", "c32", (37, 6, 5), 37 * 4, None, 0.5, [(-1, 0, 0), (2, -1, 0), (1, 1, -2)]),
    # more than one 1 KiB piece per row and more rows than one pass of the grid covers
    ("f32-wide", "f32", (300, 70, 40), None, None, NAN, [(8, 0, 0), (-5, 3, 8), (0, 0, -3)]),
]


def _cells(buf, vol):
    """strided (d, h, w) view of the cells of `vol` (a roo volume or view) in the byte array `buf` of its storage"""
    dt = np.uint64 if vol.ELEM == 8 else np.uint32
    n = (vol.d - 1) * vol.img_pitch + (vol.h - 1) * vol.pitch + vol.w * vol.ELEM
    return np.lib.stride_tricks.as_strided(buf[vol.offset:vol.offset + n].view(dt), (vol.d, vol.h, vol.w), (vol.img_pitch, vol.pitch, vol.ELEM))


def _shifted(cells, shift, fill_bits):
    sx, sy, sz = shift
    d, h, w = cells.shape
    out = np.full_like(cells, fill_bits)
    z0, z1, y0, y1, x0, x1 = max(0, -sz), min(d, d - sz), max(0, -sy), min(h, h - sy), max(0, -sx), min(w, w - sx)
    if z0 < z1 and y0 < y1 and x0 < x1:
        out[z0:z1, y0:y1, x0:x1] = cells[z0 + sz:z1 + sz, y0 + sy:y1 + sy, x0 + sx:x1 + sx]
    return out


def _fill_bits(roo, kind, fill):
    """the bytes of a cell after the matching reset"""
    import torch
    if kind == "c32":
        return np.array([fill], np.float32).view(np.uint32)[0]
    v = roo.BoundedVolume(8, 8, 8, kind=kind)
    roo.SdfReset(v, fill)
    torch.cuda.synchronize()
    return _cells(v.storage.cpu().numpy(), v)[3, 4, 5]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gpu_shift_equals_numpy_byte_for_byte(roo, case):
    import torch
    _, kind, dims, pitch, view, fill, shifts = case
    fill_bits = _fill_bits(roo, kind, fill)
    if kind == "f32" and fill != fill:
        assert fill_bits == 0x7fc00000   # {NaN, 0.0f}
    rng = np.random.default_rng(7)
    for k, shift in enumerate(shifts):
        staged = shift[2] == 0
        for planes in ((1, 3, 16) if staged else (16,)):
            vol = roo.BoundedVolume(dims[0], dims[1], dims[2], LO, HI, pitch=pitch, kind=kind)
            before = rng.integers(0, 256, vol.storage.numel(), dtype=np.uint8)   # the sentinel: every byte of the storage, NaN payloads among the cells
            vol.storage.copy_(torch.from_numpy(before))
            tgt = vol if view is None else vol.SubVolume(*view)
            if view is not None:
                tgt.boxmin = vol.VoxelPositionInUnits(*view[0])
                tgt.boxmax = vol.VoxelPositionInUnits(*(view[0][i] + view[1][i] - 1 for i in range(3)))
            want_lo, want_hi = roo.VolumeShiftBox(tgt, shift)
            need = roo.VolumeShiftScratchBytes(tgt, shift)
            inside = all(abs(s) < n for s, n in zip(shift, (tgt.w, tgt.h, tgt.d)))
            assert (need > 0) == (staged and inside)
            scratch = None
            if need:   # exactly `planes` packed planes (at least the minimum), guarded by a sentinel behind them
                nbytes = max(need, min(planes, tgt.d) * tgt.w * tgt.h * tgt.ELEM)
                whole = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
                scratch = whole[:nbytes]
            roo.VolumeShift(tgt, shift, fill, scratch)
            torch.cuda.synchronize()
            after = vol.storage.cpu().numpy()
            expect = before.copy()
            _cells(expect, tgt)[...] = _shifted(_cells(before, tgt), shift, fill_bits)
            bad = np.flatnonzero(after != expect)
            assert bad.size == 0, (case[0], shift, planes, "%d bytes differ, first at %s" % (bad.size, bad[:8].tolist()))
            assert np.array_equal(tgt.boxmin.view(np.uint32), want_lo.view(np.uint32)) and np.array_equal(tgt.boxmax.view(np.uint32), want_hi.view(np.uint32))
            if need:
                assert bool((whole[nbytes:] == 0xA5).all()), "the scratch was written beyond its end"


def test_gpu_shift_commutes_with_sdf_fuse_against_the_oracle(roo):
    """Dims 32^3, box (-1, -1, 2) - (0.9375, 0.9375, 3.9375): voxel positions are multiples of 1/16, exact in fp32, and stay the same
    floats under a shift by (8, 0, -8), so a cell's update depends on nothing the shift changes."""
    import torch
    N, w, h, shift = 32, 80, 60, (8, 0, -8)
    lo, hi = (-1.0, -1.0, 2.0), (0.9375, 0.9375, 3.9375)
    assert roo.get_math_mode() == "exact"
    K = scenes.intrinsics(w, h)
    tr = scenes.trunc_dist(lo, hi, (N, N, N))
    frames = []
    for i in range(3):
        T_wc = scenes.orbit_pose(i, 8)
        f, _, nrm = T.preprocess_oracle(scenes.render_depth("room", w, h, T_wc, K), K)
        frames.append((scenes.se3_inverse(T_wc), f, nrm))
    vol = roo.BoundedVolume(N, N, N, lo, hi)
    roo.SdfReset(vol, NAN)
    for T_cw, f, nrm in frames:
        roo.SdfFuse(vol, T.upload_image(roo, f.data), T.upload_image(roo, nrm.data), T_cw, K, tr, scenes.MAX_W, scenes.MIN_COS_THETA)
    roo.VolumeShift(vol, shift, NAN)
    torch.cuda.synchronize()
    assert vol.boxmin.tolist() == [-0.5, -1.0, 1.5] and vol.boxmax.tolist() == [1.4375, 0.9375, 3.4375]
    # the premise itself: all 32 positions per axis of the shifted box are the old box's floats
    old, new = oracle.Volume(N, N, N, lo, hi), oracle.Volume(N, N, N, vol.boxmin, vol.boxmax)
    for i in range(N):
        a, b = oracle.voxel_position(new, i, i, i), oracle.voxel_position(old, i + shift[0], i + shift[1], i + shift[2])
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), i
    assert scenes.trunc_dist(vol.boxmin, vol.boxmax, (N, N, N)) == tr
    oracle.sdf_reset(new, NAN)
    updated = 0
    for T_cw, f, nrm in frames:
        updated += oracle.sdf_fuse(new, f, nrm, T_cw, K, tr, scenes.MAX_W, scenes.MIN_COS_THETA)
    got, want = vol.MemcpyToHost().view(np.uint32), np.ascontiguousarray(new.data).view(np.uint32)
    kept = np.zeros((N, N, N), bool)
    kept[8:, :, :24] = True   # z - 8 >= 0 and x + 8 < 32
    assert np.array_equal(got[kept], want[kept]), T.mismatch_report(vol.MemcpyToHost()[kept], new.data[kept])
    assert int((new.data[kept][:, 1] > 0).sum()) > 1000 and updated > 0   # the retained region holds fused cells
    blank = roo.BoundedVolume(N, N, N, lo, hi)
    roo.SdfReset(blank, NAN)
    torch.cuda.synchronize()
    assert np.array_equal(got[~kept], blank.MemcpyToHost().view(np.uint32)[~kept])   # the exposed region: exactly SdfReset(NaN)'s bytes


def _images_equal(a, b):
    return all(np.array_equal(x.MemcpyToHost().view(np.uint32), y.MemcpyToHost().view(np.uint32)) for x, y in zip(a, b))


def test_gpu_shift_with_a_summary_leaves_a_summary_the_march_can_trust(roo):
    import torch
    N, w, h = 64, 160, 120
    bmin, bmax, near, far = scenes.SCENES["room"]
    K = scenes.intrinsics(w, h)
    tr = scenes.trunc_dist(bmin, bmax, (N, N, N))
    vol = roo.BoundedVolume(N, N, N, bmin, bmax)
    summ = roo.SdfSummary(vol)
    roo.SdfReset(vol, NAN, summary=summ)
    mk = lambda: (roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h))
    f, vbo, nrm = roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h, "f32x4")

    def fuse(i):
        T_wc = scenes.orbit_pose(i, 8)
        roo.BilateralFilter(f, T.upload_image(roo, scenes.render_depth("room", w, h, T_wc, K)), **scenes.BILATERAL)
        roo.DepthToVbo(vbo, f, K)
        roo.NormalsFromVbo(nrm, vbo)
        roo.SdfFuse(vol, f, nrm, scenes.se3_inverse(T_wc), K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, summary=summ)
        return T_wc

    def marches_agree(T_wc):
        a, b = mk(), mk()
        roo.RaycastSdf(a[0], a[1], a[2], vol, T_wc, K, near, far, tr, True, summary=summ)
        roo.RaycastSdf(b[0], b[1], b[2], vol, T_wc, K, near, far, tr, True)
        torch.cuda.synchronize()
        assert int(np.isfinite(b[0].MemcpyToHost()).sum()) > w * h // 10   # the model is in view
        return _images_equal(a, b)

    for i in range(3):
        T_wc = fuse(i)
    assert marches_agree(T_wc)
    before = vol.MemcpyToHost()
    roo.VolumeShift(vol, (8, 0, -8), NAN, summary=summ)
    torch.cuda.synchronize()
    after = vol.MemcpyToHost()
    assert T.nan_equal(after[8:, :, :56], before[:56, :, 8:]) and np.isnan(after[:8, :, :, 0]).all() and np.isnan(after[:, :, 56:, 0]).all()
    assert marches_agree(T_wc)
    T_wc = fuse(3)                 # one more tracked fuse into the moved volume
    assert marches_agree(T_wc)
    roo.VolumeShift(vol, (0, -8, 0), NAN, summary=summ)   # the staged path
    assert marches_agree(T_wc)


@pytest.mark.parametrize("track", [False, True])
def test_gpu_frame_shift_equals_the_separate_entry_points(roo, track):
    import torch
    N, w, h = 64, 160, 120
    bmin, bmax, near, far = scenes.SCENES["room"]
    K = scenes.intrinsics(w, h)
    tr = scenes.trunc_dist(bmin, bmax, (N, N, N))
    va, vb = roo.BoundedVolume(N, N, N, bmin, bmax), roo.BoundedVolume(N, N, N, bmin, bmax)
    mk = lambda: [roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h, "f32x4"), roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h)]
    ia, ib = mk(), mk()
    fr = roo.Frame(vb, roo.Image(w, h), ib[0], ib[1], ib[2], ib[3], ib[4], ib[5], K, scenes.BILATERAL, near, far, tr, scenes.MAX_W, scenes.MIN_COS_THETA)
    summ = roo.SdfSummary(va) if track else None
    roo.SdfReset(va, NAN, summary=summ)
    fr.set_track(track)
    fr.reset()
    kw = {"summary": summ} if track else {}
    for i in range(6):
        if i == 3:
            for shift in ((8, 0, -8), (0, 8, 0)):   # a direct and a staged shift
                roo.VolumeShift(va, shift, NAN, summary=summ)
                fr.shift(shift)
            assert np.array_equal(va.boxmin, vb.boxmin) and np.array_equal(va.boxmax, vb.boxmax) and va.boxmin.tolist() != list(bmin)
        T_wc = scenes.orbit_pose(i, 8)
        raw = T.upload_image(roo, scenes.render_depth("room", w, h, T_wc, K))
        roo.BilateralFilter(ia[0], raw, **scenes.BILATERAL)
        roo.DepthToVbo(ia[1], ia[0], K)
        roo.NormalsFromVbo(ia[2], ia[1])
        roo.SdfFuse(va, ia[0], ia[2], scenes.se3_inverse(T_wc), K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, **kw)
        roo.RaycastSdf(ia[3], ia[4], ia[5], va, T_wc, K, near, far, tr, True, **kw)
        fr.step(T_wc, scenes.se3_inverse(T_wc), raw)
        torch.cuda.synchronize()
        assert np.array_equal(va.MemcpyToHost().view(np.uint32), vb.MemcpyToHost().view(np.uint32)), i
        assert _images_equal(ia[3:], ib[3:]), i
    assert int(np.isfinite(ib[3].MemcpyToHost()).sum()) > w * h // 10


@pytest.mark.parametrize("color", [False, True])
def test_gpu_pipeline_follows_the_camera(roo, color):
    import torch
    from kangaroo_amd.pipeline import FramePipeline, follow_shift

    class Operators(FramePipeline):
        USE_FRAME = False   # the manual loop shifts with roo.VolumeShift: its steps must read the volume's box at every call

    N, w, h = 64, 160, 120
    bmin, bmax, near, far = scenes.SCENES["room"]
    a = FramePipeline(roo, (N, N, N), bmin, bmax, w, h, near=near, far=far, color=color, follow=dict(quantum=8, slack=8))
    b = Operators(roo, (N, N, N), bmin, bmax, w, h, near=near, far=far, color=color)
    assert (a.kframe is None) == color and b.kframe is None and a.shifts == []
    focus, expected, fused = None, [], 0
    step = 0.1 * (bmax[0] - bmin[0])
    for i in range(12):
        T_wc = np.array([[1, 0, 0, step * i], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
        if focus is None:   # focus=None: the distance from the camera centre to the box centre at the first step
            focus = float(np.linalg.norm(0.5 * (np.float64(bmin) + np.float64(bmax)) - np.float64(T_wc[:, 3])))
        s = follow_shift(b.vol.boxmin, b.vol.boxmax, (N, N, N), T_wc, focus, quantum=8, slack=8)
        if any(s):
            expected.append((i, s))
            roo.VolumeShift(b.vol, s, NAN)
            if color:
                roo.VolumeShift(b.cvol, s, 0.5)
                torch.cuda.synchronize()
                c = b.cvol.MemcpyToHost()[..., 0]
                assert s[0] > 0 and s[1] == 0 and s[2] == 0 and np.all(c[:, :, N - s[0]:] == 0.5)   # the exposed cells
        raw = T.upload_image(roo, scenes.render_depth("room", w, h, T_wc, a.K))
        a.step(T_wc, raw)
        b.step(T_wc, raw)
        torch.cuda.synchronize()
        assert np.array_equal(a.vol.boxmin.view(np.uint32), b.vol.boxmin.view(np.uint32)) and np.array_equal(a.vol.boxmax.view(np.uint32), b.vol.boxmax.view(np.uint32)), i
        got = a.vol.MemcpyToHost()
        assert np.array_equal(got.view(np.uint32), b.vol.MemcpyToHost().view(np.uint32)), i
        fused = max(fused, int((got[..., 1] > 0).sum()))
        if color:
            assert np.array_equal(a.cvol.boxmin, b.cvol.boxmin) and np.array_equal(a.cvol.MemcpyToHost().view(np.uint32), b.cvol.MemcpyToHost().view(np.uint32)), i
    assert a.shifts == expected and len(expected) >= 2, (a.shifts, expected)
    assert a.trunc == b.trunc == scenes.trunc_dist(bmin, bmax, (N, N, N))
    assert fused > 1000   # a model was fused along the way


def test_gpu_tracking_pipeline_follows_the_camera_and_keeps_tracking(roo):
    """TrackingPipeline(follow=): the shift is evaluated for the PREVIOUS frame's pose, the summary is rebuilt, the bound SdfFuse calls
    take the new box -- a model left at the wrong place would be a quantum (8 voxels) off, and the tracker with it."""
    from kangaroo_amd.pipeline import TrackingPipeline, follow_shift
    N, w, h, n = 64, 160, 120, 16
    bmin, bmax, near, far = scenes.SCENES["room"]
    K = scenes.intrinsics(w, h)
    voxel = (bmax[0] - bmin[0]) / (N - 1)
    p = TrackingPipeline(roo, (N, N, N), bmin, bmax, w, h, K=K, near=near, far=far, device_icp=True, track=True, follow=dict(quantum=8, slack=8))
    truth = [np.array([[1, 0, 0, 0.04 * i], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32) for i in range(n)]
    expected, focus = [], None
    for i in range(n):
        if i > 0:   # what the step is to decide: the box as it stands, the pose of the frame before
            if focus is None:
                focus = float(np.linalg.norm(0.5 * (np.float64(p.vol.boxmin) + np.float64(p.vol.boxmax)) - p.T_wl[:3, 3]))
            s = follow_shift(p.vol.boxmin, p.vol.boxmax, (N, N, N), p.T_wl, focus, quantum=8, slack=8)
            if any(s):
                expected.append((i, s))
        T_wl = p.step(truth[0] if i == 0 else None, T.upload_image(roo, scenes.render_depth("room", w, h, truth[i], K)))
        err = float(np.linalg.norm(T_wl[:3, 3] - np.float64(truth[i][:, 3])))
        print("frame %d: rmse %.5f, position error %.5f m, box x %.4f .. %.4f" % (i, p.rmse, err, p.vol.boxmin[0], p.vol.boxmax[0]))
        assert p.tracking_good and np.isfinite(p.rmse) and err < voxel, (i, err)
    assert p.shifts == expected and len(expected) >= 2 and all(s == (8, 0, 0) for _, s in expected), (p.shifts, expected)
    assert p.resets == 0 and abs(float(p.vol.boxmin[0]) - (bmin[0] + 8 * len(expected) * voxel)) < 1e-5


def test_gpu_slab_pipelines_refuse_follow(roo):
    from kangaroo_amd.pipeline import SlabPipeline, TrackingSlabPipeline

    class Dist:
        def get_rank(self):
            return 0

        def get_world_size(self):
            return 1
    for cls in (SlabPipeline, TrackingSlabPipeline):
        with pytest.raises(ValueError, match="follow="):
            cls(roo, Dist(), (32, 32, 32), LO, HI, 80, 60, follow=dict(quantum=8, slack=8))
