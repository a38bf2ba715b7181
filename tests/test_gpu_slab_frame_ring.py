"""The ring of timing events (kangaroo_amd/csrc/frame_host.h) through kfx_slab_frame: it wraps, honours the event mask, and
reports what it no longer holds.  (The plain frame's ring: tests/test_gpu_frame.py.)  32^3 fp32 cells, 64 x 48 images, 4 timing
slots.  Fields of kfx_slab_frame_timings: preprocess, sdf_fuse, raycast, merge, frame, period.  With one rank (world = 1) no step
records event 4 -- there is nothing to merge and the exact raycast is not pipelined -- so the merge field is NaN there; the event's
two paths (late, from the side stream, and on the caller's stream) are taken by one rank of two over the loop-back transport."""
import ctypes as C

import numpy as np
import pytest

from kfx_testlib import scenes

pytestmark = pytest.mark.gpu

N, W, H, SLOTS = 32, 64, 48, 4
PRE, FUSE, MARCH, MERGE, TOTAL, PERIOD = range(6)
E_SHAPE, E_RANGE = -2, -4


class OneRank:
    @staticmethod
    def get_rank():
        return 0

    @staticmethod
    def get_world_size():
        return 1


@pytest.mark.parametrize("raycast", ["exact", "composite"])
def test_gpu_slab_frame_timing_ring_wraps_and_honours_the_mask(roo, raycast):
    from kangaroo_amd import _lib, slab as S
    from kangaroo_amd.pipeline import SlabPipeline
    bmin, bmax, near, far = scenes.SCENES["room"]
    comm = S.Comm.threads(1)[0]
    try:
        sp = SlabPipeline(roo, OneRank, (N, N, N), bmin, bmax, W, H, near=near, far=far, driver="c", comm=comm, raycast=raycast, timing_slots=SLOTS)
        f = sp.sframe
        assert f.timing_slots == SLOTS
        sp.raw.MemcpyFromHost(scenes.render_depth("room", W, H, scenes.orbit_pose(0, 8), sp.K))
        f.reset()

        def step(n):
            for _ in range(n):
                f.step(scenes.orbit_pose(f.count, 8))

        def code(first, n):
            with pytest.raises(_lib.KfxError) as e:
                f.timings(first, n)
            return e.value.code

        # all five events, six frames into four slots: frames 2 .. 5 are held, frame 0 has been overwritten
        step(6)
        t = f.timings(2, 4)
        assert np.isfinite(t[:, [PRE, FUSE, MARCH, TOTAL]]).all(), t
        assert np.isfinite(t[:3, PERIOD]).all() and np.isnan(t[3, PERIOD]), t
        assert code(0, 1) == E_RANGE and code(1, 5) == E_RANGE
        # the two events around SdfFuse: its span and the period from one frame to the next, nothing else
        f.set_timing(f.EVENTS_FUSE)
        step(2)
        t = f.timings(6, 2)
        assert np.isfinite(t[:, FUSE]).all() and np.isfinite(t[0, PERIOD]) and np.isnan(t[1, PERIOD]), t
        assert np.isnan(t[:, [PRE, MARCH, MERGE]]).all(), t
        assert (t[:, TOTAL] == t[:, FUSE]).all(), t   # ("frame" = first to last recorded event, include/kfx_slab.h: the same two events)
        assert np.isnan(f.timings(5, 1)[0, PERIOD])   # (frame 6 did not record frame 5's first event)
        # no events
        f.set_timing(f.EVENTS_NONE)
        step(1)
        assert np.isnan(f.timings(8, 1)).all()
        assert code(8, 2) == E_RANGE and code(9, 1) == E_RANGE   # more frames than were stepped
        f.sync()

        # kfx_slab_frame_set_color's rgb image: one broken rule each (tests/test_abi_images_cpu.py has the other entry points, where no device
        # exists).  The pointers are fake: rejections only here, nothing that would get as far as a launch.
        if raycast == "exact":
            L, K = S._L(), (C.c_float * 4)(*[float(x) for x in sp.K])
            cv = _lib.KfxVolume(N * 4, 1 << 20, N, N, N * 4 * N, N)
            cv.boxmin, cv.boxmax = sp.vol.view().boxmin, sp.vol.view().boxmax
            rgb = lambda **kw: C.byref(_lib.KfxImage(kw.get("pitch", W * 3), kw.get("ptr", 1 << 20), kw.get("w", W), H))   # noqa: E731
            assert L.kfx_slab_frame_set_color(f.handle, C.byref(cv), rgb(ptr=None), K, None) == -1
            assert L.kfx_slab_frame_set_color(f.handle, C.byref(cv), rgb(pitch=W * 3 - 3), K, None) == E_SHAPE
            assert L.kfx_slab_frame_set_color(f.handle, C.byref(cv), rgb(w=3, pitch=9), K, None) == E_SHAPE
        del sp, f
    finally:
        comm.destroy()


class RankOfTwo:
    """torch.distributed's rank / world queries for rank 1 of 2 (the C driver's collectives go through the loop-back transport)"""
    @staticmethod
    def get_rank():
        return 1

    @staticmethod
    def get_world_size():
        return 2


@pytest.mark.parametrize("raycast,overlap", [("exact", True), ("composite", False), ("composite", True)])
def test_gpu_slab_frame_merge_event_is_waited_for_on_either_stream(roo, raycast, overlap):
    """Rank 1 of 2 over the loop-back transport (every collective moves this rank's own bytes: times are a rank's, the images are not
    a rendering).  Pipelined exact raycast: event 4 is recorded late, by the final exchange on the side stream; composite: after the
    merge, on the caller's stream or, overlapped, on the side stream.  timings() is asked with nothing synchronised: its one wait
    plus the side-stream events must cover event 4, so the merge span is finite for every frame the ring holds."""
    from kangaroo_amd import slab as S
    from kangaroo_amd.pipeline import SlabPipeline
    bmin, bmax, near, far = scenes.SCENES["room"]
    comm = S.Comm.loopback(1, 2)
    sp = SlabPipeline(roo, RankOfTwo, (N, N, N), bmin, bmax, W, H, near=near, far=far, driver="c", comm=comm, raycast=raycast, overlap=overlap,
                      halo="recompute", ghost=2, unchecked=True, pipeline=2, timing_slots=SLOTS)
    f = sp.sframe
    sp.raw.MemcpyFromHost(scenes.render_depth("room", W, H, scenes.orbit_pose(0, 8), sp.K))
    f.reset()
    for i in range(6):
        f.step(scenes.orbit_pose(i, 8))
    t = f.timings(2, 4)   # (no wait(), no sync() before)
    assert np.isfinite(t[:, [PRE, FUSE, MARCH, MERGE, TOTAL]]).all(), t
    assert np.isfinite(t[:3, PERIOD]).all() and np.isnan(t[3, PERIOD]), t
    with pytest.raises(Exception) as e:
        f.timings(0, 1)
    assert e.value.code == E_RANGE
    f.wait()
    try:
        f.sync()
    except Exception:   # noqa: BLE001  (nobody marches the other slab: rays may stay open)
        pass
    del sp, f
