"""The plan of a volume shift (kfx_volume_shift_plan, include/kfx_shift.h) -- the list of launches kfx_volume_shift enqueues -- checked
without a device: no step reads what it writes, the steps run one after another in numpy give the shifted volume, a STAGE never
exceeds the scratch, and a shift along z is DIRECT chunks only."""
import ctypes as C

import numpy as np
import pytest

from kangaroo_amd import _lib

FAKE = 1 << 20
FILL, DIRECT, STAGE, PLACE = 0, 1, 2, 3
W, H, D, CB = 40, 24, 16, 8
PLANE = W * H * CB
SHIFTS = [(1, 0, 0), (-1, 0, 0), (0, 3, 0), (0, 0, -5), (3, -2, 5), (-7, 5, -1), (39, 23, 15), (40, 0, 0), (0, 0, -16)]
SCRATCH_PLANES = [1, 3, 16]
FILLV = np.uint64(0xFFFFFFFFFFFFFFFF)


def volume():
    v = _lib.KfxVolume(W * CB, FAKE, W, H, PLANE, D)
    for i in range(3):
        v.boxmin[i], v.boxmax[i] = -1.0, 1.0
    return v


def plan_of(shift, scratch_bytes):
    L, v, n, s = _lib.load(), volume(), C.c_int(-1), (C.c_int * 3)(*shift)
    assert L.kfx_volume_shift_plan(C.byref(v), 0, s, scratch_bytes, None, 0, C.byref(n)) == 0
    assert 0 <= n.value <= 2 * D + 1
    steps = (_lib.KfxShiftStep * max(n.value, 1))()
    m = C.c_int(-1)
    assert L.kfx_volume_shift_plan(C.byref(v), 0, s, scratch_bytes, steps, n.value, C.byref(m)) == 0 and m.value == n.value
    if n.value > 1:   # a shorter array takes the first steps only, and the count stays the whole plan's
        few, k = (_lib.KfxShiftStep * n.value)(), C.c_int(-1)
        assert L.kfx_volume_shift_plan(C.byref(v), 0, s, scratch_bytes, few, 1, C.byref(k)) == 0 and k.value == n.value
        assert (few[0].kind, few[0].dst_z0, few[0].dst_z1) == (steps[0].kind, steps[0].dst_z0, steps[0].dst_z1) and few[1].dst_z1 == 0
    return [(st.kind, st.dst_z0, st.dst_z1, st.src_z0, st.src_z1) for st in steps[:n.value]]


def reference(vol, shift):
    sx, sy, sz = shift
    out = np.full_like(vol, FILLV)
    for z in range(D):
        for y in range(H):
            if 0 <= z + sz < D and 0 <= y + sy < H:
                x0, x1 = max(0, -sx), min(W, W - sx)
                if x0 < x1:
                    out[z, y, x0:x1] = vol[z + sz, y + sy, x0 + sx:x1 + sx]
    return out


def in_plane(src, sx, sy):
    """planes shifted in x and y, the fill where the source is outside"""
    out = np.full_like(src, FILLV)
    y0, y1, x0, x1 = max(0, -sy), min(H, H - sy), max(0, -sx), min(W, W - sx)
    if y0 < y1 and x0 < x1:
        out[:, y0:y1, x0:x1] = src[:, y0 + sy:y1 + sy, x0 + sx:x1 + sx]
    return out


def byte_ranges(kind, d0, d1, s0, s1):
    """(buffer, first byte, end byte) of what a step reads and of what it writes: whole planes of the volume or of the scratch"""
    write = ("scratch" if kind == STAGE else "volume", d0 * PLANE, d1 * PLANE)
    read = None if kind == FILL else ("scratch" if kind == PLACE else "volume", s0 * PLANE, s1 * PLANE)
    return read, write


@pytest.mark.parametrize("planes", SCRATCH_PLANES)
@pytest.mark.parametrize("shift", SHIFTS)
def test_plan_is_hazard_free_and_computes_the_shift(shift, planes):
    scratch_bytes = planes * PLANE
    steps = plan_of(shift, scratch_bytes)
    vol = (np.arange(W * H * D, dtype=np.uint64) + np.uint64(1)).reshape(D, H, W)
    want = reference(vol, shift)
    scratch = np.zeros((planes, H, W), np.uint64)
    sx, sy, sz = shift
    for kind, d0, d1, s0, s1 in steps:
        assert kind in (FILL, DIRECT, STAGE, PLACE) and 0 <= d0 < d1
        read, write = byte_ranges(kind, d0, d1, s0, s1)
        assert write[2] <= (scratch_bytes if write[0] == "scratch" else D * PLANE), "a step writes beyond its buffer"
        if read is not None:
            assert 0 <= s0 < s1 and s1 - s0 == d1 - d0
            assert read[2] <= (scratch_bytes if read[0] == "scratch" else D * PLANE), "a step reads beyond its buffer"
            assert read[0] != write[0] or read[2] <= write[1] or write[2] <= read[1], "a launch reads bytes that it writes: %r" % ((kind, d0, d1, s0, s1),)
        if kind == FILL:
            vol[d0:d1] = FILLV
        elif kind == DIRECT:
            assert s0 - d0 == sz
            vol[d0:d1] = in_plane(vol[s0:s1].copy(), sx, sy)
        elif kind == STAGE:
            scratch[d0:d1] = vol[s0:s1]
        else:
            vol[d0:d1] = in_plane(scratch[s0:s1], sx, sy)
    assert np.array_equal(vol, want)
    kinds = [s[0] for s in steps]
    if abs(sx) >= W or abs(sy) >= H or abs(sz) >= D:
        assert steps == [(FILL, 0, D, 0, 0)]        # out of the volume: one fill
    elif sz != 0:                                   # a z-shift: DIRECT chunks of |sz| planes, whatever the scratch
        assert set(kinds) == {DIRECT, FILL} and kinds.count(FILL) == 1
        assert all(d1 - d0 <= abs(sz) for k, d0, d1, _, _ in steps if k == DIRECT)
        assert kinds.count(DIRECT) == -(-(D - abs(sz)) // abs(sz))
    else:                                           # in-plane: STAGE + PLACE per chunk of the planes the scratch holds
        assert kinds == [STAGE, PLACE] * (-(-D // planes))
        assert max(d1 - d0 for k, d0, d1, _, _ in steps if k == STAGE) == min(planes, D)
