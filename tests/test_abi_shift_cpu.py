"""The moving volume (include/kfx_shift.h) is exported by libkfx.so, has its ctypes bindings, stays out of kfx.h and kfx_mesh.h,
refuses bad arguments before any HIP call, and its box is BoundedVolume.VoxelPositionInUnits bit for bit.  No GPU: the pointers below
are never dereferenced, and every call is a refusal, a host-only function or a zero shift, which launches nothing."""
import ctypes as C
import os
import re

import numpy as np

import kfx_testlib as T
from kangaroo_amd import _lib, roo

E_NULL, E_SHAPE, E_ALIGN, E_RANGE = -1, -2, -3, -4
FAKE = 1 << 20   # an aligned address that nothing may touch
F32, F16, COLOR = 0, 1, 2
CELL_BYTES = {F32: 8, F16: 4, COLOR: 4}
R = C.byref

NAMES = ["kfx_frame_shift", "kfx_volume_shift", "kfx_volume_shift_box", "kfx_volume_shift_plan", "kfx_volume_shift_scratch_bytes"]
MESH_NAMES = ["kfx_mesh_emit", "kfx_mesh_plan", "kfx_mesh_scratch_bytes"]


def declared(header):
    src = open(os.path.join(T.ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kfx_[a-z0-9_]+)\s*\(", src)))


def volume(w, h, d, cell_bytes, lo=(-1.0, -1.0, 2.0), hi=(1.0, 1.0, 4.0)):
    v = _lib.KfxVolume(w * cell_bytes, FAKE, w, h, w * cell_bytes * h, d)
    for i in range(3):
        v.boxmin[i], v.boxmax[i] = lo[i], hi[i]
    return v


def s3(*s):
    return (C.c_int * 3)(*s)


def test_shift_symbols_are_exported_and_bound_and_the_other_headers_keep_their_lists():
    L = _lib.load()
    names = declared("kfx_shift.h")
    assert names == NAMES, names
    for n in names:
        assert hasattr(L, n), "libkfx.so does not export %s" % n
        assert n in _lib.SIGNATURES, "python binding missing for %s" % n
    path = declared("kfx.h")
    assert len(path) <= 80 and not set(path) & set(names)
    assert declared("kfx_mesh.h") == MESH_NAMES
    header = open(os.path.join(T.ROOT, "include", "kfx_shift.h")).read()
    assert re.search(r"#define\s+KFX_CELL_COLOR\s+2\b", header)
    assert (roo.CELL_KIND["f32"], roo.CELL_KIND["f16"], roo.CELL_KIND["c32"]) == (F32, F16, COLOR)


def shift(L, vol, cell, s, scratch, nbytes, fill=float("nan")):
    return L.kfx_volume_shift(R(vol) if vol is not None else None, cell, s, fill, scratch, nbytes, None)


def plan(L, vol, cell, s, nbytes, steps=None, max_steps=0, n=None):
    n = C.c_int(-1) if n is None else n
    return L.kfx_volume_shift_plan(R(vol) if vol is not None else None, cell, s, nbytes, steps, max_steps, R(n) if n is not False else None)


def test_every_refusal_gives_its_code_before_any_hip_call():
    L = _lib.load()
    for cell, cb in CELL_BYTES.items():
        vol = volume(40, 24, 16, cb)
        staged, direct, gone, zero = s3(3, -2, 0), s3(3, -2, 5), s3(40, 0, 0), s3(0, 0, 0)
        need = L.kfx_volume_shift_scratch_bytes(R(vol), cell, staged)
        assert need == (40 * 24 * cb + 255) // 256 * 256
        # no scratch where the plan never stages: a z-shift (direct), a shift out of the volume (one fill), no shift at all
        for s in (direct, gone, zero, s3(0, 0, -16), s3(0, 24, 0)):
            assert L.kfx_volume_shift_scratch_bytes(R(vol), cell, s) == 0
        # null volume, null shift, null scratch where one is needed
        assert L.kfx_volume_shift_scratch_bytes(None, cell, staged) == 0 and L.kfx_volume_shift_scratch_bytes(R(vol), cell, None) == 0
        assert shift(L, None, cell, staged, FAKE, need) == E_NULL
        assert shift(L, vol, cell, None, FAKE, need) == E_NULL
        assert shift(L, vol, cell, staged, None, need) == E_NULL
        nullvol = volume(40, 24, 16, cb)
        nullvol.ptr = None
        assert shift(L, nullvol, cell, staged, FAKE, need) == E_NULL and shift(L, nullvol, cell, zero, None, 0) == E_NULL
        assert plan(L, None, cell, staged, need) == E_NULL and plan(L, vol, cell, None, need) == E_NULL
        assert plan(L, vol, cell, staged, need, n=False) == E_NULL
        assert plan(L, vol, cell, staged, need, steps=None, max_steps=4) == E_NULL
        # scratch below the minimum, misaligned scratch
        assert shift(L, vol, cell, staged, FAKE, need - 1) == E_SHAPE and shift(L, vol, cell, staged, FAKE, 0) == E_SHAPE
        assert plan(L, vol, cell, staged, need - 1) == E_SHAPE
        for off in (1, 8, 16, 128):
            assert shift(L, vol, cell, staged, FAKE + off, need + 256) == E_ALIGN
        # the volume's own rules come first, each with its code
        def broken(**kw):
            v = volume(40, 24, 16, cb)
            for k, val in kw.items():
                setattr(v, k, val)
            return shift(L, v, cell, staged, FAKE, need)
        assert broken(ptr=FAKE + cb // 2) == E_ALIGN
        assert broken(w=0) == E_SHAPE and broken(h=0) == E_SHAPE and broken(d=0) == E_SHAPE and broken(d=65536) == E_SHAPE
        assert broken(pitch=39 * cb) == E_SHAPE and broken(img_pitch=40 * cb * 24 - cb) == E_SHAPE
        # a zero shift launches nothing and needs nothing
        assert shift(L, vol, cell, zero, None, 0) == 0
        n = C.c_int(-1)
        assert plan(L, vol, cell, zero, 0, n=n) == 0 and n.value == 0
    # unknown cell kind
    vol = volume(40, 24, 16, 8)
    for bad in (3, -1, 7):
        assert L.kfx_volume_shift_scratch_bytes(R(vol), bad, s3(1, 0, 0)) == 0
        assert shift(L, vol, bad, s3(1, 0, 0), FAKE, 1 << 20) == E_RANGE
        assert plan(L, vol, bad, s3(1, 0, 0), 1 << 20) == E_RANGE
    # the frame hook and the box
    assert L.kfx_frame_shift(None, s3(1, 0, 0), FAKE, 1 << 20, None) == E_NULL
    lo, hi = (C.c_float * 3)(), (C.c_float * 3)()
    assert L.kfx_volume_shift_box(None, s3(1, 0, 0), lo, hi) == E_NULL and L.kfx_volume_shift_box(R(vol), None, lo, hi) == E_NULL
    assert L.kfx_volume_shift_box(R(vol), s3(1, 0, 0), None, hi) == E_NULL and L.kfx_volume_shift_box(R(vol), s3(1, 0, 0), lo, None) == E_NULL


class HostVolume:
    """what roo.BoundedVolume.VoxelPositionInUnits reads of a volume, without device memory"""
    VoxelPositionInUnits = roo.BoundedVolume.VoxelPositionInUnits

    def __init__(self, dims, lo, hi):
        self.w, self.h, self.d = dims
        self.boxmin, self.boxmax = np.asarray(lo, np.float32), np.asarray(hi, np.float32)


SHIFTS = [(1, 0, 0), (-1, 0, 0), (0, 3, 0), (0, 0, -5), (3, -2, 5), (-7, 5, -1), (8, 0, 0), (8, 0, -8), (31, 31, 31), (32, 0, 0), (0, 0, -32),
          (-100, 7, 1000)]
BOXES = [((32, 32, 32), (-1, -1, 2), (1, 1, 4)),                       # positions that round: the box may move by an ulp
         ((32, 32, 32), (-1, -1, 2), (0.9375, 0.9375, 3.9375)),        # positions that are multiples of 1/16: exact
         ((40, 24, 16), (-0.7, 0.1, 1.3), (1.9, 2.2, 2.05))]


def test_shift_box_is_voxel_position_in_units_bit_for_bit():
    L = _lib.load()
    for dims, lo, hi in BOXES:
        v = volume(dims[0], dims[1], dims[2], 8, lo, hi)
        host = HostVolume(dims, lo, hi)
        for s in SHIFTS:
            blo, bhi = (C.c_float * 3)(), (C.c_float * 3)()
            assert L.kfx_volume_shift_box(R(v), s3(*s), blo, bhi) == 0
            want_lo = host.VoxelPositionInUnits(*s)
            want_hi = host.VoxelPositionInUnits(dims[0] - 1 + s[0], dims[1] - 1 + s[1], dims[2] - 1 + s[2])
            assert np.array_equal(np.array(blo[:], np.float32).view(np.uint32), want_lo.view(np.uint32)), (dims, lo, s)
            assert np.array_equal(np.array(bhi[:], np.float32).view(np.uint32), want_hi.view(np.uint32)), (dims, lo, s)
    # on the exact lattice a shift by 8 cells moves the box by exactly half a unit and leaves every voxel position what it was
    dims, lo, hi = BOXES[1]
    v, blo, bhi = volume(32, 32, 32, 8, lo, hi), (C.c_float * 3)(), (C.c_float * 3)()
    assert L.kfx_volume_shift_box(R(v), s3(8, 0, -8), blo, bhi) == 0
    assert list(blo) == [-0.5, -1.0, 1.5] and list(bhi) == [1.4375, 0.9375, 3.4375]
    old, new = HostVolume(dims, lo, hi), HostVolume(dims, blo[:], bhi[:])
    for i in range(32):
        p_new = new.VoxelPositionInUnits(i, i, i)
        p_old = old.VoxelPositionInUnits(i + 8, i, i - 8)
        assert np.array_equal(p_new.view(np.uint32), p_old.view(np.uint32)), i
