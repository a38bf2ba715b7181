"""The planned mesh extraction (include/kfx_mesh.h) is exported by libkfx.so, has its ctypes bindings, and refuses bad arguments
before any HIP call: null pointers, an unknown cell kind, a slab whose stored planes do not cover its cubes and their normals'
stencil, too little scratch.  No GPU: the pointers below are never dereferenced."""
import ctypes as C
import os
import re

import kfx_testlib as T
from kangaroo_amd import _lib

E_NULL, E_SHAPE, E_ALIGN, E_RANGE = -1, -2, -3, -4
FAKE = 1 << 20   # an aligned address that nothing may touch


def declared():
    src = open(os.path.join(T.ROOT, "include", "kfx_mesh.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kfx_[a-z0-9_]+)\s*\(", src)))


def volume(w, h, d, cell_bytes, z0=-1.0, z1=1.0):
    v = _lib.KfxVolume(w * cell_bytes, FAKE, w, h, w * cell_bytes * h, d)
    for i in range(3):
        v.boxmin[i], v.boxmax[i] = -1.0, 1.0
    v.boxmin[2], v.boxmax[2] = z0, z1
    return v


def test_mesh_symbols_are_exported_and_bound():
    L = _lib.load()
    names = declared()
    assert names == ["kfx_mesh_emit", "kfx_mesh_plan", "kfx_mesh_scratch_bytes"], names
    for n in names:
        assert hasattr(L, n), "libkfx.so does not export %s" % n
        assert n in _lib.SIGNATURES, "python binding missing for %s" % n


def plan(L, vol, cell, slab, lo, hi, scratch, nbytes, totals):
    return L.kfx_mesh_plan(C.byref(vol) if vol is not None else None, cell, C.byref(slab) if slab is not None else None, lo, hi,
                           scratch, nbytes, totals, None)


def emit(L, vol, cell, slab, lo, hi, scratch, nbytes, totals, out=FAKE):
    return L.kfx_mesh_emit(C.byref(vol) if vol is not None else None, cell, C.byref(slab) if slab is not None else None, lo, hi, None,
                           scratch, nbytes, totals, out, out, out, out, None, None)


def test_mesh_entry_points_refuse_before_any_hip_call():
    L = _lib.load()
    tot = (C.c_ulonglong * 2)(10, 20)
    for cell, cb in ((0, 8), (1, 4)):
        vol = volume(40, 30, 50, cb)
        need = L.kfx_mesh_scratch_bytes(C.byref(vol), cell, None, 0, 0)
        assert need > 0 and need % 256 == 0
        # null pointers
        assert L.kfx_mesh_scratch_bytes(None, cell, None, 0, 0) == 0
        assert plan(L, None, cell, None, 0, 0, FAKE, need, tot) == E_NULL
        assert plan(L, vol, cell, None, 0, 0, None, need, tot) == E_NULL
        assert plan(L, vol, cell, None, 0, 0, FAKE, need, None) == E_NULL
        assert emit(L, None, cell, None, 0, 0, FAKE, need, tot) == E_NULL
        assert emit(L, vol, cell, None, 0, 0, None, need, tot) == E_NULL
        assert emit(L, vol, cell, None, 0, 0, FAKE, need, None) == E_NULL
        assert emit(L, vol, cell, None, 0, 0, FAKE, need, tot, out=None) == E_NULL
        nullvol = volume(40, 30, 50, cb)
        nullvol.ptr = None
        assert plan(L, nullvol, cell, None, 0, 0, FAKE, need, tot) == E_NULL
        # unknown cell kind
        for bad in (2, -1, 7):
            assert L.kfx_mesh_scratch_bytes(C.byref(vol), bad, None, 0, 0) == 0
            assert plan(L, vol, bad, None, 0, 0, FAKE, need, tot) == E_RANGE
            assert emit(L, vol, bad, None, 0, 0, FAKE, need, tot) == E_RANGE
        # too little scratch
        assert plan(L, vol, cell, None, 0, 0, FAKE, need - 1, tot) == E_SHAPE
        assert emit(L, vol, cell, None, 0, 0, FAKE, need - 1, tot) == E_SHAPE
        # a mesh of 2^32 / 3 triangles or more cannot be emitted
        big = (C.c_ulonglong * 2)(5, 2 ** 32 // 3)
        assert emit(L, vol, cell, None, 0, 0, FAKE, need, big) == E_RANGE
        # slabs of a 60-plane volume, 3 ranks of 20 planes: a ghost of 2 planes suffices, 1 does not
        D = 60
        for r in range(3):
            z0, z1 = 20 * r, 20 * r + 20
            for ghost, ok in ((2, True), (1, False), (0, False)):
                s0, s1 = max(z0 - ghost, 0), min(z1 + ghost, D)
                part = volume(40, 30, s1 - s0, cb)
                slab = _lib.KfxSlab(D, s0, -1.0, 1.0)
                n = L.kfx_mesh_scratch_bytes(C.byref(part), cell, C.byref(slab), z0, z1)
                if ok:
                    assert n > 0
                    assert plan(L, part, cell, slab, z0, z1, FAKE, n - 1, tot) == E_SHAPE
                else:
                    assert n == 0, (r, ghost)
                    assert plan(L, part, cell, slab, z0, z1, FAKE, 1 << 30, tot) == E_RANGE, (r, ghost)
                    assert emit(L, part, cell, slab, z0, z1, FAKE, 1 << 30, tot) == E_RANGE, (r, ghost)
        # the last rank's cubes end at plane D - 2: its stencil needs planes up to D - 1 only
        slab = _lib.KfxSlab(D, 38, -1.0, 1.0)
        assert L.kfx_mesh_scratch_bytes(C.byref(volume(40, 30, 22, cb)), cell, C.byref(slab), 40, 60) > 0
        assert L.kfx_mesh_scratch_bytes(C.byref(volume(40, 30, 21, cb)), cell, C.byref(slab), 40, 60) == 0
        # a slab that leaves the full volume
        slab = _lib.KfxSlab(D, 50, -1.0, 1.0)
        assert plan(L, volume(40, 30, 20, cb), cell, slab, 50, 60, FAKE, 1 << 30, tot) == E_SHAPE
        # one argument per broken rule of the volume, whole and as a slab (stored planes [10, 30) of 60): the exact code
        slab = _lib.KfxSlab(D, 10, -1.0, 1.0)
        for sl, lo, hi, min_d in ((None, 0, 0, 3), (slab, 12, 28, 1)):
            def broken(**kw):
                v = volume(40, 30, 20, cb)
                for k, val in kw.items():
                    setattr(v, k, val)
                return plan(L, v, cell, sl, lo, hi, FAKE, 1 << 30, tot)
            assert broken(ptr=None) == E_NULL and broken(ptr=FAKE + cb // 2) == E_ALIGN
            assert broken(w=2) == E_SHAPE and broken(h=2) == E_SHAPE and broken(d=min_d - 1) == E_SHAPE
            assert broken(w=65536, pitch=65536 * cb, img_pitch=65536 * cb * 30) == E_SHAPE and broken(h=65536, img_pitch=40 * cb * 65536) == E_SHAPE
            assert broken(d=65536) == E_SHAPE
            assert broken(pitch=39 * cb) == E_SHAPE and broken(img_pitch=40 * cb * 30 - cb) == E_SHAPE
        # a slab may store a single plane: with no cubes of its own to mesh it gets past the volume's checks, to the scratch pointer
        assert plan(L, volume(40, 30, 1, cb), cell, slab, 10, 10, None, 1 << 30, tot) == E_NULL
        assert L.kfx_mesh_scratch_bytes(C.byref(volume(40, 30, 1, cb)), cell, C.byref(slab), 10, 10) > 0
    # kfx_mc_count (fp32 cells): the same rules, dimensions from 3
    def count(**kw):
        v = volume(40, 30, 20, 8)
        for k, val in kw.items():
            setattr(v, k, val)
        return L.kfx_mc_count(C.byref(v), FAKE, None)
    assert count(ptr=None) == E_NULL and count(ptr=FAKE + 4) == E_ALIGN
    assert count(w=2) == E_SHAPE and count(h=2) == E_SHAPE and count(d=2) == E_SHAPE
    assert count(w=65536, pitch=65536 * 8, img_pitch=65536 * 8 * 30) == E_SHAPE and count(h=65536, img_pitch=40 * 8 * 65536) == E_SHAPE and count(d=65536) == E_SHAPE
    assert count(pitch=39 * 8) == E_SHAPE and count(img_pitch=40 * 8 * 30 - 8) == E_SHAPE
