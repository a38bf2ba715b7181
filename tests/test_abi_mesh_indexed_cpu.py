"""The indexed mesh extraction (include/kfx_mesh_index.h) is exported by libkfx.so, has its ctypes bindings, and refuses bad arguments
before any HIP call, in the order of kfx_mesh.h: null pointers, then an unknown cell kind / totals out of range / a slab whose stored
planes do not cover its cubes, then too little scratch.  No GPU: the pointers below are never dereferenced."""
import ctypes as C
import os
import re

import kfx_testlib as T
from kangaroo_amd import _lib
from test_abi_mesh_cpu import E_ALIGN, E_NULL, E_RANGE, E_SHAPE, FAKE, volume


def test_indexed_mesh_symbols_are_exported_and_bound():
    src = open(os.path.join(T.ROOT, "include", "kfx_mesh_index.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(kfx_[a-z0-9_]+)\s*\(", src)))
    assert names == ["kfx_mesh_emit_indexed", "kfx_mesh_index_plan", "kfx_mesh_index_scratch_bytes"], names
    L = _lib.load()
    for n in names:
        assert hasattr(L, n), "libkfx.so does not export %s" % n
        assert n in _lib.SIGNATURES, "python binding missing for %s" % n


def ref(x):
    return C.byref(x) if x is not None else None


def bytes_(L, vol, cell, slab, lo, hi, totals):
    return L.kfx_mesh_index_scratch_bytes(ref(vol), cell, ref(slab), lo, hi, totals)


def plan(L, vol, cell, slab, lo, hi, scratch, nbytes, totals, xscratch, xbytes, nv):
    return L.kfx_mesh_index_plan(ref(vol), cell, ref(slab), lo, hi, scratch, nbytes, totals, xscratch, xbytes, nv, None)


def emit(L, vol, cell, slab, lo, hi, xscratch, xbytes, totals, nv, out=FAKE):
    return L.kfx_mesh_emit_indexed(ref(vol), cell, ref(slab), lo, hi, None, xscratch, xbytes, totals, nv, out, out, None, out, None)


def test_indexed_mesh_entry_points_refuse_before_any_hip_call():
    L = _lib.load()
    tot = (C.c_ulonglong * 2)(1000, 2000)
    nv = C.c_ulonglong(7)
    for cell, cb in ((0, 8), (1, 4)):
        vol = volume(40, 30, 50, cb)
        need = L.kfx_mesh_scratch_bytes(C.byref(vol), cell, None, 0, 0)
        xneed = bytes_(L, vol, cell, None, 0, 0, tot)
        # 20 bytes per active cube, the scan partials of ceil(1000 / 256) blocks, the header; every part 256-byte aligned
        assert xneed % 256 == 0 and 20 * 1000 + 24 * 4 + 256 <= xneed <= 20 * 1000 + 24 * 4 + 256 + 6 * 255
        none = (C.c_ulonglong * 2)(0, 0)
        assert bytes_(L, vol, cell, None, 0, 0, none) >= 256
        # null pointers
        assert bytes_(L, None, cell, None, 0, 0, tot) == 0 and bytes_(L, vol, cell, None, 0, 0, None) == 0
        assert plan(L, None, cell, None, 0, 0, FAKE, need, tot, FAKE, xneed, C.byref(nv)) == E_NULL
        assert plan(L, vol, cell, None, 0, 0, None, need, tot, FAKE, xneed, C.byref(nv)) == E_NULL
        assert plan(L, vol, cell, None, 0, 0, FAKE, need, None, FAKE, xneed, C.byref(nv)) == E_NULL
        assert plan(L, vol, cell, None, 0, 0, FAKE, need, tot, None, xneed, C.byref(nv)) == E_NULL
        assert plan(L, vol, cell, None, 0, 0, FAKE, need, tot, FAKE, xneed, None) == E_NULL
        assert emit(L, None, cell, None, 0, 0, FAKE, xneed, tot, 1500) == E_NULL
        assert emit(L, vol, cell, None, 0, 0, None, xneed, tot, 1500) == E_NULL
        assert emit(L, vol, cell, None, 0, 0, FAKE, xneed, None, 1500) == E_NULL
        assert emit(L, vol, cell, None, 0, 0, FAKE, xneed, tot, 1500, out=None) == E_NULL
        nullvol = volume(40, 30, 50, cb)
        nullvol.ptr = None
        assert plan(L, nullvol, cell, None, 0, 0, FAKE, need, tot, FAKE, xneed, C.byref(nv)) == E_NULL
        # unknown cell kind
        for bad in (2, -1, 7):
            assert bytes_(L, vol, bad, None, 0, 0, tot) == 0
            assert plan(L, vol, bad, None, 0, 0, FAKE, need, tot, FAKE, xneed, C.byref(nv)) == E_RANGE
            assert emit(L, vol, bad, None, 0, 0, FAKE, xneed, tot, 1500) == E_RANGE
        # totals out of range: 2^32 / 3 triangles or more, more cubes than triangles, more vertices than 3 T -- before the scratch sizes
        for a, t in ((5, 2 ** 32 // 3), (2001, 2000)):
            big = (C.c_ulonglong * 2)(a, t)
            assert bytes_(L, vol, cell, None, 0, 0, big) == 0
            assert plan(L, vol, cell, None, 0, 0, FAKE, 0, big, FAKE, 0, C.byref(nv)) == E_RANGE
            assert emit(L, vol, cell, None, 0, 0, FAKE, 0, big, 10) == E_RANGE
        assert emit(L, vol, cell, None, 0, 0, FAKE, xneed, tot, 3 * 2000 + 1) == E_RANGE
        # misaligned scratch
        assert plan(L, vol, cell, None, 0, 0, FAKE + 128, need, tot, FAKE, xneed, C.byref(nv)) == E_ALIGN
        assert plan(L, vol, cell, None, 0, 0, FAKE, need, tot, FAKE + 128, xneed, C.byref(nv)) == E_ALIGN
        assert emit(L, vol, cell, None, 0, 0, FAKE + 128, xneed, tot, 1500) == E_ALIGN
        # too little scratch, either one
        assert plan(L, vol, cell, None, 0, 0, FAKE, need - 1, tot, FAKE, xneed, C.byref(nv)) == E_SHAPE
        assert plan(L, vol, cell, None, 0, 0, FAKE, need, tot, FAKE, xneed - 1, C.byref(nv)) == E_SHAPE
        assert emit(L, vol, cell, None, 0, 0, FAKE, xneed - 1, tot, 1500) == E_SHAPE
        # nothing to mesh: no launch, no vertices
        nv.value = 7
        assert plan(L, vol, cell, None, 0, 0, FAKE, need, none, FAKE, 1 << 20, C.byref(nv)) == 0 and nv.value == 0
        assert emit(L, vol, cell, None, 0, 0, FAKE, 1 << 20, none, 0, out=None) == 0
        # slabs of a 60-plane volume, 3 ranks of 20 planes: a ghost of 2 planes suffices, 1 does not
        D = 60
        for r in range(3):
            z0, z1 = 20 * r, 20 * r + 20
            for ghost, ok in ((2, True), (1, False), (0, False)):
                s0, s1 = max(z0 - ghost, 0), min(z1 + ghost, D)
                part = volume(40, 30, s1 - s0, cb)
                slab = _lib.KfxSlab(D, s0, -1.0, 1.0)
                n = bytes_(L, part, cell, slab, z0, z1, tot)
                if ok:
                    assert n == xneed
                    assert emit(L, part, cell, slab, z0, z1, FAKE, n - 1, tot, 1500) == E_SHAPE
                else:
                    assert n == 0, (r, ghost)
                    assert plan(L, part, cell, slab, z0, z1, FAKE, 1 << 30, tot, FAKE, 1 << 30, C.byref(nv)) == E_RANGE, (r, ghost)
                    assert emit(L, part, cell, slab, z0, z1, FAKE, 1 << 30, tot, 1500) == E_RANGE, (r, ghost)
        # a slab that leaves the full volume
        slab = _lib.KfxSlab(D, 50, -1.0, 1.0)
        assert plan(L, volume(40, 30, 20, cb), cell, slab, 50, 60, FAKE, 1 << 30, tot, FAKE, 1 << 30, C.byref(nv)) == E_SHAPE
        assert emit(L, volume(40, 30, 20, cb), cell, slab, 50, 60, FAKE, 1 << 30, tot, 1500) == E_SHAPE
