"""Sparse brick snapshots (include/kfx_bricks.h) are exported by libkfx.so, have their ctypes bindings, stay out of the other headers,
refuse bad arguments before any HIP call, and size their scratch by the header's formula.  No GPU: the pointers below are never
dereferenced, and every call is a refusal, a host-only function or an empty list, which launches nothing."""
import ctypes as C
import os
import re

import kfx_testlib as T
from kangaroo_amd import _lib

E_NULL, E_SHAPE, E_ALIGN, E_RANGE = -1, -2, -3, -4
FAKE = 1 << 20   # an aligned address that nothing may touch
F32, F16, COLOR = 0, 1, 2
CELL_BYTES = {F32: 8, F16: 4, COLOR: 4}
R = C.byref
NAN = float("nan")

NAMES = ["kfx_bricks_pack", "kfx_bricks_plan", "kfx_bricks_scratch_bytes", "kfx_bricks_unpack"]


def declared(header):
    src = open(os.path.join(T.ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kfx_[a-z0-9_]+)\s*\(", src)))


def volume(w, h, d, cell_bytes):
    v = _lib.KfxVolume(w * cell_bytes, FAKE, w, h, w * cell_bytes * h, d)
    for i in range(3):
        v.boxmin[i], v.boxmax[i] = -1.0, 1.0
    return v


def formula(w, h, d):
    """include/kfx_bricks.h: 256 + round256(nb) + 2 * round256(4 * nblk)"""
    r256 = lambda n: (n + 255) // 256 * 256
    nb = ((w + 7) // 8) * ((h + 7) // 8) * ((d + 7) // 8)
    nblk = (nb + 255) // 256
    return 256 + r256(nb) + 2 * r256(4 * nblk)


def test_brick_symbols_are_exported_and_bound_and_stay_in_their_header():
    L = _lib.load()
    names = declared("kfx_bricks.h")
    assert names == NAMES, names
    for n in names:
        assert hasattr(L, n), "libkfx.so does not export %s" % n
        assert n in _lib.SIGNATURES, "python binding missing for %s" % n
    for other in ("kfx.h", "kfx_mesh.h", "kfx_shift.h"):
        assert not set(declared(other)) & set(names), other


def test_scratch_bytes_match_the_headers_formula():
    L = _lib.load()
    for dims in ((40, 24, 16), (8, 8, 8), (1, 1, 1), (7, 9, 65), (512, 512, 512), (41, 5, 6), (2048, 2048, 2048), (8, 8, 65535)):
        for cell, cb in CELL_BYTES.items():
            assert L.kfx_bricks_scratch_bytes(R(volume(*dims, cb)), cell) == formula(*dims), (dims, cell)
    assert formula(512, 512, 512) == 270592   # the figure the header quotes
    assert L.kfx_bricks_scratch_bytes(None, F32) == 0
    assert L.kfx_bricks_scratch_bytes(R(volume(40, 24, 16, 8)), 3) == 0 and L.kfx_bricks_scratch_bytes(R(volume(40, 24, 16, 8)), -1) == 0
    assert L.kfx_bricks_scratch_bytes(R(volume(0, 24, 16, 8)), F32) == 0
    assert L.kfx_bricks_scratch_bytes(R(volume(65535, 65535, 65535, 4)), F16) == 0   # more than 2^31 - 1 bricks


def test_every_refusal_gives_its_code_before_any_hip_call():
    L = _lib.load()
    n = C.c_ulonglong(123)
    for cell, cb in CELL_BYTES.items():
        vol = volume(40, 24, 16, cb)
        need = L.kfx_bricks_scratch_bytes(R(vol), cell)
        plan = lambda v, scratch, nbytes, out=n: L.kfx_bricks_plan(R(v) if v is not None else None, cell, NAN, scratch, nbytes, R(out) if out is not None else None, None)
        pack = lambda v, scratch, nbytes, live, ids, cells: L.kfx_bricks_pack(R(v) if v is not None else None, cell, NAN, scratch, nbytes, live, ids, cells, None)
        unpack = lambda v, ids, cells, cnt: L.kfx_bricks_unpack(R(v) if v is not None else None, cell, ids, cells, cnt, None)
        # null volume, null scratch, null n_live, null lists
        nullvol = volume(40, 24, 16, cb)
        nullvol.ptr = None
        for v in (None, nullvol):
            assert plan(v, FAKE, need) == E_NULL and pack(v, FAKE, need, 1, FAKE, FAKE) == E_NULL and unpack(v, FAKE, FAKE, 1) == E_NULL
        assert plan(vol, None, need) == E_NULL and plan(vol, FAKE, need, None) == E_NULL
        assert pack(vol, None, need, 1, FAKE, FAKE) == E_NULL
        assert pack(vol, FAKE, need, 1, None, FAKE) == E_NULL and pack(vol, FAKE, need, 1, FAKE, None) == E_NULL
        assert unpack(vol, None, FAKE, 1) == E_NULL and unpack(vol, FAKE, None, 1) == E_NULL
        # a short scratch, a misaligned scratch, misaligned lists
        assert plan(vol, FAKE, need - 1) == E_SHAPE and plan(vol, FAKE, 0) == E_SHAPE
        assert pack(vol, FAKE, need - 1, 1, FAKE, FAKE) == E_SHAPE
        for off in (1, 8, 16, 128):
            assert plan(vol, FAKE + off, need + 256) == E_ALIGN and pack(vol, FAKE + off, need + 256, 1, FAKE, FAKE) == E_ALIGN
        assert pack(vol, FAKE, need, 1, FAKE + 2, FAKE) == E_ALIGN and pack(vol, FAKE, need, 1, FAKE, FAKE + 8) == E_ALIGN
        assert unpack(vol, FAKE + 1, FAKE, 1) == E_ALIGN and unpack(vol, FAKE, FAKE + 4, 1) == E_ALIGN
        # more entries than the view has bricks cannot be a plan's; more than 2^31 - 1 entries are refused
        assert pack(vol, FAKE, need, 5 * 3 * 2 + 1, FAKE, FAKE) == E_RANGE
        assert unpack(vol, FAKE, FAKE, 1 << 31) == E_RANGE
        # the volume's own rules come first, each with its code
        def broken(**kw):
            v = volume(40, 24, 16, cb)
            for k, val in kw.items():
                setattr(v, k, val)
            return plan(v, FAKE, need), unpack(v, FAKE, FAKE, 1)
        assert broken(ptr=FAKE + cb // 2) == (E_ALIGN, E_ALIGN)
        for kw in (dict(w=0), dict(h=0), dict(d=0), dict(d=65536), dict(pitch=39 * cb), dict(img_pitch=40 * cb * 24 - cb)):
            assert broken(**kw) == (E_SHAPE, E_SHAPE), kw
        # an empty list launches nothing and needs nothing
        assert unpack(vol, None, None, 0) == 0 and unpack(vol, FAKE, FAKE, 0) == 0
    assert n.value == 123   # no refusal wrote the count
    vol = volume(40, 24, 16, 8)
    for bad in (3, -1, 7):
        assert L.kfx_bricks_plan(R(vol), bad, NAN, FAKE, 1 << 20, R(n), None) == E_RANGE
        assert L.kfx_bricks_pack(R(vol), bad, NAN, FAKE, 1 << 20, 1, FAKE, FAKE, None) == E_RANGE
        assert L.kfx_bricks_unpack(R(vol), bad, FAKE, FAKE, 1, None) == E_RANGE
        assert L.kfx_bricks_unpack(R(vol), bad, FAKE, FAKE, 0, None) == E_RANGE   # (the kind is checked before the list is looked at)
