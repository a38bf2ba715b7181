"""The brick pool (include/kfx_brick_pool.h) is exported by libkfx.so, has its ctypes bindings, stays out of the other headers, refuses
bad arguments before any HIP call -- each rule with its code, in the header's order -- and sizes a pool and its scratch by the header's
formulas.  No GPU: the pointers below are never dereferenced and every call is a refusal or a host-only function.  The host-check
program (scripts/brick_pool_host_check.cpp) builds with a plain host compiler, and under the host sanitizers, and passes."""
import ctypes as C
import os
import re
import subprocess

import pytest

import kfx_testlib as T
from kangaroo_amd import _lib

E_NULL, E_SHAPE, E_ALIGN, E_RANGE = -1, -2, -3, -4
FAKE = 1 << 20   # an aligned address that nothing may touch
F32, F16, COLOR = 0, 1, 2
CB = {F32: 8, F16: 4, COLOR: 4}
R = C.byref
INT_MAX = (1 << 31) - 1

NAMES = ["kfx_brick_pool_bytes", "kfx_brick_pool_discard", "kfx_brick_pool_gather", "kfx_brick_pool_init", "kfx_brick_pool_restore",
         "kfx_brick_pool_scratch_bytes", "kfx_brick_pool_spill", "kfx_brick_pool_stats"]


def declared(header):
    src = open(os.path.join(T.ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kfx_[a-z0-9_]+)\s*\(", src)))


def r256(v):
    return (v + 255) // 256 * 256


def pool_formula(cell, capacity):
    """include/kfx_brick_pool.h: 256 + round256(16 capacity) + round256(4 capacity) + 512 cb capacity"""
    return 256 + r256(16 * capacity) + r256(4 * capacity) + 512 * CB[cell] * capacity


def scratch_formula(nb, capacity):
    """include/kfx_brick_pool.h: 256 + round256(n) + 2 round256(4 nblk) + round256(4 n), n = max(bricks of the view, capacity)"""
    n = max(nb, capacity)
    nblk = (n + 255) // 256
    return 256 + r256(n) + 2 * r256(4 * nblk) + r256(4 * n)


def volume(cell, w=40, h=24, d=16, pitch=None, img_pitch=None, ptr=FAKE):
    cb = CB[cell]
    pitch = w * cb if pitch is None else pitch
    return _lib.KfxVolume(pitch, ptr, w, h, pitch * h if img_pitch is None else img_pitch, d)


def i3(*v):
    return (C.c_int * 3)(*v)


def test_brick_pool_symbols_are_exported_and_bound_and_stay_in_their_header():
    L = _lib.load()
    names = declared("kfx_brick_pool.h")
    assert names == NAMES, names
    for n in names:
        assert hasattr(L, n), "libkfx.so does not export %s" % n
        assert n in _lib.SIGNATURES, "python binding missing for %s" % n
    for other in ("kfx.h", "kfx_mesh.h", "kfx_shift.h", "kfx_bricks.h", "kfx_mesh_bricks.h", "kfx_raycast_bricks.h", "kfx_color.h", "kfx_extras.h"):
        assert not set(declared(other)) & set(names), other
    text = open(os.path.join(T.ROOT, "include", "kfx_brick_pool.h")).read()
    assert "256 + round256(16 capacity) + round256(4 capacity) + 512 cb capacity" in text
    assert "256 + round256(n) + 2 * round256(4 * nblk) + round256(4 * n)" in text


@pytest.mark.parametrize("capacity", [1, 255, 256, 257, 65537])
def test_pool_and_scratch_bytes_equal_the_documented_formulas(capacity):
    L = _lib.load()
    for cell in (F32, F16, COLOR):
        assert L.kfx_brick_pool_bytes(cell, capacity) == pool_formula(cell, capacity), (cell, capacity)
        # views of 1, 30, 300 and 66 000 bricks: below and above the capacities, partial last bricks, more than one scan block
        for dims, nb in (((8, 8, 8), 1), ((40, 24, 16), 30), ((33, 17, 9), 30), ((80, 48, 40), 300), ((8, 8 * 66, 8 * 1000), 66000)):
            got = L.kfx_brick_pool_scratch_bytes(R(volume(cell, *dims)), cell, capacity)
            assert got == scratch_formula(nb, capacity), (cell, capacity, dims)
    assert pool_formula(F32, 1) == 256 + 256 + 256 + 4096 and scratch_formula(1, 1) == 256 + 256 + 2 * 256 + 256
    assert scratch_formula(30, 257) == 256 + 512 + 2 * 256 + 1280


def test_refused_sizes_are_zero():
    L = _lib.load()
    for cell, capacity in ((3, 16), (-1, 16), (F32, 0), (F16, 1 << 31), (COLOR, 1 << 40)):
        assert L.kfx_brick_pool_bytes(cell, capacity) == 0
        assert L.kfx_brick_pool_scratch_bytes(R(volume(F32)), cell, capacity) == 0
    assert L.kfx_brick_pool_bytes(F32, INT_MAX) == pool_formula(F32, INT_MAX)
    assert L.kfx_brick_pool_scratch_bytes(None, F32, 16) == 0 and L.kfx_brick_pool_scratch_bytes(R(volume(F32, ptr=None)), F32, 16) == 0
    assert L.kfx_brick_pool_scratch_bytes(R(volume(F32, w=0)), F32, 16) == 0
    assert L.kfx_brick_pool_scratch_bytes(R(volume(F32, w=65535, h=65535, d=65535, pitch=1 << 20, img_pitch=1 << 40)), F32, 16) == 0   # > 2^31 - 1 bricks


def test_every_refusal_gives_its_code_in_the_headers_order_before_any_hip_call():
    L = _lib.load()
    cap = 64
    pool_need = L.kfx_brick_pool_bytes(F32, cap)
    good = volume(F32)
    need = L.kfx_brick_pool_scratch_bytes(R(good), F32, cap)
    key0 = i3(-3, 5, 1000)
    ref = lambda x: R(x) if x is not None else None

    def spill(pool=FAKE, nbytes=pool_need, cell=F32, capacity=cap, view=good, key=key0, scratch=FAKE, sbytes=need):
        return L.kfx_brick_pool_spill(pool, nbytes, cell, capacity, ref(view), float("nan"), key, scratch, sbytes, None)

    def restore(pool=FAKE, nbytes=pool_need, cell=F32, capacity=cap, view=good, key=key0, scratch=FAKE, sbytes=need):
        return L.kfx_brick_pool_restore(pool, nbytes, cell, capacity, ref(view), key, scratch, sbytes, None)

    def discard(pool=FAKE, nbytes=pool_need, cell=F32, capacity=cap, nb=i3(5, 3, 2), key=key0, scratch=FAKE, sbytes=need):
        return L.kfx_brick_pool_discard(pool, nbytes, cell, capacity, nb, key, scratch, sbytes, None)

    def init(pool=FAKE, nbytes=pool_need, cell=F32, capacity=cap):
        return L.kfx_brick_pool_init(pool, nbytes, cell, capacity, None)

    out = (C.c_ulonglong * 4)()

    def stats(pool=FAKE, nbytes=pool_need, cell=F32, capacity=cap, o=out):
        return L.kfx_brick_pool_stats(pool, nbytes, cell, capacity, o, None)

    def gather(pool=FAKE, nbytes=pool_need, cell=F32, capacity=cap, slots=FAKE, n=4, cells=FAKE):
        return L.kfx_brick_pool_gather(pool, nbytes, cell, capacity, slots, n, cells, None)

    for call in (spill, restore):
        # null pool, view, key0, scratch
        assert call(pool=None) == E_NULL and call(view=None) == E_NULL and call(view=volume(F32, ptr=None)) == E_NULL
        assert call(key=None) == E_NULL and call(scratch=None) == E_NULL
        # the cell kind, then the capacity
        for bad in (3, -1, 7):
            assert call(cell=bad) == E_RANGE
        assert call(capacity=0) == E_RANGE and call(capacity=1 << 31, nbytes=1 << 62) == E_RANGE
        # the pool: too small, then misaligned
        assert call(nbytes=pool_need - 1) == E_SHAPE and call(nbytes=0) == E_SHAPE
        for off in (1, 8, 16, 128):
            assert call(pool=FAKE + off) == E_ALIGN
        # the view: the volume's own rules
        for axis in "whd":
            assert call(view=volume(F32, **{axis: 0})) == E_SHAPE and call(view=volume(F32, **{axis: 65536})) == E_SHAPE, axis
        assert call(view=volume(F32, pitch=40 * 8 - 8, img_pitch=40 * 8 * 24)) == E_SHAPE and call(view=volume(F32, img_pitch=40 * 8 * 24 - 8)) == E_SHAPE
        assert call(view=volume(F32, ptr=FAKE + 4)) == E_ALIGN
        assert call(view=volume(F32, w=65535, h=65535, d=65535, pitch=1 << 20, img_pitch=1 << 40), sbytes=1 << 62) == E_RANGE
        # the scratch: too small (by the view's bricks or by the capacity, whichever are more), then misaligned
        assert call(sbytes=need - 1) == E_SHAPE and call(sbytes=0) == E_SHAPE
        big = L.kfx_brick_pool_bytes(F32, 1000)
        assert call(capacity=1000, nbytes=big, sbytes=need) == E_SHAPE
        assert call(capacity=1000, nbytes=big, sbytes=scratch_formula(30, 1000) - 1) == E_SHAPE
        assert call(capacity=1000, nbytes=big, sbytes=scratch_formula(30, 1000), key=i3(INT_MAX, 0, 0)) == E_RANGE   # (accepted: the next check)
        for off in (1, 8, 16, 128):
            assert call(scratch=FAKE + off, sbytes=need + 256) == E_ALIGN
        # a key range that leaves int32: the view has 5 x 3 x 2 bricks
        assert call(key=i3(INT_MAX - 3, 0, 0)) == E_RANGE and call(key=i3(0, INT_MAX - 1, 0)) == E_RANGE and call(key=i3(0, 0, INT_MAX)) == E_RANGE
        # the order: nulls, kind, capacity, pool size, pool alignment, view, scratch size, scratch alignment, keys
        assert call(scratch=None, cell=9) == E_NULL and call(cell=9, capacity=0) == E_RANGE and call(capacity=0, nbytes=0) == E_RANGE
        assert call(nbytes=0, pool=FAKE + 8) == E_SHAPE and call(pool=FAKE + 8, view=volume(F32, w=0)) == E_ALIGN
        assert call(view=volume(F32, w=0), sbytes=0) == E_SHAPE and call(view=volume(F32, ptr=FAKE + 4), sbytes=0) == E_ALIGN
        assert call(sbytes=0, scratch=FAKE + 8) == E_SHAPE and call(scratch=FAKE + 8, key=i3(INT_MAX, 0, 0)) == E_ALIGN
    # the cell kind decides the cell size of the view's rules: a 4-byte aligned volume is a usable half-cell or colour view
    half = L.kfx_brick_pool_bytes(F16, cap)
    assert spill(cell=F16, nbytes=half, view=volume(F16, ptr=FAKE + 4), key=i3(INT_MAX, 0, 0)) == E_RANGE
    assert restore(cell=COLOR, nbytes=half, view=volume(COLOR, ptr=FAKE + 2)) == E_ALIGN

    # discard: a key box in place of the view
    assert discard(pool=None) == E_NULL and discard(nb=None) == E_NULL and discard(key=None) == E_NULL and discard(scratch=None) == E_NULL
    assert discard(cell=5) == E_RANGE and discard(capacity=0) == E_RANGE
    assert discard(nbytes=pool_need - 1) == E_SHAPE and discard(pool=FAKE + 64) == E_ALIGN
    assert discard(nb=i3(0, 3, 2)) == E_SHAPE and discard(nb=i3(5, -1, 2)) == E_SHAPE
    assert discard(nb=i3(INT_MAX, INT_MAX, 2)) == E_RANGE and discard(nb=i3(1 << 16, 1 << 15, 1)) == E_RANGE
    assert discard(sbytes=scratch_formula(0, cap) - 1) == E_SHAPE and discard(scratch=FAKE + 16) == E_ALIGN
    assert discard(key=i3(0, INT_MAX - 1, 0)) == E_RANGE
    assert discard(nb=i3(0, 1, 1), sbytes=0) == E_SHAPE and discard(pool=FAKE + 64, nb=i3(0, 1, 1)) == E_ALIGN
    assert discard(sbytes=scratch_formula(0, cap), key=i3(INT_MAX, 0, 0)) == E_RANGE   # (the capacity's scratch is enough: the next check)

    # init, stats, gather
    assert init(pool=None) == E_NULL and init(cell=4) == E_RANGE and init(capacity=0) == E_RANGE and init(capacity=INT_MAX + 1) == E_RANGE
    assert init(nbytes=pool_need - 1) == E_SHAPE and init(pool=FAKE + 32) == E_ALIGN and init(pool=FAKE + 32, nbytes=0) == E_SHAPE
    assert stats(pool=None) == E_NULL and stats(o=None) == E_NULL and stats(cell=-2) == E_RANGE and stats(capacity=0) == E_RANGE
    assert stats(nbytes=pool_need - 1) == E_SHAPE and stats(pool=FAKE + 1) == E_ALIGN
    assert gather(pool=None) == E_NULL and gather(cell=3) == E_RANGE and gather(capacity=0) == E_RANGE
    assert gather(nbytes=pool_need - 1) == E_SHAPE and gather(pool=FAKE + 128) == E_ALIGN
    assert gather(n=1 << 31) == E_RANGE and gather(slots=None) == E_NULL and gather(cells=None) == E_NULL
    assert gather(slots=FAKE + 2) == E_ALIGN and gather(cells=FAKE + 8) == E_ALIGN
    assert gather(n=0, slots=None, cells=None) == 0   # nothing to move: nothing is asked of the lists, nothing is launched


def test_the_host_check_program_builds_plainly_and_under_the_host_sanitizers_and_passes(tmp_path):
    src = os.path.join(T.ROOT, "scripts", "brick_pool_host_check.cpp")
    # (the sanitizers' runtimes linked into the program: it runs as it is, whatever else the process environment loads)
    sanitize = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    for name, flags in (("plain", []), ("sanitized", sanitize)):
        exe = str(tmp_path / ("brick_pool_host_check_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + flags + [src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "brick_pool_host_check: ok" in out.stdout, name + ": " + out.stdout + out.stderr
