"""The indexed brick mesh (include/kfx_mesh_bricks_index.h) is exported by libkfx.so, has its ctypes bindings, stays out of the other
headers, refuses bad arguments before any HIP call, and sizes its index scratch from the brick count and the plan's totals alone, by
the header's formula.  No GPU: the pointers below are never dereferenced, and every call is a refusal, a host-only function or an
empty mesh, which launches nothing.  The host-check program (scripts/mesh_bricks_index_host_check.cpp) builds with a plain host
compiler under the address and undefined-behaviour sanitizers, as a stand-alone executable, and passes."""
import ctypes as C
import os
import re
import subprocess

import kfx_testlib as T
from kangaroo_amd import _lib

E_NULL, E_SHAPE, E_ALIGN, E_RANGE = -1, -2, -3, -4
FAKE = 1 << 20   # an aligned address that nothing may touch
F32, F16, COLOR = 0, 1, 2
R = C.byref
U2 = C.c_ulonglong * 2

NAMES = ["kfx_mesh_bricks_emit_indexed", "kfx_mesh_bricks_index_plan", "kfx_mesh_bricks_index_scratch_bytes"]


def declared(header):
    src = open(os.path.join(T.ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kfx_[a-z0-9_]+)\s*\(", src)))


def frame(w, h, d):
    """a frame: dimensions and a box, no storage"""
    v = _lib.KfxVolume(0, None, w, h, 0, d)
    for i in range(3):
        v.boxmin[i], v.boxmax[i] = -1.0, 1.0
    return v


def formula(n, a):
    """include/kfx_mesh_bricks_index.h: 256 + round256(8 A) + 3 round256(4 A) + round256(4 n) + round256(8 xblk) + round256(16 xblk)"""
    r256 = lambda v: (v + 255) // 256 * 256
    xblk = (a + 255) // 256
    return 256 + r256(8 * a) + 3 * r256(4 * a) + r256(4 * n) + r256(8 * xblk) + r256(16 * xblk)


def test_indexed_brick_mesh_symbols_are_exported_and_bound_and_stay_in_their_header():
    L = _lib.load()
    names = declared("kfx_mesh_bricks_index.h")
    assert names == NAMES, names
    for n in names:
        assert hasattr(L, n), "libkfx.so does not export %s" % n
        assert n in _lib.SIGNATURES, "python binding missing for %s" % n
    for other in ("kfx.h", "kfx_mesh.h", "kfx_mesh_index.h", "kfx_bricks.h", "kfx_mesh_bricks.h"):
        assert not set(declared(other)) & set(names), other


def test_index_scratch_bytes_match_the_headers_formula_and_know_no_frame():
    L = _lib.load()
    for n in (0, 1, 255, 256, 257, 800, 70000):
        for a in (0, 1, 255, 256, 257, 65536, 2200000):
            assert L.kfx_mesh_bricks_index_scratch_bytes(n, U2(a, 3 * a)) == formula(n, a), (n, a)
    assert formula(0, 0) == 256 and formula(60, 1000) == 21504
    # the triangles do not enter, only their range does
    assert L.kfx_mesh_bricks_index_scratch_bytes(60, U2(1000, 1000)) == L.kfx_mesh_bricks_index_scratch_bytes(60, U2(1000, 5000)) == 21504
    # about 20 bytes per active cube
    assert 20 * 2200000 < formula(9000, 2200000) < 20.2 * 2200000
    # refused: null totals, counts or totals out of range
    assert L.kfx_mesh_bricks_index_scratch_bytes(60, None) == 0
    assert L.kfx_mesh_bricks_index_scratch_bytes(1 << 31, U2(1, 1)) == 0
    assert L.kfx_mesh_bricks_index_scratch_bytes(60, U2(5, 4)) == 0 and L.kfx_mesh_bricks_index_scratch_bytes(60, U2(1, 2 ** 32 // 3)) == 0
    assert L.kfx_mesh_bricks_index_scratch_bytes((1 << 31) - 1, U2(1, 2 ** 32 // 3 - 1)) == formula((1 << 31) - 1, 1)
    # a 40 x 24 x 16 frame and a 4096^3 frame with the same n and totals: an index plan accepts exactly these bytes for both
    n, tot = 30, U2(500, 1200)
    need, xneed = L.kfx_mesh_bricks_scratch_bytes(n, 0), L.kfx_mesh_bricks_index_scratch_bytes(n, tot)
    nv = C.c_ulonglong(77)
    for dims in ((40, 24, 16), (4096, 4096, 4096)):
        call = lambda xs, xb: L.kfx_mesh_bricks_index_plan(R(frame(*dims)), F32, FAKE, FAKE, n, FAKE, need, tot, xs, xb, R(nv), None)
        assert call(FAKE, xneed - 1) == E_SHAPE
        assert call(FAKE + 8, xneed) == E_ALIGN   # (large enough: the next check)
    assert nv.value == 77


def test_every_refusal_gives_its_code_before_any_hip_call():
    L = _lib.load()
    good = frame(40, 24, 16)
    n, nc = 30, 12
    totals = U2(500, 1200)
    V = 700
    need, need_c = L.kfx_mesh_bricks_scratch_bytes(n, 0), L.kfx_mesh_bricks_scratch_bytes(n, nc)
    xneed = L.kfx_mesh_bricks_index_scratch_bytes(n, totals)
    nv = C.c_ulonglong(77)

    def plan(f=good, cell=F32, ids=FAKE, cells=FAKE, cnt=n, scratch=FAKE, nbytes=need, tot=totals, xs=FAKE, xb=xneed, out=nv):
        return L.kfx_mesh_bricks_index_plan(R(f) if f is not None else None, cell, ids, cells, cnt, scratch, nbytes, tot, xs, xb,
                                            R(out) if out is not None else None, None)

    def emit(f=good, cell=F32, ids=FAKE, cells=FAKE, cnt=n, cids=FAKE, ccells=FAKE, ccnt=nc, scratch=FAKE, nbytes=need_c, xs=FAKE, xb=xneed,
             tot=totals, v=V, outs=(FAKE, FAKE, FAKE, FAKE)):
        return L.kfx_mesh_bricks_emit_indexed(R(f) if f is not None else None, cell, ids, cells, cnt, cids, ccells, ccnt, scratch, nbytes, xs, xb,
                                              tot, v, *outs, None)

    # null pointers
    assert plan(f=None) == E_NULL and emit(f=None) == E_NULL
    assert plan(ids=None) == E_NULL and plan(cells=None) == E_NULL and plan(scratch=None) == E_NULL and plan(tot=None) == E_NULL
    assert plan(xs=None) == E_NULL and plan(out=None) == E_NULL
    assert emit(ids=None) == E_NULL and emit(cells=None) == E_NULL and emit(scratch=None) == E_NULL and emit(tot=None) == E_NULL
    assert emit(cids=None) == E_NULL and emit(ccells=None) == E_NULL and emit(xs=None) == E_NULL
    for k in (0, 1, 3):   # verts, norms, faces (colours may be null: no colours are written then)
        outs = [FAKE] * 4
        outs[k] = None
        assert emit(outs=tuple(outs)) == E_NULL, k
    # an unknown cell kind (the colour kind is no SDF kind)
    for bad in (COLOR, 3, -1):
        assert plan(cell=bad) == E_RANGE and emit(cell=bad) == E_RANGE
    # more than 2^31 - 1 bricks in the frame, or entries in a list
    assert plan(f=frame(65535, 65535, 65535)) == E_RANGE and emit(f=frame(65535, 65535, 65535)) == E_RANGE
    assert plan(cnt=1 << 31, nbytes=1 << 62, xb=1 << 62) == E_RANGE and emit(cnt=1 << 31, nbytes=1 << 62, xb=1 << 62) == E_RANGE
    assert emit(ccnt=1 << 31, nbytes=1 << 62) == E_RANGE
    # frame dimensions the dense kfx_mesh_plan would refuse
    for dims in ((2, 24, 16), (40, 0, 16), (40, 24, 1), (65536, 24, 16), (40, 24, 65536)):
        assert plan(f=frame(*dims)) == E_SHAPE and emit(f=frame(*dims)) == E_SHAPE, dims
    # too little of either scratch: the index plan needs the plan's bytes without colour, the emit those with
    assert plan(nbytes=need - 1) == E_SHAPE and plan(nbytes=0) == E_SHAPE and plan(xb=xneed - 1) == E_SHAPE and plan(xb=0) == E_SHAPE
    assert emit(nbytes=need_c - 1) == E_SHAPE and emit(nbytes=need) == E_SHAPE and emit(xb=xneed - 1) == E_SHAPE
    # misalignment: both scratches 256, ids 4, cells 16, outputs 4
    for off in (1, 8, 16, 128):
        assert plan(scratch=FAKE + off, nbytes=need + 256) == E_ALIGN and emit(scratch=FAKE + off, nbytes=need_c + 256) == E_ALIGN
        assert plan(xs=FAKE + off, xb=xneed + 256) == E_ALIGN and emit(xs=FAKE + off, xb=xneed + 256) == E_ALIGN
    assert plan(ids=FAKE + 2) == E_ALIGN and plan(cells=FAKE + 8) == E_ALIGN
    assert emit(ids=FAKE + 1) == E_ALIGN and emit(cells=FAKE + 4) == E_ALIGN and emit(cids=FAKE + 2) == E_ALIGN and emit(ccells=FAKE + 8) == E_ALIGN
    for k in range(4):
        outs = [FAKE] * 4
        outs[k] = FAKE + 2
        assert emit(outs=tuple(outs)) == E_ALIGN, k
    # totals that no plan can have made, and a V no index plan can have made of them, are refused before a scratch is read back
    big = 1 << 40
    for bad in (U2(5, 4), U2(1, 2 ** 32 // 3)):
        assert plan(tot=bad, xb=big) == E_RANGE and emit(tot=bad, xb=big) == E_RANGE
    assert emit(v=3 * 1200 + 1) == E_RANGE
    assert nv.value == 77 and (totals[0], totals[1]) == (500, 1200)   # no refusal wrote anything

    # no bricks: totals (0, 0) only, V = 0, nothing launched, the lists may be null
    zero = U2(0, 0)
    xzero = L.kfx_mesh_bricks_index_scratch_bytes(0, zero)
    assert xzero == 256
    assert plan(ids=None, cells=None, cnt=0, nbytes=256, tot=zero, xb=xzero) == 0 and nv.value == 0
    nv.value = 77
    assert plan(ids=None, cells=None, cnt=0, nbytes=256, tot=U2(1, 1), xb=1 << 20) == E_RANGE and nv.value == 77
    assert emit(ids=None, cells=None, cnt=0, cids=None, ccells=None, ccnt=0, nbytes=256, tot=zero, v=0, xb=xzero) == 0
    assert emit(ids=None, cells=None, cnt=0, cids=None, ccells=None, ccnt=0, nbytes=256, tot=U2(1, 1), v=0, xb=1 << 20) == E_RANGE
    assert emit(ids=None, cells=None, cnt=0, cids=None, ccells=None, ccnt=0, nbytes=256, tot=zero, v=1, xb=xzero) == E_RANGE
    # a mesh without cubes: V = 0, no launch, and the emit needs no outputs
    assert plan(tot=zero, xb=L.kfx_mesh_bricks_index_scratch_bytes(n, zero)) == 0 and nv.value == 0
    assert emit(tot=zero, v=0, outs=(None,) * 4) == 0


def test_the_host_check_program_builds_and_passes_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "mesh_bricks_index_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(T.ROOT, "scripts", "mesh_bricks_index_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "mesh_bricks_index_host_check: ok" in out.stdout, out.stdout + out.stderr
