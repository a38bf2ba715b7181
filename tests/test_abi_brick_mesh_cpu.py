"""The brick mesh (include/kfx_mesh_bricks.h) is exported by libkfx.so, has its ctypes bindings, stays out of the other headers, refuses
bad arguments before any HIP call, and sizes its scratch from the brick counts alone, by the header's formula.  No GPU: the pointers
below are never dereferenced, and every call is a refusal, a host-only function or an empty list, which launches nothing.  The
host-check program (scripts/mesh_bricks_host_check.cpp) builds with a plain host compiler and passes."""
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

NAMES = ["kfx_mesh_bricks_emit", "kfx_mesh_bricks_plan", "kfx_mesh_bricks_scratch_bytes"]


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


def formula(n, n_color=0):
    """include/kfx_mesh_bricks.h: 256 + round256(108 n) + round256(4 n) + round256(8 nblk) + round256(16 nblk) [+ round256(108 n)]"""
    r256 = lambda v: (v + 255) // 256 * 256
    nblk = (n + 255) // 256
    return 256 + r256(108 * n) + r256(4 * n) + r256(8 * nblk) + r256(16 * nblk) + (r256(108 * n) if n_color else 0)


def test_brick_mesh_symbols_are_exported_and_bound_and_stay_in_their_header():
    L = _lib.load()
    names = declared("kfx_mesh_bricks.h")
    assert names == NAMES, names
    for n in names:
        assert hasattr(L, n), "libkfx.so does not export %s" % n
        assert n in _lib.SIGNATURES, "python binding missing for %s" % n
    for other in ("kfx.h", "kfx_mesh.h", "kfx_mesh_index.h", "kfx_shift.h", "kfx_bricks.h"):
        assert not set(declared(other)) & set(names), other


def test_scratch_bytes_depend_on_the_brick_counts_alone_and_match_the_headers_formula():
    L = _lib.load()
    for n in (0, 1, 255, 256, 257, 70000):
        assert L.kfx_mesh_bricks_scratch_bytes(n, 0) == formula(n), n
        assert L.kfx_mesh_bricks_scratch_bytes(n, 5) == formula(n, 5) == formula(n) + (108 * n + 255) // 256 * 256, n
    assert formula(70000) == 7847424 and formula(0) == 256
    sizes = [L.kfx_mesh_bricks_scratch_bytes(n, 0) for n in range(0, 3000, 7)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]   # monotone in n
    # a 40 x 24 x 16 frame and a 4096^3 frame with the same n: the function has no frame to look at, and a plan accepts exactly
    # these bytes for both (one byte less is too little for both)
    n = 30
    need = L.kfx_mesh_bricks_scratch_bytes(n, 0)
    totals = (C.c_ulonglong * 2)(7, 7)
    for dims in ((40, 24, 16), (4096, 4096, 4096)):
        assert L.kfx_mesh_bricks_plan(R(frame(*dims)), F32, FAKE, FAKE, n, FAKE, need - 1, totals, None) == E_SHAPE
        assert L.kfx_mesh_bricks_plan(R(frame(*dims)), F32, FAKE, FAKE, n, FAKE + 8, need, totals, None) == E_ALIGN   # (large enough: the next check)
    # refused counts
    assert L.kfx_mesh_bricks_scratch_bytes(1 << 31, 0) == 0 and L.kfx_mesh_bricks_scratch_bytes(1, 1 << 31) == 0
    assert L.kfx_mesh_bricks_scratch_bytes((1 << 31) - 1, (1 << 31) - 1) == formula((1 << 31) - 1, 1)


def test_every_refusal_gives_its_code_before_any_hip_call():
    L = _lib.load()
    totals = (C.c_ulonglong * 2)(123, 456)
    good = frame(40, 24, 16)
    n, nc = 30, 12
    need, need_c = L.kfx_mesh_bricks_scratch_bytes(n, 0), L.kfx_mesh_bricks_scratch_bytes(n, nc)
    assert need_c > need

    def plan(f=good, cell=F32, ids=FAKE, cells=FAKE, cnt=n, scratch=FAKE, nbytes=need, tot=totals):
        return L.kfx_mesh_bricks_plan(R(f) if f is not None else None, cell, ids, cells, cnt, scratch, nbytes, tot, None)

    def emit(f=good, cell=F32, ids=FAKE, cells=FAKE, cnt=n, cids=FAKE, ccells=FAKE, ccnt=nc, scratch=FAKE, nbytes=need_c, tot=totals,
             outs=(FAKE, FAKE, FAKE, FAKE, FAKE)):
        return L.kfx_mesh_bricks_emit(R(f) if f is not None else None, cell, ids, cells, cnt, cids, ccells, ccnt, scratch, nbytes, tot, *outs, None)

    # null pointers
    assert plan(f=None) == E_NULL and emit(f=None) == E_NULL
    assert plan(ids=None) == E_NULL and plan(cells=None) == E_NULL and plan(scratch=None) == E_NULL and plan(tot=None) == E_NULL
    assert emit(ids=None) == E_NULL and emit(cells=None) == E_NULL and emit(scratch=None) == E_NULL and emit(tot=None) == E_NULL
    assert emit(cids=None) == E_NULL and emit(ccells=None) == E_NULL
    for k in range(4):   # cube_index, tri_offset, verts, norms (colours may be null: no colours are written then)
        outs = [FAKE] * 5
        outs[k] = None
        assert emit(outs=tuple(outs)) == E_NULL, k
    # an unknown cell kind (the colour kind is no SDF kind)
    for bad in (COLOR, 3, -1):
        assert plan(cell=bad) == E_RANGE and emit(cell=bad) == E_RANGE
    # more than 2^31 - 1 bricks in the frame, or entries in a list
    assert plan(f=frame(65535, 65535, 65535)) == E_RANGE and emit(f=frame(65535, 65535, 65535)) == E_RANGE
    assert plan(cnt=1 << 31, nbytes=1 << 62) == E_RANGE and emit(cnt=1 << 31, nbytes=1 << 62) == E_RANGE and emit(ccnt=1 << 31, nbytes=1 << 62) == E_RANGE
    # frame dimensions the dense kfx_mesh_plan would refuse
    for dims in ((2, 24, 16), (40, 0, 16), (40, 24, 1), (65536, 24, 16), (40, 24, 65536)):
        assert plan(f=frame(*dims)) == E_SHAPE and emit(f=frame(*dims)) == E_SHAPE, dims
    assert plan(f=frame(3, 3, 3), cnt=1, nbytes=L.kfx_mesh_bricks_scratch_bytes(1, 0) - 1) == E_SHAPE   # (3 is accepted: the scratch is refused)
    # too little scratch: the plan needs the bytes without colour, the emit those with
    assert plan(nbytes=need - 1) == E_SHAPE and plan(nbytes=0) == E_SHAPE
    assert emit(nbytes=need_c - 1) == E_SHAPE and emit(nbytes=need) == E_SHAPE
    # misalignment: scratch 256, ids 4, cells 16, outputs 8 / 4
    for off in (1, 8, 16, 128):
        assert plan(scratch=FAKE + off, nbytes=need + 256) == E_ALIGN and emit(scratch=FAKE + off, nbytes=need_c + 256) == E_ALIGN
    assert plan(ids=FAKE + 2) == E_ALIGN and plan(cells=FAKE + 8) == E_ALIGN
    assert emit(ids=FAKE + 1) == E_ALIGN and emit(cells=FAKE + 4) == E_ALIGN and emit(cids=FAKE + 2) == E_ALIGN and emit(ccells=FAKE + 8) == E_ALIGN
    assert emit(outs=(FAKE + 4, FAKE, FAKE, FAKE, FAKE)) == E_ALIGN and emit(outs=(FAKE, FAKE, FAKE + 2, FAKE, FAKE)) == E_ALIGN
    assert emit(outs=(FAKE, FAKE, FAKE, FAKE, FAKE + 1)) == E_ALIGN
    # totals that no plan can have made are refused before the scratch is read back
    assert emit(tot=(C.c_ulonglong * 2)(5, 4)) == E_RANGE and emit(tot=(C.c_ulonglong * 2)(1, 2 ** 32 // 3)) == E_RANGE
    assert (totals[0], totals[1]) == (123, 456)   # no refusal wrote the totals

    # no bricks: (0, 0), nothing launched, the lists may be null; an emit of no bricks takes only the totals (0, 0)
    assert plan(ids=None, cells=None, cnt=0) == 0 and (totals[0], totals[1]) == (0, 0)
    totals[0], totals[1] = 9, 9
    assert plan(cnt=0, f=frame(4096, 4096, 4096), nbytes=256) == 0 and (totals[0], totals[1]) == (0, 0)
    assert emit(ids=None, cells=None, cnt=0, cids=None, ccells=None, ccnt=0, nbytes=256) == 0
    assert emit(ids=None, cells=None, cnt=0, cids=None, ccells=None, ccnt=0, nbytes=256, tot=(C.c_ulonglong * 2)(1, 1)) == E_RANGE
    # a mesh without cubes needs no outputs
    assert emit(tot=(C.c_ulonglong * 2)(0, 0), outs=(None,) * 5) == 0


def test_the_host_check_program_builds_and_passes(tmp_path):
    exe = str(tmp_path / "mesh_bricks_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(T.ROOT, "scripts", "mesh_bricks_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "mesh_bricks_host_check: ok" in out.stdout, out.stdout + out.stderr
