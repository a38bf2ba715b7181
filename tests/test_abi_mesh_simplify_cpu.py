"""The mesh simplification (include/kfx_mesh_simplify.h) is exported by libkfx.so, has its ctypes bindings, stays out of the other
headers, refuses bad arguments before any HIP call, and sizes its scratch from (V, T) alone by the header's formula, monotone in both.
No GPU: the pointers below are never dereferenced, and every call is a refusal, a host-only function or an empty mesh, which launches
nothing."""
import ctypes as C
import os
import re

import kfx_testlib as T
from kangaroo_amd import _lib

E_NULL, E_SHAPE, E_ALIGN, E_RANGE = -1, -2, -3, -4
FAKE = 1 << 30   # an aligned address that nothing may touch
U2 = C.c_ulonglong * 2
F3 = C.c_float * 3
TMAX = (2 ** 32 - 1) // 3   # the most faces: 3T < 2^32

NAMES = ["kfx_mesh_simplify_emit", "kfx_mesh_simplify_plan", "kfx_mesh_simplify_scratch_bytes"]


def declared(header):
    src = open(os.path.join(T.ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kfx_[a-z0-9_]+)\s*\(", src)))


def formula(v, t):
    """include/kfx_mesh_simplify.h: 256 + 8 p2(2 V) + 4 p2(2 T) + 3 r256(4 V) + r256(4 T) + 2 r256(4 ceil(V / 256)) + 2 r256(4 ceil(T / 256))"""
    r256 = lambda n: (n + 255) // 256 * 256
    p2 = lambda n: max(64, 1 << (n - 1).bit_length()) if n > 0 else 64
    return (256 + 8 * p2(2 * v) + 4 * p2(2 * t) + 3 * r256(4 * v) + r256(4 * t) + 2 * r256(4 * ((v + 255) // 256))
            + 2 * r256(4 * ((t + 255) // 256)))


def test_mesh_simplify_symbols_are_exported_and_bound_and_stay_in_their_header():
    L = _lib.load()
    names = declared("kfx_mesh_simplify.h")
    assert names == NAMES, names
    for n in names:
        assert hasattr(L, n), "libkfx.so does not export %s" % n
        assert n in _lib.SIGNATURES, "python binding missing for %s" % n
    for other in ("kfx.h", "kfx_mesh.h", "kfx_mesh_index.h", "kfx_mesh_bricks.h", "kfx_mesh_bricks_index.h", "kfx_mesh_clean.h"):
        assert not set(declared(other)) & set(names), other


def test_scratch_bytes_match_the_headers_formula_and_are_monotone():
    L = _lib.load()
    size = L.kfx_mesh_simplify_scratch_bytes
    for t in (1, 16, 32, 33, 85, 86, 255, 256, 257, 4948, 65536, 70000, 2200000, TMAX):
        for v in (1, 3, 32, 33, 255, 256, 257, 2480, 65536, 1170000, 3 * TMAX):
            if v <= 3 * t:
                assert size(v, t) == formula(v, t), (v, t)
    assert size(0, 0) == 256 + 512 + 256
    # both tables are at most half full: at least 2 V slots of 8 bytes and 2 T slots of 4
    for v, t in ((1170000, 2200000), (2480, 4948), (64, 64)):
        assert size(v, t) >= 256 + 16 * v + 8 * t + 12 * v + 4 * t
        assert size(v, t) <= 256 + 32 * v + 16 * t + 12 * v + 4 * t + 16 * 256
    # monotone in V and in T
    last = 0
    for v in range(1, 3000):
        now = size(v, 1000)
        assert now >= last > 0 or v == 1
        last = now
    last = 0
    for t in range(1, 3000):
        now = size(3, t)
        assert now >= last > 0 or t == 1
        last = now
    # refused: vertices without faces, more vertices than corners, 3T >= 2^32
    assert size(0, 5) == 0 and size(1, 0) == 0 and size(4, 1) == 0 and size(1, TMAX + 1) == 0 and size(3, 2 ** 63) == 0 and size(2 ** 63, 5) == 0


def test_every_refusal_gives_its_code_before_any_hip_call():
    L = _lib.load()
    V, Tn = 700, 1200
    need = L.kfx_mesh_simplify_scratch_bytes(V, Tn)
    kept = U2(600, 1000)
    out = U2(77, 77)
    IN = [FAKE + (1 << 24) + k * (1 << 16) for k in range(4)]
    OUT = [FAKE + (1 << 25) + k * (1 << 16) for k in range(4)]
    MAP = FAKE + (1 << 26)

    def plan(verts=IN[0], faces=IN[3], t=Tn, v=V, origin=F3(0, 0, 0), cell=0.01, scratch=FAKE, nbytes=need, o=out):
        return L.kfx_mesh_simplify_plan(verts, faces, t, v, origin, cell, scratch, nbytes, o, None)

    def emit(scratch=FAKE, nbytes=need, v=V, t=Tn, k=kept, ins=IN, outs=OUT, vmap=MAP):
        return L.kfx_mesh_simplify_emit(scratch, nbytes, v, t, k, *ins, *outs, vmap, None)

    # null pointers
    assert plan(verts=None) == E_NULL and plan(faces=None) == E_NULL and plan(scratch=None) == E_NULL and plan(o=None) == E_NULL
    assert plan(origin=None) == E_NULL
    assert emit(scratch=None) == E_NULL and emit(k=None) == E_NULL
    for i in (0, 3):   # verts and faces (normals and colours are optional, on either side)
        a, b = list(IN), list(OUT)
        a[i] = None
        b[i] = None
        assert emit(ins=a) == E_NULL and emit(outs=b) == E_NULL, i
    # counts: V = 0 with T > 0, vertices without faces, V > 3T, 3T >= 2^32
    for v, t in ((0, Tn), (1, 0), (3 * Tn + 1, Tn), (V, TMAX + 1), (V, 2 ** 62)):
        big = 1 << 62
        assert plan(v=v, t=t, nbytes=big) == E_RANGE and emit(v=v, t=t, nbytes=big) == E_RANGE, (v, t)
    # the grid: a cell that is not a finite length > 0 (or whose reciprocal is not finite), an origin that is not finite
    for cell in (0.0, -0.01, float("nan"), float("inf"), -float("inf"), 1e-45):
        assert plan(cell=cell) == E_RANGE, cell
    for k in range(3):
        for bad in (float("nan"), float("inf"), -float("inf")):
            o = [0.0, 0.0, 0.0]
            o[k] = bad
            assert plan(origin=F3(*o)) == E_RANGE, (k, bad)
    # too little scratch
    for call in (plan, emit):
        assert call(nbytes=need - 1) == E_SHAPE and call(nbytes=0) == E_SHAPE, call.__name__
    # misalignment: the scratch 256, every array 4
    for off in (1, 8, 16, 128):
        for call in (plan, emit):
            assert call(scratch=FAKE + off, nbytes=need + 256) == E_ALIGN, (call.__name__, off)
    assert plan(faces=IN[3] + 2) == E_ALIGN and plan(verts=IN[0] + 1) == E_ALIGN
    for i in range(4):
        a, b = list(IN), list(OUT)
        a[i] += 2
        b[i] += 1
        assert emit(ins=a) == E_ALIGN and emit(outs=b) == E_ALIGN, i
    assert emit(vmap=MAP + 2) == E_ALIGN
    # counts no plan can have made are refused before a scratch is read back
    assert emit(k=U2(V + 1, 5)) == E_RANGE and emit(k=U2(5, Tn + 1)) == E_RANGE
    # outputs that overlap inputs, each other or the scratch; a scratch that overlaps the plan's inputs
    for i in range(4):
        b = list(OUT)
        b[i] = IN[i]
        assert emit(outs=b) == E_RANGE, i
    b = list(OUT)
    b[0] = IN[3] + 12 * Tn - 4   # the last word of the input faces
    assert emit(outs=b) == E_RANGE
    b[0] = OUT[1] - 12 * 600 + 4   # the first word of the next output
    assert emit(outs=b) == E_RANGE
    b[0] = FAKE + need - 4   # the last word of the scratch
    assert emit(outs=b) == E_RANGE
    assert emit(vmap=IN[0] + 12 * V - 4) == E_RANGE and emit(vmap=OUT[3] - 4 * V + 4) == E_RANGE and emit(vmap=FAKE + 256) == E_RANGE
    assert plan(verts=FAKE + need - 4) == E_RANGE and plan(faces=FAKE + 512) == E_RANGE
    assert (out[0], out[1]) == (77, 77) and (kept[0], kept[1]) == (600, 1000)   # no refusal wrote anything


def test_an_empty_mesh_returns_zeros_and_launches_nothing():
    L = _lib.load()
    need = L.kfx_mesh_simplify_scratch_bytes(0, 0)
    assert need == 1024
    out = U2(77, 77)
    assert L.kfx_mesh_simplify_plan(None, None, 0, 0, F3(0, 0, 0), 0.01, FAKE, need, out, None) == 0 and (out[0], out[1]) == (0, 0)
    assert L.kfx_mesh_simplify_emit(FAKE, need, 0, 0, U2(0, 0), *([None] * 9), None) == 0
    # ... but not without a scratch or a grid, however small the mesh
    assert L.kfx_mesh_simplify_plan(None, None, 0, 0, F3(0, 0, 0), 0.01, None, need, out, None) == E_NULL
    assert L.kfx_mesh_simplify_plan(None, None, 0, 0, F3(0, 0, 0), 0.01, FAKE, need - 1, out, None) == E_SHAPE
    assert L.kfx_mesh_simplify_plan(None, None, 0, 0, F3(0, 0, 0), 0.01, FAKE + 4, need, out, None) == E_ALIGN
    assert L.kfx_mesh_simplify_plan(None, None, 0, 0, F3(0, 0, 0), 0.0, FAKE, need, out, None) == E_RANGE
