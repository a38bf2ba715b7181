"""The mesh clean-up (include/kfx_mesh_clean.h) is exported by libkfx.so, has its ctypes bindings, stays out of the other headers,
refuses bad arguments before any HIP call, and sizes its scratch from (V, T) alone by the header's formula, monotone in both.  No GPU:
the pointers below are never dereferenced, and every call is a refusal, a host-only function or an empty mesh, which launches nothing."""
import ctypes as C
import os
import re

import kfx_testlib as T
from kangaroo_amd import _lib

E_NULL, E_SHAPE, E_ALIGN, E_RANGE = -1, -2, -3, -4
FAKE = 1 << 20   # an aligned address that nothing may touch
U2 = C.c_ulonglong * 2
TMAX = (2 ** 32 - 1) // 3   # the most faces: 3T < 2^32

NAMES = ["kfx_mesh_components_emit", "kfx_mesh_components_plan", "kfx_mesh_components_scratch_bytes", "kfx_mesh_filter_emit", "kfx_mesh_filter_plan"]


def declared(header):
    src = open(os.path.join(T.ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kfx_[a-z0-9_]+)\s*\(", src)))


def formula(v, t):
    """include/kfx_mesh_clean.h: 256 + 3 r256(4 V) + 4 r256(4 ceil(V / 256)) + 2 r256(4 ceil(T / 256))"""
    r256 = lambda n: (n + 255) // 256 * 256
    return 256 + 3 * r256(4 * v) + 4 * r256(4 * ((v + 255) // 256)) + 2 * r256(4 * ((t + 255) // 256))


def test_mesh_clean_symbols_are_exported_and_bound_and_stay_in_their_header():
    L = _lib.load()
    names = declared("kfx_mesh_clean.h")
    assert names == NAMES, names
    for n in names:
        assert hasattr(L, n), "libkfx.so does not export %s" % n
        assert n in _lib.SIGNATURES, "python binding missing for %s" % n
    for other in ("kfx.h", "kfx_mesh.h", "kfx_mesh_index.h", "kfx_mesh_bricks.h", "kfx_mesh_bricks_index.h"):
        assert not set(declared(other)) & set(names), other


def test_scratch_bytes_match_the_headers_formula_and_are_monotone():
    L = _lib.load()
    size = L.kfx_mesh_components_scratch_bytes
    for t in (1, 85, 86, 255, 256, 257, 4948, 70000, 2200000, TMAX):
        for v in (1, 3, 255, 256, 257, 2480, 1170000, 3 * TMAX):
            if v <= 3 * t:
                assert size(v, t) == formula(v, t), (v, t)
    assert size(0, 0) == 256 and size(3, 1) == 10 * 256
    # about 12 bytes per vertex, next to nothing per face: the S_room orbit mesh
    assert 12.0 * 1170000 < size(1170000, 2200000) < 12.2 * 1170000
    assert size(3, 2200000) - size(3, 1) < 2200000 * 8 // 256 + 1024
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
    need = L.kfx_mesh_components_scratch_bytes(V, Tn)
    counts, kept = U2(77, 77), U2(600, 1000)

    def plan(faces=FAKE, t=Tn, v=V, scratch=FAKE, nbytes=need, out=counts):
        return L.kfx_mesh_components_plan(faces, t, v, scratch, nbytes, out, None)

    def emit(scratch=FAKE, nbytes=need, v=V, t=Tn, cnt=U2(3, 900), vc=FAKE, cf=FAKE + (1 << 16)):
        return L.kfx_mesh_components_emit(scratch, nbytes, v, t, cnt, vc, cf, None)

    def fplan(scratch=FAKE, nbytes=need, v=V, t=Tn, faces=FAKE, min_faces=10, largest=0, out=counts):
        return L.kfx_mesh_filter_plan(scratch, nbytes, v, t, faces, min_faces, largest, out, None)

    IN = [FAKE + (1 << 24) + k * (1 << 16) for k in range(4)]
    OUT = [FAKE + (1 << 25) + k * (1 << 16) for k in range(4)]

    def femit(scratch=FAKE, nbytes=need, v=V, t=Tn, k=kept, ins=IN, outs=OUT):
        return L.kfx_mesh_filter_emit(scratch, nbytes, v, t, k, *ins, *outs, None)

    # null pointers
    assert plan(faces=None) == E_NULL and plan(scratch=None) == E_NULL and plan(out=None) == E_NULL
    assert emit(scratch=None) == E_NULL and emit(cnt=None) == E_NULL and emit(vc=None) == E_NULL and emit(cf=None) == E_NULL
    assert fplan(scratch=None) == E_NULL and fplan(faces=None) == E_NULL and fplan(out=None) == E_NULL
    assert femit(scratch=None) == E_NULL and femit(k=None) == E_NULL
    for i in (0, 3):   # verts and faces (normals and colours are optional, on either side)
        a, b = list(IN), list(OUT)
        a[i] = None
        b[i] = None
        assert femit(ins=a) == E_NULL and femit(outs=b) == E_NULL, i
    # counts: V = 0 with T > 0, vertices without faces, V > 3T, 3T >= 2^32
    for v, t in ((0, Tn), (1, 0), (3 * Tn + 1, Tn), (V, TMAX + 1), (V, 2 ** 62)):
        big = 1 << 62
        assert plan(v=v, t=t, nbytes=big) == E_RANGE and emit(v=v, t=t, nbytes=big) == E_RANGE, (v, t)
        assert fplan(v=v, t=t, nbytes=big) == E_RANGE and femit(v=v, t=t, nbytes=big) == E_RANGE, (v, t)
    # too little scratch
    for call in (plan, emit, fplan, femit):
        assert call(nbytes=need - 1) == E_SHAPE and call(nbytes=0) == E_SHAPE, call.__name__
    # misalignment: the scratch 256, every array 4
    for off in (1, 8, 16, 128):
        for call in (plan, emit, fplan, femit):
            assert call(scratch=FAKE + off, nbytes=need + 256) == E_ALIGN, (call.__name__, off)
    assert plan(faces=FAKE + 2) == E_ALIGN and fplan(faces=FAKE + 1) == E_ALIGN
    assert emit(vc=FAKE + 2) == E_ALIGN and emit(cf=FAKE + (1 << 16) + 1) == E_ALIGN
    for i in range(4):
        a, b = list(IN), list(OUT)
        a[i] += 2
        b[i] += 1
        assert femit(ins=a) == E_ALIGN and femit(outs=b) == E_ALIGN, i
    # counts no plan can have made are refused before a scratch is read back
    assert emit(cnt=U2(V + 1, 5)) == E_RANGE and emit(cnt=U2(3, Tn + 1)) == E_RANGE and emit(cnt=U2(0, 0)) == E_RANGE
    assert femit(k=U2(V + 1, 5)) == E_RANGE and femit(k=U2(5, Tn + 1)) == E_RANGE
    # outputs that overlap inputs, each other or the scratch
    for i in range(4):
        b = list(OUT)
        b[i] = IN[i]
        assert femit(outs=b) == E_RANGE, i
    b = list(OUT)
    b[0] = IN[3] + 12 * Tn - 4   # the last word of the input faces
    assert femit(outs=b) == E_RANGE
    b[0] = OUT[1] - 12 * 600 + 4   # the first word of the next output
    assert femit(outs=b) == E_RANGE
    b[0] = FAKE + need - 4   # the last word of the scratch
    assert femit(outs=b) == E_RANGE
    assert emit(vc=FAKE + 256) == E_RANGE and emit(cf=FAKE + (1 << 16), vc=FAKE + (1 << 16) - 4 * V + 4) == E_RANGE
    assert (counts[0], counts[1]) == (77, 77) and (kept[0], kept[1]) == (600, 1000)   # no refusal wrote anything


def test_an_empty_mesh_returns_zeros_and_launches_nothing():
    L = _lib.load()
    assert L.kfx_mesh_components_scratch_bytes(0, 0) == 256
    out = U2(77, 77)
    assert L.kfx_mesh_components_plan(None, 0, 0, FAKE, 256, out, None) == 0 and (out[0], out[1]) == (0, 0)
    out = U2(77, 77)
    assert L.kfx_mesh_filter_plan(FAKE, 256, 0, 0, None, 5, 1, out, None) == 0 and (out[0], out[1]) == (0, 0)
    assert L.kfx_mesh_components_emit(FAKE, 256, 0, 0, U2(0, 0), None, None, None) == 0
    assert L.kfx_mesh_filter_emit(FAKE, 256, 0, 0, U2(0, 0), *([None] * 8), None) == 0
    # ... but not without a scratch, however small the mesh
    assert L.kfx_mesh_components_plan(None, 0, 0, None, 256, out, None) == E_NULL
    assert L.kfx_mesh_components_plan(None, 0, 0, FAKE, 255, out, None) == E_SHAPE
    assert L.kfx_mesh_components_plan(None, 0, 0, FAKE + 4, 256, out, None) == E_ALIGN
