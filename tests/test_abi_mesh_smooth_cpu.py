"""The mesh smoothing (include/kfx_mesh_smooth.h) is exported by libkfx.so, has its ctypes bindings, stays out of the other headers,
refuses bad arguments before any HIP call, and sizes its scratches from (V, T) alone by the header's formulas, monotone in both.
No GPU: the pointers below are never dereferenced, and every call is a refusal, a host-only function or an empty mesh, which launches
nothing."""
import ctypes as C
import os
import re

import kfx_testlib as T
from kangaroo_amd import _lib

E_NULL, E_SHAPE, E_ALIGN, E_RANGE = -1, -2, -3, -4
FAKE = 1 << 30   # an aligned address that nothing may touch
TMAX = (2 ** 32 - 1) // 3   # the most faces: 3T < 2^32

NAMES = ["kfx_mesh_adjacency", "kfx_mesh_adjacency_scratch_bytes", "kfx_mesh_smooth", "kfx_mesh_smooth_scratch_bytes", "kfx_mesh_vertex_normals",
         "kfx_mesh_vertex_normals_scratch_bytes"]


def declared(header):
    src = open(os.path.join(T.ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kfx_[a-z0-9_]+)\s*\(", src)))


r256 = lambda n: (n + 255) // 256 * 256


def adjacency_formula(v, t):
    """include/kfx_mesh_smooth.h: 256 + r256(4 V) + r256(12 T) + r256(4 (3T / 64 + 1)) + 2 r256(4 ceil(V / 256))"""
    return 256 + r256(4 * v) + r256(12 * t) + r256(4 * (3 * t // 64 + 1)) + 2 * r256(4 * ((v + 255) // 256))


def smooth_formula(v, t):
    """include/kfx_mesh_smooth.h: 256 + r256(12 V) + r256(24 T)"""
    return 256 + r256(12 * v) + r256(24 * t)


def test_mesh_smooth_symbols_are_exported_and_bound_and_stay_in_their_header():
    L = _lib.load()
    names = declared("kfx_mesh_smooth.h")
    assert names == NAMES, names
    for n in names:
        assert hasattr(L, n), "libkfx.so does not export %s" % n
        assert n in _lib.SIGNATURES, "python binding missing for %s" % n
    for other in ("kfx.h", "kfx_mesh.h", "kfx_mesh_index.h", "kfx_mesh_bricks.h", "kfx_mesh_bricks_index.h", "kfx_mesh_clean.h", "kfx_mesh_simplify.h"):
        assert not set(declared(other)) & set(names), other


def test_scratch_bytes_match_the_headers_formulas_and_are_monotone():
    L = _lib.load()
    adj, smooth, normals = L.kfx_mesh_adjacency_scratch_bytes, L.kfx_mesh_smooth_scratch_bytes, L.kfx_mesh_vertex_normals_scratch_bytes
    for t in (1, 16, 21, 22, 85, 86, 171, 255, 256, 257, 4948, 65536, 70000, 2200000, TMAX):
        for v in (1, 3, 32, 33, 255, 256, 257, 2480, 65536, 1170000, 3 * TMAX):
            if v <= 3 * t:
                assert adj(v, t) == adjacency_formula(v, t), (v, t)
                assert smooth(v, t) == smooth_formula(v, t), (v, t)
                assert normals(v, t) == 256
    assert adj(0, 0) == 512 and smooth(0, 0) == 256 and normals(0, 0) == 256
    # the neighbour table has 8 bytes per incidence, the second buffer 12 per vertex; the slots of the fill 4 per corner
    for v, t in ((1170000, 2200000), (2480, 4948), (64, 64)):
        assert 256 + 12 * v + 24 * t <= smooth(v, t) < 256 + 12 * v + 24 * t + 512
        assert adj(v, t) >= 256 + 4 * v + 12 * t
    for size in (adj, smooth):
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
    for size in (adj, smooth, normals):
        assert size(0, 5) == 0 and size(1, 0) == 0 and size(4, 1) == 0 and size(1, TMAX + 1) == 0 and size(3, 2 ** 63) == 0 and size(2 ** 63, 5) == 0


def test_every_refusal_gives_its_code_before_any_hip_call():
    L = _lib.load()
    V, Tn = 700, 1200
    VERTS, FACES, START, INC, FLAGS, OUT, OUT2, OUT3 = [FAKE + (1 << 24) + k * (1 << 16) for k in range(8)]
    SCRATCH = FAKE + (1 << 26)
    need = {"adj": L.kfx_mesh_adjacency_scratch_bytes(V, Tn), "smooth": L.kfx_mesh_smooth_scratch_bytes(V, Tn), "normals": 256}

    def adj(faces=FACES, t=Tn, v=V, start=OUT, inc=OUT2, flags=OUT3, scratch=SCRATCH, nbytes=need["adj"]):
        return L.kfx_mesh_adjacency(faces, t, v, start, inc, flags, scratch, nbytes, None)

    def smooth(verts=VERTS, faces=FACES, t=Tn, v=V, start=START, inc=INC, flags=FLAGS, iterations=5, lam=0.5, mu=-0.53, pin=1, out=OUT,
               scratch=SCRATCH, nbytes=need["smooth"]):
        return L.kfx_mesh_smooth(verts, faces, t, v, start, inc, flags, iterations, lam, mu, pin, out, scratch, nbytes, None)

    def normals(verts=VERTS, faces=FACES, t=Tn, v=V, start=START, inc=INC, out=OUT, scratch=SCRATCH, nbytes=256):
        return L.kfx_mesh_vertex_normals(verts, faces, t, v, start, inc, out, scratch, nbytes, None)

    # null pointers; the flags are optional for the adjacency, and for the smoothing when nothing is pinned
    assert adj(faces=None) == E_NULL and adj(start=None) == E_NULL and adj(inc=None) == E_NULL and adj(scratch=None) == E_NULL
    for name in ("verts", "faces", "start", "inc", "out", "scratch"):
        assert smooth(**{name: None}) == E_NULL and normals(**{name: None}) == E_NULL, name
    assert smooth(flags=None) == E_NULL
    # counts: V = 0 with T > 0, vertices without faces, V > 3T, 3T >= 2^32
    for v, t in ((0, Tn), (1, 0), (3 * Tn + 1, Tn), (V, TMAX + 1), (V, 2 ** 62)):
        big = 1 << 62
        assert adj(v=v, t=t, nbytes=big) == E_RANGE and smooth(v=v, t=t, nbytes=big) == E_RANGE and normals(v=v, t=t, nbytes=big) == E_RANGE, (v, t)
    # the parameters: iterations < 0, lambda outside (0, 1] or not finite, mu > 0 or not finite
    assert smooth(iterations=-1) == E_RANGE
    for lam in (0.0, -0.5, 1.0000001, float("nan"), float("inf"), -float("inf")):
        assert smooth(lam=lam) == E_RANGE, lam
    for mu in (1e-6, 0.53, float("nan"), float("inf"), -float("inf")):
        assert smooth(mu=mu) == E_RANGE, mu
    # too little scratch
    for call, key in ((adj, "adj"), (smooth, "smooth"), (normals, "normals")):
        assert call(nbytes=need[key] - 1) == E_SHAPE and call(nbytes=0) == E_SHAPE, key
    # misalignment: the scratch 256, every array 4
    for off in (1, 8, 16, 128):
        for call, key in ((adj, "adj"), (smooth, "smooth"), (normals, "normals")):
            assert call(scratch=SCRATCH + off, nbytes=need[key] + 256) == E_ALIGN, (key, off)
    assert adj(faces=FACES + 2) == E_ALIGN and adj(start=OUT + 1) == E_ALIGN and adj(inc=OUT2 + 2) == E_ALIGN and adj(flags=OUT3 + 3) == E_ALIGN
    for name, at in (("verts", VERTS), ("faces", FACES), ("start", START), ("inc", INC), ("out", OUT)):
        assert smooth(**{name: at + 2}) == E_ALIGN and normals(**{name: at + 1}) == E_ALIGN, name
    assert smooth(flags=FLAGS + 2) == E_ALIGN
    # an output that overlaps an input, another output or the scratch; a scratch that overlaps an input
    assert adj(start=FACES + 12 * Tn - 4) == E_RANGE and adj(inc=FACES) == E_RANGE and adj(flags=FACES + 4) == E_RANGE
    assert adj(inc=OUT + 4 * V) == E_RANGE and adj(flags=OUT2 + 12 * Tn - 4) == E_RANGE   # (inc_start has V + 1 words)
    assert adj(start=SCRATCH + need["adj"] - 4) == E_RANGE and adj(scratch=FACES - need["adj"] + 256) == E_RANGE
    for at, n in ((VERTS, 12 * V), (FACES, 12 * Tn), (START, 4 * (V + 1)), (INC, 12 * Tn)):
        assert smooth(out=at + n - 4) == E_RANGE and smooth(out=at - 12 * V + 4) == E_RANGE and normals(out=at + n - 4) == E_RANGE, at
    assert smooth(out=FLAGS + 4 * V - 4) == E_RANGE and smooth(out=VERTS) == E_RANGE
    assert smooth(out=SCRATCH + need["smooth"] - 4) == E_RANGE and normals(out=SCRATCH + 252) == E_RANGE
    assert smooth(scratch=VERTS + 256 * 32 - need["smooth"], nbytes=need["smooth"]) == E_RANGE
    # what is accepted up to here fails only at the first HIP call, which these addresses never reach: no such call is made in this test


def test_an_empty_mesh_launches_nothing():
    L = _lib.load()
    assert L.kfx_mesh_adjacency(None, 0, 0, None, None, None, FAKE, 512, None) == 0
    assert L.kfx_mesh_smooth(None, None, 0, 0, None, None, None, 5, 0.5, -0.53, 1, None, FAKE, 256, None) == 0
    assert L.kfx_mesh_vertex_normals(None, None, 0, 0, None, None, None, FAKE, 256, None) == 0
    # ... but not without a scratch or with parameters out of range, however small the mesh
    assert L.kfx_mesh_adjacency(None, 0, 0, None, None, None, None, 512, None) == E_NULL
    assert L.kfx_mesh_adjacency(None, 0, 0, None, None, None, FAKE, 511, None) == E_SHAPE
    assert L.kfx_mesh_adjacency(None, 0, 0, None, None, None, FAKE + 4, 512, None) == E_ALIGN
    assert L.kfx_mesh_smooth(None, None, 0, 0, None, None, None, 5, 1.5, -0.53, 1, None, FAKE, 256, None) == E_RANGE
