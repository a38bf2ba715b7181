"""The brick ray-cast (include/kfx_raycast_bricks.h) is exported by libkfx.so, has its ctypes bindings, stays out of the other headers,
refuses bad arguments before any HIP call, and sizes its scratch from the brick counts alone, by the header's formula.  No GPU: the
pointers below are never dereferenced and every call is a refusal, a host-only function or an empty image, which launches nothing.  The
host-check program (scripts/raycast_bricks_host_check.cpp) builds with a plain host compiler, and under the host sanitizers, and passes."""
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

NAMES = ["kfx_raycast_bricks", "kfx_raycast_bricks_plan", "kfx_raycast_bricks_scratch_bytes"]


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


def image(w, h, elem, ptr=FAKE, pitch=None):
    return _lib.KfxImage(w * elem if pitch is None else pitch, ptr, w, h)


def cap(m):
    c = 1
    while c < 2 * m:
        c *= 2
    return c if m else 0


def formula(n, n_color=0):
    """include/kfx_raycast_bricks.h: 256 + round256(8 cap(n)) + round256(8 cap(n_color)), cap(0) = 0, cap(m) = the power of two >= 2 m"""
    r256 = lambda v: (v + 255) // 256 * 256
    return 256 + r256(8 * cap(n)) + r256(8 * cap(n_color))


def test_brick_raycast_symbols_are_exported_and_bound_and_stay_in_their_header():
    L = _lib.load()
    names = declared("kfx_raycast_bricks.h")
    assert names == NAMES, names
    for n in names:
        assert hasattr(L, n), "libkfx.so does not export %s" % n
        assert n in _lib.SIGNATURES, "python binding missing for %s" % n
    for other in ("kfx.h", "kfx_mesh.h", "kfx_shift.h", "kfx_bricks.h", "kfx_mesh_bricks.h", "kfx_color.h", "kfx_extras.h"):
        assert not set(declared(other)) & set(names), other


def test_the_headers_text_states_the_formula_the_library_computes():
    text = open(os.path.join(T.ROOT, "include", "kfx_raycast_bricks.h")).read()
    assert "256 + round256(8 cap(n)) + round256(8 cap(n_color))" in text
    assert "cap(0) = 0, cap(m) = the smallest power of two >= 2 m" in text


def test_scratch_bytes_depend_on_the_brick_counts_alone_and_match_the_headers_formula():
    L = _lib.load()
    for n in (0, 1, 2, 3, 16, 17, 255, 256, 257, 832, 70000):
        assert L.kfx_raycast_bricks_scratch_bytes(n, 0) == formula(n), n
        assert L.kfx_raycast_bricks_scratch_bytes(n, 5) == formula(n, 5) == formula(n) + 256, n
        assert L.kfx_raycast_bricks_scratch_bytes(n, 300) == formula(n) + 8 * 1024, n
    assert formula(0) == 256 and formula(1) == 512 and formula(832) == 256 + 8 * 2048 and formula(70000) == 256 + 8 * 262144
    assert all(cap(m) >= 2 * m and cap(m) < 4 * m and cap(m) & (cap(m) - 1) == 0 for m in range(1, 3000))   # the capacity rule
    sizes = [L.kfx_raycast_bricks_scratch_bytes(n, 0) for n in range(0, 3000, 7)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]   # monotone in n
    # a 40 x 24 x 16 frame and a 4096^3 frame with the same n: the function has no frame to look at, and a plan accepts exactly these
    # bytes for both (one byte less is too little for both)
    n = 30
    need = L.kfx_raycast_bricks_scratch_bytes(n, 0)
    for dims in ((40, 24, 16), (4096, 4096, 4096)):
        assert L.kfx_raycast_bricks_plan(R(frame(*dims)), FAKE, n, None, 0, FAKE, need - 1, None) == E_SHAPE
        assert L.kfx_raycast_bricks_plan(R(frame(*dims)), FAKE, n, None, 0, FAKE + 8, need, None) == E_ALIGN   # (large enough: the next check)
    # refused counts
    assert L.kfx_raycast_bricks_scratch_bytes(1 << 31, 0) == 0 and L.kfx_raycast_bricks_scratch_bytes(1, 1 << 31) == 0
    assert L.kfx_raycast_bricks_scratch_bytes((1 << 31) - 1, (1 << 31) - 1) == formula((1 << 31) - 1, (1 << 31) - 1) == 256 + 2 * 8 * (1 << 32)


def test_every_refusal_gives_its_code_before_any_hip_call():
    L = _lib.load()
    good = frame(40, 24, 16)
    n, nc = 30, 12
    need, need_c = L.kfx_raycast_bricks_scratch_bytes(n, 0), L.kfx_raycast_bricks_scratch_bytes(n, nc)
    assert need_c > need
    pose = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -3)
    K = (C.c_float * 4)(100, 100, 47.5, 35.5)
    W, H = 96, 72

    def plan(f=good, ids=FAKE, cnt=n, cids=FAKE, ccnt=nc, scratch=FAKE, nbytes=need_c):
        return L.kfx_raycast_bricks_plan(R(f) if f is not None else None, ids, cnt, cids, ccnt, scratch, nbytes, None)

    def render(d="ok", nr="ok", im="ok", f=good, cell=F32, ids=FAKE, cells=FAKE, cnt=n, cids=FAKE, ccells=FAKE, ccnt=nc, color=1, scratch=FAKE,
               nbytes=need_c, t=pose, k=K):
        d = image(W, H, 4) if d == "ok" else d
        nr = image(W, H, 16) if nr == "ok" else nr
        im = image(W, H, 4) if im == "ok" else im
        ref = lambda x: R(x) if x is not None else None
        return L.kfx_raycast_bricks(ref(d), ref(nr), ref(im), ref(f), cell, ids, cells, cnt, cids, ccells, ccnt, color, scratch, nbytes, t, k,
                                    0.1, 10.0, 0.25, 1, None)

    # null pointers
    assert plan(f=None) == E_NULL and plan(ids=None) == E_NULL and plan(cids=None) == E_NULL and plan(scratch=None) == E_NULL
    assert render(t=None) == E_NULL and render(k=None) == E_NULL
    assert render(d=None) == E_NULL and render(nr=None) == E_NULL and render(im=None) == E_NULL
    assert render(d=image(W, H, 4, ptr=None)) == E_NULL and render(nr=image(W, H, 16, ptr=None)) == E_NULL
    assert render(f=None) == E_NULL and render(ids=None) == E_NULL and render(cells=None) == E_NULL and render(scratch=None) == E_NULL
    assert render(cids=None) == E_NULL and render(ccells=None) == E_NULL
    # an unknown cell kind (the colour kind is no SDF kind); colour with half cells
    for bad in (COLOR, 3, -1):
        assert render(cell=bad) == E_RANGE
    assert render(cell=F16, color=1) == E_RANGE
    # more than 2^31 - 1 bricks in the frame, or entries in a list
    assert plan(f=frame(65535, 65535, 65535)) == E_RANGE and render(f=frame(65535, 65535, 65535)) == E_RANGE
    assert plan(cnt=1 << 31, nbytes=1 << 62) == E_RANGE and plan(ccnt=1 << 31, nbytes=1 << 62) == E_RANGE
    assert render(cnt=1 << 31, nbytes=1 << 62) == E_RANGE and render(ccnt=1 << 31, nbytes=1 << 62) == E_RANGE
    # frame dimensions kfx_raycast_sdf would refuse
    for dims in ((2, 24, 16), (40, 0, 16), (40, 24, 1), (65536, 24, 16), (40, 24, 65536)):
        assert plan(f=frame(*dims)) == E_SHAPE and render(f=frame(*dims)) == E_SHAPE, dims
    assert plan(f=frame(3, 3, 3), cnt=1, ccnt=0, nbytes=L.kfx_raycast_bricks_scratch_bytes(1, 0) - 1) == E_SHAPE   # (3 is accepted: the scratch is refused)
    # too little scratch: by the counts of the call
    assert plan(nbytes=need_c - 1) == E_SHAPE and plan(nbytes=0) == E_SHAPE and plan(ccnt=0, cids=None, nbytes=need - 1) == E_SHAPE
    assert render(nbytes=need_c - 1) == E_SHAPE and render(nbytes=need) == E_SHAPE and render(ccnt=0, cids=None, ccells=None, nbytes=need - 1) == E_SHAPE
    # images check_render_images refuses: smaller than img, a pitch below a row, misaligned
    assert render(d=image(W - 1, H, 4)) == E_SHAPE and render(nr=image(W, H - 1, 16)) == E_SHAPE
    assert render(im=image(W, H, 4, pitch=4 * W - 4)) == E_SHAPE and render(nr=image(W, H, 16, pitch=8 * W)) == E_SHAPE
    assert render(d=image(W, H, 4, ptr=FAKE + 2)) == E_ALIGN and render(nr=image(W, H, 16, ptr=FAKE + 8)) == E_ALIGN
    assert render(im=image(W, H, 4, pitch=4 * W + 2)) == E_ALIGN
    # misalignment: scratch 256, ids 4, cells 16
    for off in (1, 8, 16, 128):
        assert plan(scratch=FAKE + off, nbytes=need_c + 256) == E_ALIGN and render(scratch=FAKE + off, nbytes=need_c + 256) == E_ALIGN
    assert plan(ids=FAKE + 2) == E_ALIGN and plan(cids=FAKE + 1) == E_ALIGN
    assert render(ids=FAKE + 1) == E_ALIGN and render(cells=FAKE + 4) == E_ALIGN and render(cids=FAKE + 2) == E_ALIGN and render(ccells=FAKE + 8) == E_ALIGN
    # the order: pose before images before the frame before the counts before the lists before the scratch
    assert render(t=None, d=None, f=None) == E_NULL and render(d=image(W - 1, H, 4), cell=7) == E_SHAPE
    assert render(cell=7, f=frame(2, 2, 2)) == E_RANGE and render(f=frame(2, 2, 2), cnt=1 << 31) == E_SHAPE
    assert render(cnt=1 << 31, ids=None) == E_RANGE and render(ids=FAKE + 1, scratch=None) == E_ALIGN
    assert plan(f=frame(2, 2, 2), cnt=1 << 31) == E_SHAPE and plan(cnt=1 << 31, ids=None) == E_RANGE and plan(ids=FAKE + 2, scratch=None) == E_ALIGN
    # an empty image launches nothing, whatever the lists hold; without entries the lists may be null
    assert render(d=image(0, H, 4), nr=image(0, H, 16), im=image(0, H, 4)) == 0
    assert render(d=image(W, 0, 4), nr=image(W, 0, 16), im=image(W, 0, 4), ids=None, cells=None, cnt=0, cids=None, ccells=None, ccnt=0, nbytes=256) == 0
    assert render(d=image(W, 0, 4), nr=image(W, 0, 16), im=image(W, 0, 4), cell=F16, color=0, f=frame(4096, 4096, 4096)) == 0


def test_the_host_check_program_builds_plainly_and_under_the_host_sanitizers_and_passes(tmp_path):
    src = os.path.join(T.ROOT, "scripts", "raycast_bricks_host_check.cpp")
    # (the sanitizers' runtimes linked into the program: it runs as it is, whatever else the process environment loads)
    sanitize = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    for name, flags in (("plain", []), ("sanitized", sanitize)):
        exe = str(tmp_path / ("raycast_bricks_host_check_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + flags + [src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "raycast_bricks_host_check: ok" in out.stdout, name + ": " + out.stdout + out.stderr
