"""Colour mode without a GPU: the entry points of include/kfx_color.h are exported and bound and check their arguments before any
HIP call; scenes.render_rgb; FramePipeline's colour arguments."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import scenes
from kangaroo_amd import _lib

FAKE = 0x100000   # a non-null, 16-byte aligned address that is never dereferenced


def declared():
    src = open(os.path.join(T.ROOT, "include", "kfx_color.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kfx_[a-z0-9_]+)\s*\(", src)))


def volume(n, elem, ptr=FAKE):
    v = _lib.KfxVolume(n * elem, ptr, n, n, n * elem * n, n)
    for i in range(3):
        v.boxmin[i], v.boxmax[i] = -1.0, 1.0
    return v


def image(w, h, elem, ptr=FAKE):
    return _lib.KfxImage(w * elem, ptr, w, h)


def last_error():
    return _lib.load().kfx_last_error_string().decode()


def test_colour_symbols_are_exported_and_bound():
    L = _lib.load()
    names = declared()
    assert names == ["kfx_raycast_color_hits", "kfx_sdf_fuse_color_tracked"], names
    for n in names:
        assert hasattr(L, n), "libkfx.so does not export %s" % n
        assert n in _lib.SIGNATURES, "python binding missing for %s" % n
        restype, argtypes = _lib.SIGNATURES[n]
        args = [a(0.5) if a is C.c_float else (a(0) if a in (C.c_int, C.c_uint) else None) for a in argtypes]
        assert getattr(L, n)(*args) < 0, n


def test_tracked_colour_fuse_checks_its_arguments_before_any_launch():
    L = _lib.load()
    Tm = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    K = (C.c_float * 4)(50, 50, 31.5, 23.5)
    vol, cvol, small = volume(16, 8), volume(16, 4), volume(8, 4)
    depth, norm, rgb = image(64, 48, 4), image(64, 48, 16), image(64, 48, 3)
    R = C.byref

    def call(cv, summary):
        return L.kfx_sdf_fuse_color_tracked(R(vol), R(cv), summary, R(depth), R(norm), Tm, K, R(rgb), Tm, K, 0.1, 100.0, 0.1, 0, None)

    assert call(cvol, None) == -1 and "null summary" in last_error()                       # KFX_E_NULL
    # a summary that was not created for fp32 cells (here: a zeroed struct, cell size 0; a half-cell summary says 4): KFX_E_SHAPE
    other = C.create_string_buffer(4096)
    assert call(cvol, C.cast(other, C.c_void_p)) == -2 and "other cell type" in last_error()
    assert call(small, C.cast(other, C.c_void_p)) == -2 and "colour volume smaller" in last_error()
    assert L.kfx_sdf_fuse_color(R(vol), R(small), R(depth), R(norm), Tm, K, R(rgb), Tm, K, 0.1, 100.0, 0.1, 0, None) == -2


def test_colour_pass_checks_its_arguments_before_any_launch():
    L = _lib.load()
    Tm = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    K = (C.c_float * 36)(*([50, 50, 31.5, 23.5] * 9))
    cvol = volume(16, 4)
    PI = _lib.PI

    def call(n, depth, img, cv=cvol, nptr=None):
        nptr = n if nptr is None else nptr
        d = (PI * max(nptr, 1))(*[C.pointer(x) if x is not None else None for x in depth[:nptr]])
        i = (PI * max(nptr, 1))(*[C.pointer(x) if x is not None else None for x in img[:nptr]])
        return L.kfx_raycast_color_hits(n, d, i, C.byref(cv) if cv is not None else None, Tm, K, None)

    d9, i9 = [image(64, 48, 4) for _ in range(9)], [image(64, 48, 4) for _ in range(9)]
    assert call(0, d9, i9, nptr=1) == -4 and call(9, d9, i9) == -4                          # KFX_E_RANGE: 1 <= n_levels <= 8
    assert call(2, [d9[0], None], i9) == -1 and call(2, d9, [i9[0], None]) == -1            # a null level pointer
    assert call(1, [image(64, 48, 4, ptr=None)], i9) == -1 and call(1, d9, i9, cv=None) == -1
    assert L.kfx_raycast_color_hits(1, None, None, C.byref(cvol), Tm, K, None) == -1
    assert call(2, d9, [i9[0], image(32, 24, 4)]) == -2 and "different sizes" in last_error()   # KFX_E_SHAPE
    assert call(1, [image(64, 48, 4, ptr=FAKE + 2)], i9) == -3                              # KFX_E_ALIGN
    assert call(1, d9, i9, cv=volume(16, 4, ptr=None)) == -1


def test_render_rgb():
    w, h = 160, 120
    K = scenes.intrinsics(w, h)
    a = scenes.render_rgb("room", w, h, scenes.orbit_pose(3, 30), K)
    assert a.shape == (h, w, 3) and a.dtype == np.uint8 and a.flags.c_contiguous
    assert np.array_equal(a, scenes.render_rgb("room", w, h, scenes.orbit_pose(3, 30), K))   # deterministic
    assert np.array_equal(scenes.render_rgb("room", w, h), scenes.render_rgb("room", w, h, scenes.identity_pose(), K))
    assert (a[..., 0] != a[..., 1]).mean() > 0.5 and (a[..., 1] != a[..., 2]).mean() > 0.5 and (a[..., 0] != a[..., 2]).mean() > 0.5
    assert a.min() >= 27 and a.max() <= 228 and np.ptp(a[..., 0].astype(int)) > 100         # 127.5 +- 100, and it varies
    # a camera turned 75 degrees away from the wall of S_full sees it in a part of the image only: the rest is (0, 0, 0)
    c, s = np.cos(np.radians(75.0)), np.sin(np.radians(75.0))
    T_side = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0]], np.float32)
    miss = np.isnan(scenes.render_depth("full", w, h, T_side, K))
    b = scenes.render_rgb("full", w, h, T_side, K)
    assert 0.1 < miss.mean() < 0.9 and (b[miss] == 0).all() and (b[~miss].min(-1) > 0).all()


def test_render_rgb_albedo_does_not_depend_on_the_view():
    """A world point seen from two orbit poses gets colours within one grey step (the rounding to uint8): the second camera's
    principal point is chosen so that the point falls on a pixel centre."""
    w, h = 160, 120
    K = scenes.intrinsics(w, h)
    T_b, T_a = scenes.orbit_pose(5, 30), scenes.orbit_pose(20, 30)
    rgb_b, d_b = scenes.render_rgb("room", w, h, T_b, K), scenes.render_depth("room", w, h, T_b, K)
    compared = 0
    for v in range(10, h, 25):
        for u in range(10, w, 30):
            rc = np.array([(u - K[2]) / K[0], (v - K[3]) / K[1], 1.0])
            P = T_b[:, 3].astype(np.float64) + (T_b[:, :3].astype(np.float64) @ rc) * float(d_b[v, u])
            p = T_a[:, :3].astype(np.float64).T @ (P - T_a[:, 3])
            ua, va = int(round(K[0] * p[0] / p[2] + K[2])), int(round(K[1] * p[1] / p[2] + K[3]))
            if not (0 <= ua < w and 0 <= va < h):
                continue
            K_a = np.array([K[0], K[1], ua - K[0] * p[0] / p[2], va - K[1] * p[1] / p[2]], np.float32)
            if abs(float(scenes.render_depth("room", w, h, T_a, K_a)[va, ua]) - p[2]) > 1e-3:
                continue                                                                    # another surface in front of the point
            rgb_a = scenes.render_rgb("room", w, h, T_a, K_a)
            assert np.abs(rgb_a[va, ua].astype(int) - rgb_b[v, u].astype(int)).max() <= 1, (u, v, rgb_a[va, ua], rgb_b[v, u])
            compared += 1
    assert compared >= 10


def test_frame_pipeline_colour_arguments():
    import oracle_ops
    from kangaroo_amd.pipeline import FramePipeline
    bmin, bmax, near, far = scenes.SCENES["room"]
    with pytest.raises(ValueError):
        FramePipeline(oracle_ops, (16, 16, 16), bmin, bmax, 40, 30, near=near, far=far, color=True, track="auto")
    with pytest.raises(ValueError):
        FramePipeline(oracle_ops, (16, 16, 16), bmin, bmax, 40, 30, near=near, far=far, color=True, kind="f16")
    grey = FramePipeline(oracle_ops, (16, 16, 16), bmin, bmax, 40, 30, near=near, far=far)
    assert grey.color is False and not hasattr(grey, "cvol")
