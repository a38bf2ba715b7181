"""Colour mode on Z-slabs without a GPU: include/kfx_slab_color.h declares exactly the agreed entry points, libkfx.so exports them and
kangaroo_amd._lib binds them; each checks its arguments before any HIP call (a fake non-null pointer is never dereferenced); the frame
configuration keeps its size; the combinations that stay refused raise ValueError with the reason."""
import ctypes as C
import os
import re

import pytest

import kfx_testlib as T
from kfx_testlib import scenes
from kangaroo_amd import _lib

FAKE = 0x100000   # a non-null, 16-byte aligned address that is never dereferenced
E_NULL, E_SHAPE = -1, -2
NAMES = ["kfx_raycast_sdf_slab_color", "kfx_raycast_sdf_slab_tiles_color", "kfx_sdf_fuse_color_slab", "kfx_slab_frame_set_color",
         "kfx_slab_raycast_exact_tiled_color"]
R = C.byref
Tm = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
K = (C.c_float * 4)(50, 50, 31.5, 23.5)


def declared(header):
    src = open(os.path.join(T.ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kfx_[a-z0-9_]+)\s*\(", src)))


def volume(w, h, d, elem, ptr=FAKE, zmax=1.0):
    v = _lib.KfxVolume(w * elem, ptr, w, h, w * elem * h, d)
    for i in range(3):
        v.boxmin[i], v.boxmax[i] = -1.0, 1.0
    v.boxmax[2] = zmax
    return v


def image(w, h, elem, ptr=FAKE):
    return _lib.KfxImage(w * elem, ptr, w, h)


def last_error():
    return _lib.load().kfx_last_error_string().decode()


def test_header_declares_the_colour_slab_entry_points_and_they_are_exported_and_bound():
    L = _lib.load()
    assert declared("kfx_slab_color.h") == NAMES
    assert declared("kfx_color.h") == ["kfx_raycast_color_hits", "kfx_sdf_fuse_color_tracked"]   # (that header keeps its two)
    for n in NAMES:
        assert hasattr(L, n), "libkfx.so does not export %s" % n
        assert n in _lib.SIGNATURES, "python binding missing for %s" % n


def test_called_with_nulls_each_returns_null():
    L = _lib.load()
    for n in NAMES:
        restype, argtypes = _lib.SIGNATURES[n]
        args = [a(0.5) if a is C.c_float else (a(0) if a in (C.c_int, C.c_uint, C.c_size_t) else None) for a in argtypes]
        assert getattr(L, n)(*args) == E_NULL, (n, last_error())
    assert L.kfx_slab_frame_set_color(None, R(volume(16, 16, 16, 4)), R(image(64, 48, 3)), K, None) == E_NULL


def shape_cases():
    """(colour slab, reason) pairs beside a 16 x 16 x 12 SDF slab with box [-1, 1]^2 x [-1, 0.5]"""
    return [(volume(8, 16, 12, 4, zmax=0.5), "dimensions"), (volume(16, 8, 12, 4, zmax=0.5), "dimensions"), (volume(16, 16, 16, 4, zmax=0.5), "dimensions"),
            (volume(16, 16, 12, 4, zmax=0.75), "box")]


def test_colour_fuse_on_a_slab_refuses_another_geometry_before_any_launch():
    L = _lib.load()
    vol = volume(16, 16, 12, 8, zmax=0.5)
    slab = _lib.KfxSlab(32, 4, -1.0, 1.0)
    depth, norm, rgb = image(64, 48, 4), image(64, 48, 16), image(64, 48, 3)

    def call(cv, sl=slab):
        return L.kfx_sdf_fuse_color_slab(R(vol), R(cv), R(sl) if sl is not None else None, R(depth), R(norm), Tm, K, R(rgb), Tm, K, 0.1, 100.0, 0.1, 2, None)

    for cv, why in shape_cases():
        assert call(cv) == E_SHAPE and why in last_error() and "colour slab" in last_error(), (why, last_error())
    assert call(volume(16, 16, 12, 4, zmax=0.5), None) == E_NULL and "null slab" in last_error()
    assert call(volume(16, 16, 12, 4, zmax=0.5), _lib.KfxSlab(32, 24, -1.0, 1.0)) == E_SHAPE and "outside the full volume" in last_error()
    assert call(volume(16, 16, 12, 4, ptr=None, zmax=0.5)) == E_NULL


def test_colour_march_on_a_slab_refuses_another_geometry_before_any_launch():
    L = _lib.load()
    vol = volume(16, 16, 12, 8, zmax=0.5)
    slab = _lib.KfxSlab(32, 4, -1.0, 1.0)
    state = C.c_void_p(FAKE)
    for cv, why in shape_cases():
        assert L.kfx_raycast_sdf_slab_color(state, 1, R(vol), R(cv), R(slab), 6, 14, 64, 48, Tm, K, 0.4, 8.0, 0.1, 1, None) == E_SHAPE
        assert why in last_error() and "colour slab" in last_error(), (why, last_error())
        assert L.kfx_raycast_sdf_slab_tiles_color(state, state, 64 * 12, 12, 0, 12, 1, None, 0, None, None, 6, R(vol), R(cv), R(slab), 6, 14, 64, 48, Tm, K,
                                                  0.4, 8.0, 0.1, 1, None) == E_SHAPE
        assert why in last_error(), (why, last_error())
    good = volume(16, 16, 12, 4, zmax=0.5)
    assert L.kfx_raycast_sdf_slab_color(state, 1, R(vol), None, R(slab), 6, 14, 64, 48, Tm, K, 0.4, 8.0, 0.1, 1, None) == E_NULL
    assert L.kfx_raycast_sdf_slab_color(None, 1, R(vol), R(good), R(slab), 6, 14, 64, 48, Tm, K, 0.4, 8.0, 0.1, 1, None) == E_NULL


def test_colour_hand_over_and_frame_refuse_another_geometry_before_any_launch():
    from kangaroo_amd import slab as S
    L = _lib.load()   # (through _lib.SIGNATURES: the layout, the communicator and the frame travel as void*)
    lay = S.KfxSlabLayout(32, -1.0, 1.0, 0, 1, 2, 0, 32, 0, 32, -1.0, 1.0)   # one rank (a transport without exchange_v serves it)
    d = lay.s1 - lay.s0
    zlo = lay.local_zmin
    vol = volume(16, 16, d, 8)
    vol.boxmin[2] = zlo
    comm = S.KfxComm()
    comm.rank, comm.world = 0, 1
    dep, nrm, img = image(64, 48, 4), image(64, 48, 16), image(64, 48, 4)
    scratch = C.c_void_p(FAKE)

    def colour(w=16, h=16, dd=d, z0=zlo, z1=1.0):
        v = volume(w, h, dd, 4, zmax=z1)
        v.boxmin[2] = z0
        return v

    def march(cv):
        return L.kfx_slab_raycast_exact_tiled_color(R(dep), R(nrm), R(img), scratch, R(vol), R(cv) if cv is not None else None, R(lay), Tm, K, 0.4, 8.0, 0.1, 1, 4,
                                                    R(comm), None, None, None)

    assert march(None) == E_NULL and "null colour volume" in last_error()
    for cv, why in ((colour(w=8), "dimensions"), (colour(dd=d - 1), "dimensions"), (colour(z0=-0.5), "box"), (colour(z1=0.5), "box")):
        assert march(cv) == E_SHAPE and why in last_error() and "colour slab" in last_error(), (why, last_error())
    # the frame object: created without timing slots it needs no device ... (kfx_slab_frame_create allocates: not here); a null frame
    assert L.kfx_slab_frame_set_color(None, R(colour()), R(image(64, 48, 3)), K, None) == E_NULL and "null frame" in last_error()


def test_slab_frame_config_keeps_its_size():
    """The colour arguments travel through kfx_slab_frame_set_color, not through the configuration struct: a C program that includes
    the new header measures the struct at the 744 bytes it had before colour mode, the size of the ctypes mirror, and the struct's
    text names no colour member."""
    import subprocess
    import tempfile
    from kangaroo_amd import slab as S
    code = '#include <cstdio>\n#include "kfx_slab_color.h"\nint main(){ printf("%zu\\n", sizeof(kfx_slab_frame_config)); }\n'
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.cpp"), "w").write(code)
        subprocess.check_call(["g++", "-I", os.path.join(T.ROOT, "include"), os.path.join(td, "s.cpp"), "-o", os.path.join(td, "s")])
        size = int(subprocess.check_output([os.path.join(td, "s")]))
    assert size == C.sizeof(S.KfxSlabFrameConfig) == 744
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(T.ROOT, "include", "kfx_slab.h")).read(), flags=re.S)
    body = re.search(r"typedef struct kfx_slab_frame_config \{(.*?)\} kfx_slab_frame_config;", src, re.S).group(1)
    assert "color" not in body and "colour" not in body and "rgb" not in body


def test_combinations_that_stay_refused_say_why():
    import oracle_ops
    from kangaroo_amd.pipeline import SlabPipeline, TrackingSlabPipeline

    class Dist:   # a one-rank stand-in: the constructors only ask for rank and world before they refuse
        @staticmethod
        def get_rank():
            return 0

        @staticmethod
        def get_world_size():
            return 1

    bmin, bmax, near, far = scenes.SCENES["room"]
    with pytest.raises(ValueError, match="fp32 cells"):
        SlabPipeline(oracle_ops, Dist, (16, 16, 16), bmin, bmax, 40, 30, near=near, far=far, color=True, kind="f16")
    with pytest.raises(ValueError, match="color=True is not built"):
        TrackingSlabPipeline(oracle_ops, Dist, (16, 16, 16), bmin, bmax, 40, 30, near=near, far=far, color=True)
    with pytest.raises(ValueError, match="exact_allreduce"):
        SlabPipeline(oracle_ops, Dist, (16, 16, 16), bmin, bmax, 40, 30, near=near, far=far, color=True, raycast="exact_allreduce")
