"""The sensor input path (include/kfx_sensor.h) is exported by libkfx.so, has its ctypes bindings, stays out of kfx.h, and refuses
bad arguments before any HIP call: the image-argument rule of kfx_bilateral_depth and kfx_elementwise_scale_bias_u16 row by row
(as tests/test_abi_images_cpu.py has it for the other entry points), the ring's range and null checks, the frame hook's null frame.
No GPU: the pointers below are never dereferenced, and every row is a rejection or an empty launch."""
import ctypes as C
import os
import re

import kfx_testlib as T
from kangaroo_amd import _lib
from test_abi_images_cpu import E_ALIGN, E_NULL, E_SHAPE, FAKE, Family, image

E_RANGE = -4
R = C.byref
U16, F32 = 0, 1

NAMES = ["kfx_bilateral_depth", "kfx_depth_input_acquire", "kfx_depth_input_create", "kfx_depth_input_destroy", "kfx_depth_input_filter",
         "kfx_depth_input_pending", "kfx_depth_input_submit", "kfx_elementwise_scale_bias_u16", "kfx_frame_set_input"]


def declared(header):
    src = open(os.path.join(T.ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kfx_[a-z0-9_]+)\s*\(", src)))


def test_sensor_symbols_are_exported_and_bound_and_kfx_h_keeps_its_size():
    L = _lib.load()
    names = declared("kfx_sensor.h")
    assert names == NAMES, names
    for n in names:
        assert hasattr(L, n), "libkfx.so does not export %s" % n
        assert n in _lib.SIGNATURES, "python binding missing for %s" % n
    path = declared("kfx.h")
    assert len(path) <= 80 and not set(path) & set(names)


def families():
    L = _lib.load()
    out = []
    for fmt, elem in ((U16, 2), (F32, 4)):
        out.append(Family("kfx_bilateral_depth(format %d)" % fmt, [("filtered", 4, False), ("metres", 4, True), ("raw", elem, True)],
                          lambda a, fmt=fmt: L.kfx_bilateral_depth(R(a["filtered"]), R(a["metres"]), R(a["raw"]), fmt, 1e-3, 0.0, 1.5, 0.1, 3, 0.2, None),
                          empty=0))
    out.append(Family("kfx_elementwise_scale_bias_u16", [("out", 4, False), ("in", 2, True)],
                      lambda a: L.kfx_elementwise_scale_bias_u16(R(a["out"]), R(a["in"]), 1e-3, 0.0, None), empty=0))
    return out


def test_one_broken_rule_of_one_image_argument_gives_that_rules_code():
    wrong, n = [], 0
    for fam in families():
        for family, arg, rule, call, code in fam.rows():
            got = call()
            n += 1
            if got != code:
                wrong.append((family, arg, rule, "expected %d, got %d" % (code, got)))
    assert not wrong, wrong
    assert n >= 40, n


def test_bilateral_depth_refusals_and_empty_launches():
    L = _lib.load()
    f, m, r16 = image(4), image(4), image(2)
    # the metres image is optional: a null POINTER is "no metres image", an image without memory is a broken argument
    assert L.kfx_bilateral_depth(R(f), None, None, U16, 1e-3, 0.0, 1.5, 0.1, 3, 0.2, None) == E_NULL
    assert L.kfx_bilateral_depth(None, None, R(r16), U16, 1e-3, 0.0, 1.5, 0.1, 3, 0.2, None) == E_NULL
    assert L.kfx_bilateral_depth(R(f), R(image(4, ptr=None)), R(r16), U16, 1e-3, 0.0, 1.5, 0.1, 3, 0.2, None) == E_NULL
    # a u16 row is too short a pitch for float pixels: the format decides the pixel size
    assert L.kfx_bilateral_depth(R(f), R(m), R(r16), F32, 1e-3, 0.0, 1.5, 0.1, 3, 0.2, None) == E_SHAPE
    assert L.kfx_bilateral_depth(R(f), R(m), R(image(2, ptr=FAKE + 1)), U16, 1e-3, 0.0, 1.5, 0.1, 3, 0.2, None) == E_ALIGN
    for bad in (-1, 2, 7):
        assert L.kfx_bilateral_depth(R(f), R(m), R(r16), bad, 1e-3, 0.0, 1.5, 0.1, 3, 0.2, None) == E_RANGE
    assert L.kfx_bilateral_depth(R(f), R(m), R(r16), U16, 1e-3, 0.0, 1.5, 0.1, 1025, 0.2, None) == E_RANGE
    # an empty launch is no launch: 0, with and without the metres image
    for empty in (image(4, 16, 0), image(4, 0, 8)):
        assert L.kfx_bilateral_depth(R(empty), R(m), R(r16), U16, 1e-3, 0.0, 1.5, 0.1, 3, 0.2, None) == 0
        assert L.kfx_bilateral_depth(R(empty), None, R(r16), U16, 1e-3, 0.0, 1.5, 0.1, 3, 0.2, None) == 0
        assert L.kfx_elementwise_scale_bias_u16(R(empty), R(r16), 1e-3, 0.0, None) == 0


def test_depth_input_create_refuses_before_it_allocates():
    L = _lib.load()
    h = C.c_void_p(FAKE)
    assert L.kfx_depth_input_create(None, 64, 48, U16, 1e-3, 0.0, 2) == E_NULL
    for fmt in (-1, 2, 16):
        assert L.kfx_depth_input_create(R(h), 64, 48, fmt, 1e-3, 0.0, 2) == E_RANGE and not h.value
    for slots in (-1, 0, 1, 9, 1 << 20):
        h = C.c_void_p(FAKE)
        assert L.kfx_depth_input_create(R(h), 64, 48, U16, 1e-3, 0.0, slots) == E_RANGE and not h.value
    for w, hh in ((0, 48), (64, 0), (0, 0), ((1 << 30) + 1, 48)):
        h = C.c_void_p(FAKE)
        assert L.kfx_depth_input_create(R(h), w, hh, F32, 1e-3, 0.0, 2) == E_SHAPE and not h.value
    # the other entry points with no ring
    ptr, pitch = C.c_void_p(), C.c_size_t()
    assert L.kfx_depth_input_acquire(None, R(ptr), R(pitch)) == E_NULL
    assert L.kfx_depth_input_submit(None) == E_NULL
    assert L.kfx_depth_input_pending(None) == E_NULL
    assert L.kfx_depth_input_filter(None, R(image(4)), None, 1.5, 0.1, 3, 0.2, None) == E_NULL
    assert L.kfx_depth_input_destroy(None) == E_NULL


def test_frame_set_input_refuses_a_null_frame():
    L = _lib.load()
    assert L.kfx_frame_set_input(None, None) == E_NULL
    assert L.kfx_frame_set_input(None, FAKE) == E_NULL
