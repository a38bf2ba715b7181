"""The half-cell summary entry points (include/kfx_summary_h.h) are exported by libkfx.so, have their ctypes bindings, and refuse
NULL arguments before any HIP call -- the checks test_abi_cpu.py makes for kfx.h, for the header it does not read.  No GPU."""
import ctypes as C
import os
import re

import kfx_testlib as T
from kangaroo_amd import _lib


def declared():
    src = open(os.path.join(T.ROOT, "include", "kfx_summary_h.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kfx_[a-z0-9_]+)\s*\(", src)))


def test_half_summary_symbols_are_exported_bound_and_check_null():
    L = _lib.load()
    names = declared()
    assert names == sorted(["kfx_sdf_summary_create_h", "kfx_sdf_reset_tracked_h", "kfx_sdf_fuse_tracked_h", "kfx_raycast_sdf_tracked_h",
                            "kfx_raycast_sdf_count_tracked_h", "kfx_raycast_sdf_levels_tracked_h"]), names
    for n in names:
        assert hasattr(L, n), "libkfx.so does not export %s" % n
        assert n in _lib.SIGNATURES, "python binding missing for %s" % n
        restype, argtypes = _lib.SIGNATURES[n]
        args = [a(0.5) if a is C.c_float else (a(0) if a in (C.c_int, C.c_uint) else None) for a in argtypes]
        assert getattr(L, n)(*args) == -1, n   # KFX_E_NULL
