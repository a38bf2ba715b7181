"""One launch per class-table build while the tables are staged in LDS (summary.hip, k_summary_classes_build): the fine level's
workgroups and, in the same grid, the 32^3-cell level's straight from the brick ranges; the published count carries its build's
stamp instead of an event behind the build.
  * the tables a tracked RaycastSdf marches through, and those of forced builds for the other fine levels, level by level: the
    fine level against the volume's real cells, the 32^3-cell level against the combination of the fine entries under each entry,
    the 64^3- and the 128^3-cell level (kfx_debug_summary_top_levels) against the combination of the 2 x 2 x 2 entries below;
  * a tracked RaycastSdf that follows a tracked SdfFuse issues exactly one launch for its tables, whether the build builds or
    returns early;
  * a stream the host never waits for: behind every frame whose build really built, the held tables are a forced build's."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import scenes
from test_gpu_summary import export, check_classes
from test_gpu_summary_change import conditional_builds, frame_inputs, held_equal_forced, images, shift_used, ORBIT, W, H

pytestmark = pytest.mark.gpu


def top_lib():
    from kangaroo_amd import _lib
    L = _lib.load_debug()
    L.kfx_debug_summary_top_levels.restype = C.c_int
    L.kfx_debug_summary_top_levels.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong), C.c_void_p]
    return L


def launches(summ):
    """kernel launches the summary's table builds have issued so far (a host-side counter)"""
    dims, n = (C.c_int * 12)(), C.c_ulonglong(0)
    assert top_lib().kfx_debug_summary_top_levels(summ.handle, 3, None, dims, C.byref(n), None) == 0
    return n.value


def top_levels(summ, fine_shift):
    """The 64^3- and 128^3-cell levels the summary holds behind tables built for `fine_shift`, decoded: {6: [nz, ny, nx], 7: ...}"""
    import torch
    dims = (C.c_int * 12)()
    assert top_lib().kfx_debug_summary_top_levels(summ.handle, fine_shift, None, dims, None, None) == 0
    words = torch.zeros(dims[5] + dims[11], dtype=torch.int32, device="cuda")
    assert top_lib().kfx_debug_summary_top_levels(summ.handle, fine_shift, C.c_void_p(words.data_ptr()), dims, None, None) == 0
    torch.cuda.synchronize()
    Wv, Hv, Dv = summ.vol.w, summ.vol.h, summ.vol.d
    out = {}
    for shift, (first, rw, ny, nx, nz, n_words) in ((6, dims[0:6]), (7, dims[6:12])):
        m = 1 << shift
        assert (nx, ny, nz) == (-(-Wv // m), -(-Hv // m), -(-Dv // m)) and rw == 2 * (-(-nx // 32)) and n_words >= rw * ny * nz
        w = words[first:first + rw * ny * nz].view(nz, ny, rw // 2, 2).to(torch.int64) & 0xffffffff
        bits = (w.unsqueeze(-1) >> torch.arange(32, device="cuda")) & 1
        p0 = bits[..., 0, :].reshape(nz, ny, -1)[..., :nx]
        p1 = bits[..., 1, :].reshape(nz, ny, -1)[..., :nx]
        out[shift] = (p0 | (p1 << 1)).to(torch.int8)
    assert dims[0] == 0 and dims[6] == dims[5]
    return out


def combine(below, m, shape):
    """The level above `below` ([nz, ny, nx] classes): an entry = the combination of the m^3 entries under it -- all 1 -> 1, all 2 -> 2,
    all non-zero -> 3, else 0; entries beyond the far edges repeat the last one."""
    import torch
    nz, ny, nx = shape
    b = below.to(torch.int64)
    iz = torch.arange(nz * m, device="cuda").clamp(max=b.shape[0] - 1)
    iy = torch.arange(ny * m, device="cuda").clamp(max=b.shape[1] - 1)
    ix = torch.arange(nx * m, device="cuda").clamp(max=b.shape[2] - 1)
    sub = b[iz][:, iy][:, :, ix].view(nz, m, ny, m, nx, m).permute(0, 2, 4, 1, 3, 5).reshape(nz, ny, nx, -1)
    all_free, all_nan, all_either = (sub == 1).all(-1), (sub == 2).all(-1), (sub != 0).all(-1)
    return torch.where(all_free, 1, torch.where(all_nan, 2, torch.where(all_either, 3, 0))).to(torch.int8)


def check_every_level(roo, summ, vol, tol, vref, fine_shift):
    """The tables for `fine_shift` (the held ones if the library holds tables for these parameters, else a forced build), every level.
    Returns the decoded classes {shift: tensor}."""
    _, classes = export(roo, summ, tol, vref, fine_shift=fine_shift)   # (also: published count == non-zero 32^3-cell entries)
    check_classes(vol, classes, tol, np.float32(vref))                 # the fine level (and the 32^3-cell one) against the cells
    if fine_shift < 5:
        want = combine(classes[fine_shift], 32 >> fine_shift, classes[5].shape)
        assert bool((want == classes[5]).all()), "32^3-cell level differs from the combination of its fine entries: %d" % int((want != classes[5]).sum())
    top = top_levels(summ, fine_shift)
    for shift, below in ((6, classes[5]), (7, top[6])):
        want = combine(below, 2, top[shift].shape)
        assert bool((want == top[shift]).all()), "2^%d-cell level differs from the 2 x 2 x 2 combination of the level below: %d" % (shift, int((want != top[shift]).sum()))
    classes.update(top)
    return classes


CASES = [("full", (256, 256, 256), (320, 240)), ("room", (200, 168, 232), (200, 150)), ("room", (96, 96, 96), (160, 120))]


def run_same_tables(roo, math):
    """Three tracked frames per case; after each, the tables the tracked RaycastSdf built (conditionally, in its one launch) and forced
    builds for the other fine levels, every level checked.  Returns the fine shifts the march used."""
    used = []
    prev = roo.set_math_mode(math)
    try:
        for scene, dims, (w, h) in CASES:
            bmin, bmax, near, far = scenes.SCENES[scene]
            K = scenes.intrinsics(w, h)
            tr = scenes.trunc_dist(bmin, bmax, dims)
            tol = 1e-5 if math == "fast" else 0.0
            vol = roo.BoundedVolume(*dims, bmin, bmax)
            summ = roo.SdfSummary(vol)
            shift = shift_used(summ)
            used.append(shift)
            roo.SdfReset(vol, float("nan"), summary=summ)
            f, vbo, nrm = roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h, "f32x4")
            nonzero = {}
            for i in range(3):
                T_wc = scenes.orbit_pose(3 * i, ORBIT)
                roo.BilateralFilter(f, T.upload_image(roo, scenes.render_depth(scene, w, h, T_wc, K)), **scenes.BILATERAL)
                roo.DepthToVbo(vbo, f, K)
                roo.NormalsFromVbo(nrm, vbo)
                roo.SdfFuse(vol, f, nrm, scenes.se3_inverse(T_wc), K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, summary=summ)
                roo.RaycastSdf(roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h), vol, T_wc, K, near, far, tr, True, summary=summ)
                n0 = launches(summ)
                classes = check_every_level(roo, summ, vol, tol, tr, shift)   # the march's own tables: held, nothing is built
                assert launches(summ) == n0
                for other in (3, 4, 5):
                    if other != shift:
                        check_every_level(roo, summ, vol, tol, tr, other)    # a change of parameters forces a build
                        assert launches(summ) == n0 + 1
                        n0 += 1
                for s, c in classes.items():
                    nonzero[s] = max(nonzero.get(s, 0), int((c != 0).sum()))
            if scene == "full" and math == "fast":
                # (the checks above would hold for tables of zeros: the free space in front of the wall must show)
                assert nonzero[shift] > 0 and nonzero[5] > 0, nonzero
            print("levels", scene, dims, math, "fine shift", shift, "entries of class != 0 at most:", nonzero, flush=True)
    finally:
        roo.set_math_mode(prev)
    return used


@pytest.mark.parametrize("math", ["exact", "fast"])
def test_gpu_same_tables_at_every_level(roo, math):
    used = run_same_tables(roo, math)
    assert used == [3, 3, 3], used   # 8^3-cell fine levels at these sizes (m = 4 under a 32^3-cell entry)


def test_gpu_same_tables_at_every_level_16_cell_fine_level():
    """KFX_RAYCAST_CLASS_KB=1: class_view picks the 16^3-cell fine level at 96^3 and the 32^3-cell level alone for the two larger
    volumes (the build kernel without a fine part); the knob is read once, so the cases run in a process of their own."""
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" % (T.ROOT, os.path.join(T.ROOT, "tests")) + \
           "import test_gpu_class_build_one_launch as M\nfrom kangaroo_amd import roo\n" + \
           "for math in ('exact', 'fast'):\n    used = M.run_same_tables(roo, math)\n    assert used == [5, 5, 4], used\nprint('LEVELS_OK')\n"
    env = dict(os.environ, KFX_RAYCAST_CLASS_KB="1", KFX_RAYCAST_SUMMARY="1")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    print(out.stdout)
    assert out.returncode == 0 and "LEVELS_OK" in out.stdout, out.stdout + out.stderr


def test_gpu_one_launch_per_build(roo):
    """Fast numerics, S_full 96^3: the first frame's build builds; the same frame fused again leaves every cell its bits (the
    running average of equal values), so no brick changes its class mask and the build returns early.  One launch either way."""
    N, scene = 96, "full"
    bmin, bmax, near, far = scenes.SCENES[scene]
    K = scenes.intrinsics(W, H)
    tr = scenes.trunc_dist(bmin, bmax, (N, N, N))
    prev = roo.set_math_mode("fast")
    try:
        vol = roo.BoundedVolume(N, N, N, bmin, bmax)
        summ = roo.SdfSummary(vol)
        roo.SdfReset(vol, float("nan"), summary=summ)
        T_wc, f, nrm = frame_inputs(roo, scene, K, 0, {})
        roo.RaycastSdf(*images(roo), vol, T_wc, K, near, far, tr, True, summary=summ)   # the empty model: a forced build
        assert launches(summ) == 1 and conditional_builds(summ) == (0, 0)
        moves = []
        for i in range(3):
            n0, c0 = launches(summ), conditional_builds(summ)
            roo.SdfFuse(vol, f, nrm, scenes.se3_inverse(T_wc), K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, summary=summ)
            assert launches(summ) == n0   # (SdfFuse builds no table)
            roo.RaycastSdf(*images(roo), vol, T_wc, K, near, far, tr, True, summary=summ)
            c1 = conditional_builds(summ)
            assert launches(summ) == n0 + 1, (i, n0, launches(summ))
            moves.append((c1[0] - c0[0], c1[1] - c0[1]))
            held_equal_forced(roo, summ, vol, 1e-5, tr, shift_used(summ), check_classes)
        assert moves == [(1, 0), (0, 1), (0, 1)], moves
        # a second RaycastSdf without a writer in between: the tables are current, nothing is issued
        n0 = launches(summ)
        roo.RaycastSdf(*images(roo), vol, T_wc, K, near, far, tr, True, summary=summ)
        assert launches(summ) == n0
    finally:
        roo.set_math_mode(prev)


def test_gpu_late_reader_cannot_see_a_cleared_flag(roo):
    """S_room 96^3, the orbit's 30 frames, tracked SdfFuse + tracked RaycastSdf.  A first pass (reading the counters after every
    frame) finds the frames whose conditional build really built; then, for each of them, the stream is issued again from SdfReset up
    to that frame without the host waiting for anything, and the tables held behind it must be a forced build's, word for word and
    with the same published count: no workgroup of the merged launch left rows stale (the ticket counts both levels' workgroups)."""
    import torch
    N, scene = 96, "room"
    bmin, bmax, near, far = scenes.SCENES[scene]
    K = scenes.intrinsics(W, H)
    tr = scenes.trunc_dist(bmin, bmax, (N, N, N))
    prev = roo.set_math_mode("fast")
    try:
        vol = roo.BoundedVolume(N, N, N, bmin, bmax)
        summ = roo.SdfSummary(vol)
        shift = shift_used(summ)
        cache = {}
        inputs = [frame_inputs(roo, scene, K, i, cache) for i in range(ORBIT)]
        out = images(roo)

        def stream(n, counted):
            roo.SdfReset(vol, float("nan"), summary=summ)
            roo.RaycastSdf(*out, vol, inputs[0][0], K, near, far, tr, True, summary=summ)
            built = []
            for i in range(n):
                T_wc, f, nrm = inputs[i]
                before = conditional_builds(summ) if counted else None
                roo.SdfFuse(vol, f, nrm, scenes.se3_inverse(T_wc), K, tr, scenes.MAX_W, scenes.MIN_COS_THETA, summary=summ)
                roo.RaycastSdf(*out, vol, T_wc, K, near, far, tr, True, summary=summ)
                if counted:
                    after = conditional_builds(summ)
                    assert (after[0] - before[0]) + (after[1] - before[1]) == 1, (i, before, after)
                    built.append(after[0] - before[0] == 1)
            return built

        torch.cuda.synchronize()
        built = stream(ORBIT, True)
        assert built[0] and sum(built) >= 5, built   # the scene is being discovered
        held_equal_forced(roo, summ, vol, 1e-5, tr, shift, check_classes)
        for k in [i for i, b in enumerate(built) if b]:
            l0, c0 = launches(summ), conditional_builds(summ)
            stream(k + 1, False)                      # nothing here waits for the device
            held_equal_forced(roo, summ, vol, 1e-5, tr, shift, check_classes)
            # (held_equal_forced's own builds: two forced ones; the stream's: the reset's forced one and k + 1 conditional ones)
            c1 = conditional_builds(summ)
            assert (c1[0] - c0[0]) + (c1[1] - c0[1]) == k + 1 and c1[0] - c0[0] == sum(built[:k + 1]), (k, c0, c1, built)
            assert launches(summ) - l0 == k + 2 + 2, (k, l0, launches(summ))
        print("late reader: frames of the orbit whose build built:", [i for i, b in enumerate(built) if b], flush=True)
    finally:
        roo.set_math_mode(prev)
