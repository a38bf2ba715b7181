"""Sparse brick snapshots on the GPU (include/kfx_bricks.h, roo.BrickPack / BrickUnpack, kangaroo_amd/bricks.py,
FramePipeline(follow=dict(spill=True))).  The reference is numpy on the storage bytes.

  * pack equals numpy byte for byte -- the count, the ids, the cells, the fill bytes where a partial brick leaves the view -- with
    nothing written behind the lists, and unpack after a fill restores every BYTE of the storage: pitch padding and the neighbours
    of a sub-view included;
  * a pack with another count than the plan's is refused and writes nothing; a subset unpacks exactly its bricks;
  * a volume that spills what a shift discards gets it back when it returns, bit for bit, with a summary the table march can
    trust -- and without the spill the same cells come back empty;
  * SaveBricks -> LoadBricks reproduces a volume."""
import ctypes as C

import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import scenes

pytestmark = pytest.mark.gpu

NAN = float("nan")
LO, HI = (-1.0, -1.0, 2.0), (1.0, 1.0, 4.0)
E_RANGE = -4
GUARD = 0xA5
# (name, cell kind, dims, pitch, view (start, size) or None, fill)
CASES = [
    ("f32", "f32", (40, 24, 16), None, None, NAN),
    # rows that start 8-byte aligned only, partial bricks in z; the neighbours of the view are storage that must not change
    ("f32-subview", "f32", (40, 24, 16), None, ((3, 2, 1), (32, 16, 12)), NAN),
    ("f16", "f16", (72, 16, 24), None, None, NAN),
    ("f16-subview", "f16", (72, 16, 24), None, ((1, 2, 1), (66, 9, 20)), NAN),
    # a pitch that is no multiple of 16: every row has its own distance to the 16-byte boundary below it
    ("f16-odd-pitch", "f16", (41, 5, 6), 41 * 4 + 4, None, NAN),
    ("colour", "c32", (40, 24, 16), None, None, 0.5),
    ("colour-zero-fill", "c32", (40, 24, 16), None, None, 0.0),   # (the -0.0 trap)
    ("colour-odd-pitch", "c32", (37, 6, 5), 37 * 4, None, 0.5),
    # 3 x 5500 = 16500 bricks: more than one scan block (256) and more than one pass of the wave that scans the blocks (64 x 256)
    ("f16-column", "f16", (8, 24, 8 * 5500), 8 * 4, None, NAN),
    # more than one run of 1 KiB per row: 5 runs of 16 bricks (f32), the last one short
    ("f32-wide", "f32", (600, 9, 8), None, None, NAN),
]


def _cells(buf, vol):
    """strided (d, h, w) view of the cells of `vol` (a roo volume or view) in the byte array `buf` of its storage"""
    dt = np.uint64 if vol.ELEM == 8 else np.uint32
    n = (vol.d - 1) * vol.img_pitch + (vol.h - 1) * vol.pitch + vol.w * vol.ELEM
    return np.lib.stride_tricks.as_strided(buf[vol.offset:vol.offset + n].view(dt), (vol.d, vol.h, vol.w), (vol.img_pitch, vol.pitch, vol.ELEM))


_FILL_BITS = {}


def _fill_bits(roo, kind, fill):
    """the bytes of a cell after the matching reset (computed once per kind and fill)"""
    import torch
    key = (kind, np.float32(fill).tobytes())
    if key not in _FILL_BITS:
        if kind == "c32":
            _FILL_BITS[key] = np.array([fill], np.float32).view(np.uint32)[0]
        else:
            v = roo.BoundedVolume(8, 8, 8, kind=kind)
            roo.SdfReset(v, fill)
            torch.cuda.synchronize()
            _FILL_BITS[key] = _cells(v.storage.cpu().numpy(), v)[3, 4, 5]
    return _FILL_BITS[key]


def _grid(vol):
    return (vol.w + 7) // 8, (vol.h + 7) // 8, (vol.d + 7) // 8


def _numpy_pack(cells, fill_bits):
    """(ids, bricks (n, 512)) of a (d, h, w) array of cells: padded with the fill to whole bricks, brick id = (bz * nby + by) * nbx + bx"""
    d, h, w = cells.shape
    nbx, nby, nbz = (w + 7) // 8, (h + 7) // 8, (d + 7) // 8
    padded = np.full((nbz * 8, nby * 8, nbx * 8), fill_bits, cells.dtype)
    padded[:d, :h, :w] = cells
    bricks = padded.reshape(nbz, 8, nby, 8, nbx, 8).transpose(0, 2, 4, 1, 3, 5).reshape(nbz * nby * nbx, 512)
    ids = np.flatnonzero((bricks != fill_bits).any(axis=1))
    return ids.astype(np.uint32), np.ascontiguousarray(bricks[ids])


def _traps(kind, fill, fill_bits):
    """cells that differ from the fill cell in the ways a float comparison, or one of the val half alone, would miss"""
    fb = int(fill_bits)
    if kind == "f32":     # uint64: val in the low word, w in the high word
        return [("corner", fb ^ 0x00c00000), ("w-only", fb | (0x3f800000 << 32)), ("nan-payload", (fb & ~0xffffffff) | 0x7fc00001)]
    if kind == "f16":     # uint32: val in the low half, w in the high half
        return [("corner", fb ^ 0x0200), ("w-only", fb | (0x3c00 << 16)), ("nan-payload", (fb & ~0xffff) | 0x7e01)]
    traps = [("corner", fb ^ 0x00400000), ("nan-payload", 0x7fc00001)]
    if fill == 0.0:
        traps.append(("minus-zero", 0x80000000))
    return traps


def _brick_slices(vol, bid):
    nbx, nby, _ = _grid(vol)
    bx, by, bz = bid % nbx, (bid // nbx) % nby, bid // (nbx * nby)
    return slice(bz * 8, min(bz * 8 + 8, vol.d)), slice(by * 8, min(by * 8 + 8, vol.h)), slice(bx * 8, min(bx * 8 + 8, vol.w))


def _scene(roo, case, seed=11):
    """The storage of a case: random bytes everywhere (the sentinel), then the view's cells set to the fill in about 60 % of its
    bricks, and one trap brick per trap: all fill but a single cell.  Returns (vol, view, before bytes, fill bits, trap ids)."""
    import torch
    _, kind, dims, pitch, view, fill = case
    fill_bits = _fill_bits(roo, kind, fill)
    rng = np.random.default_rng(seed)
    vol = roo.BoundedVolume(dims[0], dims[1], dims[2], LO, HI, pitch=pitch, kind=kind)
    before = rng.integers(0, 256, vol.storage.numel(), dtype=np.uint8)
    tgt = vol if view is None else vol.SubVolume(*view)
    cells = _cells(before, tgt)
    nb = int(np.prod(_grid(tgt)))
    order = rng.permutation(nb)
    traps = _traps(kind, fill, fill_bits)[:max(nb - 2, 1)]
    trap_ids = {}
    for (name, bits), bid in zip(traps, order):
        sz, sy, sx = _brick_slices(tgt, int(bid))
        cells[sz, sy, sx] = fill_bits
        # the brick's far corner -- (7, 7, 7) of a whole brick -- for the first trap, a cell in its middle for the others
        at = (sz.stop - 1, sy.stop - 1, sx.stop - 1) if name == "corner" else tuple((s.start + min(k, s.stop - s.start - 1)) for s, k in zip((sz, sy, sx), (5, 4, 3)))
        cells[at] = bits
        trap_ids[name] = int(bid)
    rest = order[len(traps):]
    blank = rng.random(rest.size) < 0.6
    blank[0], blank[-1] = True, False   # (the smallest grids too have a brick of each sort)
    for bid in rest[blank]:
        cells[_brick_slices(tgt, int(bid))] = fill_bits
    vol.storage.copy_(torch.from_numpy(before))
    return vol, tgt, before, fill_bits, trap_ids


def _pack_guarded(roo, tgt, fill):
    """kfx_bricks_plan + kfx_bricks_pack into buffers with a guard region behind the lists; (n, ids, cells, guards intact)"""
    import torch
    from kangaroo_amd import _lib
    L, kind = _lib.load(), roo.CELL_KIND[tgt.kind]
    need = roo.BrickScratchBytes(tgt)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    n = C.c_ulonglong(0)
    _lib.check(L.kfx_bricks_plan(tgt.ref(), kind, fill, scratch.data_ptr(), need, C.byref(n), None))
    n, bb = n.value, roo.brick_bytes(tgt)
    ids = torch.full((n * 4 + 256,), GUARD, dtype=torch.uint8, device="cuda")
    cells = torch.full((n * bb + 4096,), GUARD, dtype=torch.uint8, device="cuda")
    _lib.check(L.kfx_bricks_pack(tgt.ref(), kind, fill, scratch.data_ptr(), need, n, ids.data_ptr(), cells.data_ptr(), None))
    torch.cuda.synchronize()
    intact = bool((ids[n * 4:] == GUARD).all()) and bool((cells[n * bb:] == GUARD).all())
    return n, ids[:n * 4].cpu().numpy().view(np.uint32), cells[:n * bb].cpu().numpy().reshape(n, bb), intact


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gpu_pack_equals_numpy_and_unpack_restores_every_byte(roo, case):
    import torch
    _, kind, dims, pitch, view, fill = case
    vol, tgt, before, fill_bits, trap_ids = _scene(roo, case)
    want_ids, want_cells = _numpy_pack(_cells(before, tgt), fill_bits)
    nb = int(np.prod(_grid(tgt)))
    print("%s: %d bricks, %d live, traps %s" % (case[0], nb, want_ids.size, trap_ids))
    assert set(trap_ids.values()) <= set(want_ids.tolist()) and 0 < want_ids.size < nb   # the traps are live in the reference; some bricks are not
    n, ids, cells, intact = _pack_guarded(roo, tgt, fill)
    assert n == want_ids.size, (n, want_ids.size, sorted(set(want_ids.tolist()) ^ set(ids.tolist()))[:8])
    assert np.array_equal(ids, want_ids)
    got = cells.view(want_cells.dtype)
    bad = np.argwhere(got != want_cells)
    assert bad.size == 0, (case[0], "%d cells differ, first (entry, cell) %s" % (len(bad), bad[:4].tolist()))
    assert intact, "written behind n_live entries"
    assert np.array_equal(vol.storage.cpu().numpy(), before)   # packing reads
    # the operator returns the same lists
    r_ids, r_cells = roo.BrickPack(tgt, fill)
    assert np.array_equal(r_ids.cpu().numpy().view(np.uint32), want_ids) and np.array_equal(r_cells.cpu().numpy(), cells)
    # every cell of the view the fill -- and nothing else touched -- then the bricks back: the storage as it was
    roo.VolumeFill(tgt, fill)
    torch.cuda.synchronize()
    blank = before.copy()
    _cells(blank, tgt)[...] = fill_bits
    assert np.array_equal(vol.storage.cpu().numpy(), blank)
    roo.BrickUnpack(tgt, r_ids, r_cells)
    torch.cuda.synchronize()
    after = vol.storage.cpu().numpy()
    bad = np.flatnonzero(after != before)
    assert bad.size == 0, (case[0], "%d bytes differ, first at %s" % (bad.size, bad[:8].tolist()))


def test_gpu_pack_refuses_a_count_that_is_not_the_plans_and_writes_nothing(roo):
    import torch
    from kangaroo_amd import _lib
    L = _lib.load()
    vol, tgt, before, fill_bits, _ = _scene(roo, CASES[0])
    need = roo.BrickScratchBytes(tgt)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    n = C.c_ulonglong(0)
    _lib.check(L.kfx_bricks_plan(tgt.ref(), 0, NAN, scratch.data_ptr(), need, C.byref(n), None))
    assert 1 < n.value < 30
    ids = torch.full((4 * 64,), GUARD, dtype=torch.uint8, device="cuda")
    cells = torch.full((64 * 4096,), GUARD, dtype=torch.uint8, device="cuda")
    for wrong in (n.value + 1, n.value - 1, 0, 30):
        assert L.kfx_bricks_pack(tgt.ref(), 0, NAN, scratch.data_ptr(), need, wrong, ids.data_ptr(), cells.data_ptr(), None) == E_RANGE, wrong
    torch.cuda.synchronize()
    assert bool((ids == GUARD).all()) and bool((cells == GUARD).all())
    assert L.kfx_bricks_pack(tgt.ref(), 0, NAN, scratch.data_ptr(), need, n.value, ids.data_ptr(), cells.data_ptr(), None) == 0   # the plan is still good
    torch.cuda.synchronize()
    want_ids, _ = _numpy_pack(_cells(before, tgt), fill_bits)
    assert np.array_equal(ids.cpu().numpy().view(np.uint32)[:n.value], want_ids)


@pytest.mark.parametrize("case", [CASES[1], CASES[4]], ids=[CASES[1][0], CASES[4][0]])
def test_gpu_unpack_of_a_subset_changes_exactly_those_bricks(roo, case):
    import torch
    _, kind, dims, pitch, view, fill = case
    vol, tgt, before, fill_bits, _ = _scene(roo, case)
    ids, cells = roo.BrickPack(tgt, fill)
    ids_h, cells_h = ids.cpu().numpy().view(np.uint32), cells.cpu().numpy()
    nb = int(np.prod(_grid(tgt)))
    pick = np.arange(0, ids_h.size, 3)
    roo.VolumeFill(tgt, fill)
    roo.BrickUnpack(tgt, ids_h[pick], cells_h[pick])
    torch.cuda.synchronize()
    expect = before.copy()
    _cells(expect, tgt)[...] = fill_bits
    for bid in ids_h[pick]:
        sl = _brick_slices(tgt, int(bid))
        _cells(expect, tgt)[sl] = _cells(before, tgt)[sl]
    assert np.array_equal(vol.storage.cpu().numpy(), expect)
    # a list that ends in ids at and beyond the brick count: those entries are skipped, nothing outside the view changes
    roo.VolumeFill(tgt, fill)
    rng = np.random.default_rng(5)
    extra = rng.integers(0, 256, (2, cells_h.shape[1]), dtype=np.uint8)
    roo.BrickUnpack(tgt, np.concatenate([ids_h[pick], [nb, nb + 1000]]), np.concatenate([cells_h[pick], extra]))
    torch.cuda.synchronize()
    assert np.array_equal(vol.storage.cpu().numpy(), expect)
    with pytest.raises(ValueError, match="ascending"):
        roo.BrickUnpack(tgt, ids_h[pick][::-1].copy(), cells_h[pick])
    with pytest.raises(ValueError, match="ascending"):
        roo.BrickUnpack(tgt, np.array([1, 1]), cells_h[:2])


def _images_equal(a, b):
    return all(np.array_equal(x.MemcpyToHost().view(np.uint32), y.MemcpyToHost().view(np.uint32)) for x, y in zip(a, b))


def test_gpu_a_spilling_volume_gets_back_what_it_left_behind(roo, tmp_path):
    """32^3 on the lattice whose positions are exact in fp32 (tests/test_gpu_shift.py), tracked, in colour.  (8, 0, -8) and back:
    with the spill both volumes are what they were, bit for bit, and both stores are empty again; without it the cells that left
    come back as the fill -- which is what this test fails on where a shift only discards."""
    import torch
    from kangaroo_amd.bricks import LoadBricks, SaveBricks
    from kangaroo_amd.pipeline import FramePipeline
    N, w, h = 32, 80, 60
    lo, hi = (-1.0, -1.0, 2.0), (0.9375, 0.9375, 3.9375)
    there, back = (8, 0, -8), (-8, 0, 8)
    p = FramePipeline(roo, (N, N, N), lo, hi, w, h, track=True, color=True, follow=dict(quantum=8, spill=True))
    q = FramePipeline(roo, (N, N, N), lo, hi, w, h, track=True, color=True, follow=dict(quantum=8))
    assert p.spill and not q.spill and q.store is None and len(p.store) == 0 and len(p.cstore) == 0
    for i in range(3):
        T_wc = scenes.orbit_pose(i, 8)
        raw = T.upload_image(roo, scenes.render_depth("room", w, h, T_wc, p.K))
        rgb = roo.Image(w, h, "u8x3").MemcpyFromHost(scenes.render_rgb("room", w, h, T_wc, p.Kimg))
        p.step(T_wc, raw, rgb)
        q.step(T_wc, raw, rgb)
    torch.cuda.synchronize()
    assert p.shifts == [] and q.shifts == []   # the camera stayed inside the slack: the only shifts are the two below
    sdf0, col0 = p.vol.storage.cpu().numpy().copy(), p.cvol.storage.cpu().numpy().copy()
    assert np.array_equal(sdf0, q.vol.storage.cpu().numpy()) and np.array_equal(col0, q.cvol.storage.cpu().numpy())
    box0 = (p.vol.boxmin.copy(), p.vol.boxmax.copy())
    sdf_fill, col_fill = _fill_bits(roo, "f32", NAN), _fill_bits(roo, "c32", 0.5)
    left = np.zeros((N, N, N), bool)            # [z, y, x]: what (8, 0, -8) discards, and what (-8, 0, 8) exposes
    left[:, :, :8] = True
    left[24:, :, :] = True
    live0, clive0 = _cells(sdf0, p.vol) != sdf_fill, _cells(col0, p.cvol) != col_fill
    counts = [int((live0 & left).sum()), int((clive0 & left).sum()), int((live0 & ~left).sum())]
    print("cells that differ from the fill: %d SDF and %d colour cells in the part that leaves, %d SDF cells in the part that stays" % tuple(counts))
    assert min(counts) > 0   # there is something to lose and something to keep

    for pipe in (p, q):
        pipe.shift_volume(there)
    torch.cuda.synchronize()
    assert len(p.store) > 0 and len(p.cstore) > 0 and p.store.nbytes == 4096 * len(p.store) and p.cstore.nbytes == 2048 * len(p.cstore)
    assert p.origin == there and p.restored == 0
    assert np.array_equal(p.vol.storage.cpu().numpy(), q.vol.storage.cpu().numpy())   # on the way out the spill changes nothing on the device
    for pipe in (p, q):
        pipe.shift_volume(back)
    torch.cuda.synchronize()
    assert p.origin == (0, 0, 0) and p.restored > 0
    assert np.array_equal(p.vol.boxmin.view(np.uint32), box0[0].view(np.uint32)) and np.array_equal(p.vol.boxmax.view(np.uint32), box0[1].view(np.uint32))
    # without the spill: retained cells as they were, the cells that left are the fill
    got_q, gotc_q = _cells(q.vol.storage.cpu().numpy(), q.vol), _cells(q.cvol.storage.cpu().numpy(), q.cvol)
    assert np.array_equal(got_q[~left], _cells(sdf0, q.vol)[~left]) and np.all(got_q[left] == sdf_fill)
    assert np.array_equal(gotc_q[~left], _cells(col0, q.cvol)[~left]) and np.all(gotc_q[left] == col_fill)
    # with it: every byte of both storages, and nothing left on the host
    assert np.array_equal(p.vol.storage.cpu().numpy(), sdf0), "the SDF volume did not come back"
    assert np.array_equal(p.cvol.storage.cpu().numpy(), col0), "the colour volume did not come back"
    assert len(p.store) == 0 and len(p.cstore) == 0 and p.store.nbytes == 0
    # the summary was rebuilt after the restore: the table march renders the plain march's bits
    T_wc = scenes.orbit_pose(2, 8)
    near, far = p.near, p.far
    a, b = (roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h)), (roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h))
    roo.RaycastSdf(a[0], a[1], a[2], p.vol, T_wc, p.K, near, far, p.trunc, True, summary=p.summary)
    roo.RaycastSdf(b[0], b[1], b[2], p.vol, T_wc, p.K, near, far, p.trunc, True)
    torch.cuda.synchronize()
    assert int(np.isfinite(b[0].MemcpyToHost()).sum()) > w * h // 10 and _images_equal(a, b)
    # a shift that is no whole brick is refused while spilling
    with pytest.raises(ValueError, match="whole bricks"):
        p.shift_volume((4, 0, 0))

    # SaveBricks -> a fresh volume of other contents -> LoadBricks: the cells bit for bit, and the box
    for src, fill, kind in ((p.vol, NAN, "f32"), (p.cvol, 0.5, "c32")):
        path = str(tmp_path / ("snapshot_%s.npz" % kind))
        n = SaveBricks(path, src, fill)
        with np.load(path) as z:
            assert sorted(z.files) == ["boxmax", "boxmin", "cells", "dims", "fill_bits", "ids", "kind"] and z["ids"].size == n > 0
            assert z["cells"].shape == (n, roo.brick_bytes(src)) and z["dims"].tolist() == [N, N, N] and str(z["kind"]) == kind
        fresh = roo.BoundedVolume(N, N, N, LO, HI, kind=kind)
        fresh.storage.copy_(torch.from_numpy(np.random.default_rng(2).integers(0, 256, fresh.storage.numel(), dtype=np.uint8)))
        assert LoadBricks(path, fresh) == n
        torch.cuda.synchronize()
        assert np.array_equal(_cells(fresh.storage.cpu().numpy(), fresh), _cells(src.storage.cpu().numpy(), src))
        assert np.array_equal(fresh.boxmin, src.boxmin) and np.array_equal(fresh.boxmax, src.boxmax)
        with pytest.raises(ValueError, match="LoadBricks"):
            LoadBricks(path, roo.BoundedVolume(N, N, 24, LO, HI, kind=kind))
        with pytest.raises(ValueError, match="LoadBricks"):
            LoadBricks(path, roo.BoundedVolume(N, N, N, LO, HI, kind="f16"))
