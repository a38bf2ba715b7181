"""The brick pool on the GPU (include/kfx_brick_pool.h, roo.BrickPool*, bricks.DeviceBrickStore, FramePipeline(follow=dict(spill="device"))).
The reference is numpy on the storage bytes and a replay of the pool's rules on the host.

  * a spill puts exactly the live bricks of BrickPack's reference into the pool, under key0 + (bx, by, bz), slot r holding the r-th of
    them, with the counters to match, the volume unchanged and nothing written behind the pool or the scratch;
  * a restore writes the cells of those bricks inside the view and no other byte of the storage, and leaves the pool empty;
  * a pool that is too small keeps the first bricks, counts the rest as dropped and stays intact;
  * spill, partial restore and re-spill over more than one scan block -- of the view and of the pool -- match the replay, twice to the
    byte; a restore and a discard that match nothing change no byte of the pool;
  * a pipeline that spills into pools computes what the pipeline with the host store computes, bit for bit, shift by shift."""
import numpy as np
import pytest

import kfx_testlib as T
from kfx_testlib import scenes
from test_gpu_bricks import CASES, _cells, _fill_bits, _numpy_pack, _scene, _brick_slices, _grid, _images_equal

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 0xA5
TAIL = 4096
KEY0 = (-3, 5, 1000)
POOL_CASES = [c for c in CASES if c[0] in ("f32-subview", "f16-subview", "colour-zero-fill")]


def r256(v):
    return (v + 255) // 256 * 256


class Pool:
    """a pool and a scratch with a guard region behind each, and the pool's parts read through the documented layout"""

    def __init__(self, roo, kind, capacity, view):
        import torch
        self.roo, self.kind, self.cap = roo, kind, capacity
        self.bb = 512 * {"f32": 8, "f16": 4, "c32": 4}[kind]
        self.need, self.sneed = roo.BrickPoolBytes(kind, capacity), roo.BrickPoolScratchBytes(view, capacity)
        assert self.need == 256 + r256(16 * capacity) + r256(4 * capacity) + self.bb * capacity and self.sneed > 0
        self.buf = torch.full((self.need + TAIL,), GUARD, dtype=torch.uint8, device="cuda")
        self.sbuf = torch.full((self.sneed + TAIL,), GUARD, dtype=torch.uint8, device="cuda")
        self.pool, self.scratch = self.buf[:self.need], self.sbuf[:self.sneed]
        roo.BrickPoolInit(self.pool, kind, capacity)

    def spill(self, view, fill, key0):
        self.roo.BrickPoolSpill(self.pool, self.cap, view, fill, key0, self.scratch)

    def restore(self, view, key0):
        self.roo.BrickPoolRestore(self.pool, self.cap, view, key0, self.scratch)

    def bytes(self):
        import torch
        torch.cuda.synchronize()
        return self.pool.cpu().numpy()

    def read(self):
        """(header dict, keys (cap, 4) int32, free (cap,) uint32, cells (cap, brick bytes))"""
        b, cap = self.bytes(), self.cap
        h = b[:32].view(np.uint64)
        rec = b[32:40].view(np.uint32)
        assert int(rec[0]) == self.roo.CELL_KIND[self.kind] and int(rec[1]) == cap
        f0 = 256 + r256(16 * cap)
        c0 = f0 + r256(4 * cap)
        hdr = dict(free_n=int(h[0]), spilled=int(h[1]), restored=int(h[2]), dropped=int(h[3]))
        return hdr, b[256:256 + 16 * cap].view(np.int32).reshape(cap, 4), b[f0:f0 + 4 * cap].view(np.uint32), b[c0:c0 + cap * self.bb].reshape(cap, self.bb)

    def as_map(self):
        _, keys, _, cells = self.read()
        return {tuple(int(v) for v in keys[s, :3]): cells[s].tobytes() for s in np.flatnonzero(keys[:, 3] == 1)}

    def guards_intact(self):
        return bool((self.buf[self.need:] == GUARD).all()) and bool((self.sbuf[self.sneed:] == GUARD).all())

    def check_partition(self):
        """the occupied slots and free[0 .. free_n) partition [0, capacity); every state is 0 or 1"""
        hdr, keys, free, _ = self.read()
        assert set(np.unique(keys[:, 3]).tolist()) <= {0, 1}
        occupied, stack = np.flatnonzero(keys[:, 3] == 1), free[:hdr["free_n"]].astype(np.int64)
        assert hdr["free_n"] + occupied.size == self.cap
        assert np.array_equal(np.sort(np.concatenate([occupied, stack])), np.arange(self.cap))


def _keys_of(tgt, ids, key0=KEY0):
    nbx, nby, _ = _grid(tgt)
    ids = np.asarray(ids, np.int64)
    return [(key0[0] + int(i % nbx), key0[1] + int(i // nbx % nby), key0[2] + int(i // (nbx * nby))) for i in ids]


def _spilled_scene(roo, case, capacity):
    """a case's scene spilled into a fresh pool of `capacity`: (vol, tgt, before, want ids, want cells (n, brick bytes) uint8, pool)"""
    _, kind, dims, pitch, view, fill = case
    vol, tgt, before, fill_bits, trap_ids = _scene(roo, case)
    want_ids, want_cells = _numpy_pack(_cells(before, tgt), fill_bits)
    assert set(trap_ids.values()) <= set(want_ids.tolist()) and 3 < want_ids.size <= 64
    pool = Pool(roo, kind, capacity, tgt)
    pool.spill(tgt, fill, KEY0)
    return vol, tgt, before, want_ids, want_cells.view(np.uint8).reshape(want_ids.size, -1), pool


def _expect_restored(before, other, tgt, ids):
    """`other` everywhere but the cells of the listed bricks inside the view, which are `before`'s"""
    expect = other.copy()
    for bid in ids:
        sl = _brick_slices(tgt, int(bid))
        _cells(expect, tgt)[sl] = _cells(before, tgt)[sl]
    return expect


@pytest.mark.parametrize("case", POOL_CASES, ids=[c[0] for c in POOL_CASES])
def test_gpu_spill_equals_pack(roo, case):
    cap = 64
    vol, tgt, before, want_ids, want_cells, pool = _spilled_scene(roo, case, cap)
    n = want_ids.size
    hdr, keys, free, cells = pool.read()
    print("%s: %d of %d bricks live; header %s" % (case[0], n, int(np.prod(_grid(tgt))), hdr))
    want_keys = _keys_of(tgt, want_ids)
    assert pool.as_map() == {k: want_cells[r].tobytes() for r, k in enumerate(want_keys)}
    # slot r holds the r-th id: a fresh pool hands out slot 0 first
    assert np.array_equal(keys[:n], np.array([k + (1,) for k in want_keys], np.int32)) and not keys[n:, 3].any()
    assert np.array_equal(cells[:n], want_cells)
    assert hdr == dict(free_n=cap - n, spilled=n, restored=0, dropped=0)
    assert np.array_equal(free, cap - 1 - np.arange(cap, dtype=np.uint32))   # a spill pops: the stack's entries stay
    pool.check_partition()
    assert np.array_equal(vol.storage.cpu().numpy(), before)   # spilling reads
    assert pool.guards_intact(), "written behind the pool or the scratch"
    assert roo.BrickPoolStats(pool.pool, tgt.kind, cap) == dict(occupied=n, spilled=n, restored=0, dropped=0)
    # the gather of any slots, on the device: the payload in the order asked for, a slot beyond the capacity skipped
    import torch
    order = np.concatenate([np.arange(n)[::-1], [cap + 5]])
    got = roo.BrickPoolGather(pool.pool, tgt.kind, cap, order)
    torch.cuda.synchronize()
    assert np.array_equal(got[:n].cpu().numpy(), want_cells[::-1])
    slots, k = roo.BrickPoolKeys(pool.pool, cap)
    assert np.array_equal(slots, np.arange(n)) and [tuple(v) for v in k.tolist()] == want_keys


@pytest.mark.parametrize("case", POOL_CASES, ids=[c[0] for c in POOL_CASES])
def test_gpu_restore_writes_exactly_the_view(roo, case):
    import torch
    cap = 64
    vol, tgt, before, want_ids, want_cells, pool = _spilled_scene(roo, case, cap)
    n = want_ids.size
    other = np.random.default_rng(23).integers(0, 256, before.size, dtype=np.uint8)
    vol.storage.copy_(torch.from_numpy(other))
    pool.restore(tgt, KEY0)
    torch.cuda.synchronize()
    after = vol.storage.cpu().numpy()
    bad = np.flatnonzero(after != _expect_restored(before, other, tgt, want_ids))
    assert bad.size == 0, (case[0], "%d bytes differ, first at %s" % (bad.size, bad[:8].tolist()))
    hdr, keys, free, _ = pool.read()
    assert hdr == dict(free_n=cap, spilled=n, restored=n, dropped=0) and not keys[:, 3].any() and pool.as_map() == {}
    # the i-th slot taken (ascending) was pushed to free[free_n + i]
    assert np.array_equal(free[:cap - n], cap - 1 - np.arange(cap - n, dtype=np.uint32)) and np.array_equal(free[cap - n:], np.arange(n, dtype=np.uint32))
    pool.check_partition()
    assert pool.guards_intact()


@pytest.mark.parametrize("case", POOL_CASES, ids=[c[0] for c in POOL_CASES])
def test_gpu_a_full_pool_keeps_the_first_bricks_and_counts_the_rest(roo, case):
    import torch
    cap = 3
    vol, tgt, before, want_ids, want_cells, pool = _spilled_scene(roo, case, cap)
    n = want_ids.size
    hdr, keys, free, cells = pool.read()
    want_keys = _keys_of(tgt, want_ids[:3])
    assert pool.as_map() == {k: want_cells[r].tobytes() for r, k in enumerate(want_keys)}
    assert np.array_equal(keys, np.array([k + (1,) for k in want_keys], np.int32)) and np.array_equal(cells, want_cells[:3])
    assert hdr == dict(free_n=0, spilled=3, restored=0, dropped=n - 3)
    assert pool.guards_intact() and np.array_equal(vol.storage.cpu().numpy(), before)
    other = np.random.default_rng(29).integers(0, 256, before.size, dtype=np.uint8)
    vol.storage.copy_(torch.from_numpy(other))
    pool.restore(tgt, KEY0)
    torch.cuda.synchronize()
    assert np.array_equal(vol.storage.cpu().numpy(), _expect_restored(before, other, tgt, want_ids[:3]))
    hdr, keys, free, _ = pool.read()
    assert hdr == dict(free_n=3, spilled=3, restored=3, dropped=n - 3) and not keys[:, 3].any()
    pool.check_partition()
    assert pool.guards_intact()


class Replay:
    """the pool's rules on the host, in numpy: keys, free stack, counters and payload by slot"""

    def __init__(self, cap, bb):
        self.cap, self.free_n, self.spilled, self.restored, self.dropped = cap, cap, 0, 0, 0
        self.state, self.key = np.zeros(cap, bool), np.zeros((cap, 3), np.int64)
        self.free, self.cells = cap - 1 - np.arange(cap), np.zeros((cap, bb), np.uint8)

    def take(self, key0, nb, restore):
        rel = self.key - np.asarray(key0)
        slots = np.flatnonzero(self.state & np.all((rel >= 0) & (rel < np.asarray(nb)), axis=1))
        self.free[self.free_n:self.free_n + slots.size] = slots
        self.state[slots] = False
        self.free_n += slots.size
        self.restored += slots.size if restore else 0
        return slots

    def spill(self, key0, nb, live_ids, bricks):
        self.take(key0, nb, False)
        m = min(len(live_ids), self.free_n)
        for r in range(m):
            slot, i = self.free[self.free_n - 1 - r], int(live_ids[r])
            self.state[slot], self.cells[slot] = True, bricks[r]
            self.key[slot] = (key0[0] + i % nb[0], key0[1] + i // nb[0] % nb[1], key0[2] + i // (nb[0] * nb[1]))
        self.free_n -= m
        self.spilled += m
        self.dropped += len(live_ids) - m

    def check(self, pool):
        hdr, keys, free, cells = pool.read()
        assert hdr == dict(free_n=self.free_n, spilled=self.spilled, restored=self.restored, dropped=self.dropped)
        assert np.array_equal(keys[:, 3] == 1, self.state)
        occ = np.flatnonzero(self.state)
        assert np.array_equal(keys[occ, :3], self.key[occ]) and np.array_equal(cells[occ], self.cells[occ])
        assert np.array_equal(free[:self.free_n], self.free[:self.free_n])
        pool.check_partition()
        assert pool.guards_intact()


def _column_sequence(roo):
    """An f16 column of 600 bricks, all live, and a pool of 700 slots: three scan blocks on both sides.  Spill everything, restore the
    view of bricks 100..399, change one cell of brick 250, spill that view again.  Returns the pool's bytes at the end."""
    import torch
    NB, cap, key0 = 600, 700, (7, -2, -300)
    vol = roo.BoundedVolume(8, 8, 8 * NB, kind="f16", pitch=32)
    rng = np.random.default_rng(41)
    before = rng.integers(0, 256, vol.storage.numel(), dtype=np.uint8)
    vol.storage.copy_(torch.from_numpy(before))
    fill_bits = _fill_bits(roo, "f16", NAN)
    ids, bricks = _numpy_pack(_cells(before, vol), fill_bits)
    assert ids.size == NB
    bricks = bricks.view(np.uint8).reshape(NB, -1)
    pool, rep = Pool(roo, "f16", cap, vol), Replay(cap, 2048)
    pool.spill(vol, NAN, key0)
    rep.spill(key0, (1, 1, NB), ids, bricks)
    rep.check(pool)
    assert np.array_equal(np.flatnonzero(rep.state), np.arange(NB))
    # a restore and a discard whose key range matches nothing: no byte of the pool changes
    was = pool.bytes().copy()
    pool.restore(vol, (7, -1, -300))
    roo.BrickPoolDiscard(pool.pool, "f16", cap, (3, 2, 50), (8, -2, -300), pool.scratch)
    roo.BrickPoolDiscard(pool.pool, "f16", cap, (1, 1, 100), (7, -2, 300), pool.scratch)
    assert np.array_equal(pool.bytes(), was) and np.array_equal(vol.storage.cpu().numpy(), before)
    # the view of bricks 100 .. 399 comes back into a volume of other bytes
    part, pkey = vol.SubVolume((0, 0, 800), (8, 8, 8 * 300)), (7, -2, -200)
    other = rng.integers(0, 256, before.size, dtype=np.uint8)
    vol.storage.copy_(torch.from_numpy(other))
    pool.restore(part, pkey)
    taken = rep.take(pkey, (1, 1, 300), True)
    assert np.array_equal(taken, np.arange(100, 400))
    rep.check(pool)
    expect = other.copy()
    _cells(expect, part)[...] = _cells(before, part)
    assert np.array_equal(vol.storage.cpu().numpy(), expect)
    # one cell of brick 250 changes; the view is spilled again: its bricks replace nothing (they left), and take the slots on top
    now = expect.copy()
    _cells(now, vol)[250 * 8 + 3, 4, 5] ^= 0x00010000
    vol.storage.copy_(torch.from_numpy(now))
    pids, pbricks = _numpy_pack(_cells(now, part), fill_bits)
    assert pids.size == 300
    pool.spill(part, NAN, pkey)
    rep.spill(pkey, (1, 1, 300), pids, pbricks.view(np.uint8).reshape(300, -1))
    rep.check(pool)
    m = pool.as_map()
    assert len(m) == NB and m[(7, -2, -300 + 250)] == pbricks[150].tobytes() != bricks[250].tobytes()
    assert m[(7, -2, -300 + 249)] == bricks[249].tobytes() and m[(7, -2, -300)] == bricks[0].tobytes()
    # spilled again without having left: the discard step replaces the old bytes, and nothing is counted as dropped
    _cells(now, vol)[250 * 8 + 3, 4, 5] ^= 0x00020000
    vol.storage.copy_(torch.from_numpy(now))
    pids, pbricks = _numpy_pack(_cells(now, part), fill_bits)
    pool.spill(part, NAN, pkey)
    rep.spill(pkey, (1, 1, 300), pids, pbricks.view(np.uint8).reshape(300, -1))
    rep.check(pool)
    m = pool.as_map()
    assert len(m) == NB and m[(7, -2, -50)] == pbricks[150].tobytes() and rep.dropped == 0 and rep.spilled == NB + 600
    return pool.bytes().copy()


def test_gpu_more_than_one_scan_block_on_both_sides_and_twice_the_same_bytes(roo):
    first = _column_sequence(roo)
    second = _column_sequence(roo)
    assert np.array_equal(first, second), "the pool's bytes are no function of the sequence of calls"


def test_gpu_a_pipeline_with_pools_computes_what_the_host_store_computes(roo):
    """32^3, tracked, in colour (test_gpu_bricks' spilling volume): p keeps what leaves on the host, r in two pools.  (8, 0, -8), then
    (0, 8, 0), then back in the other order."""
    import torch
    from kangaroo_amd import _lib
    from kangaroo_amd.bricks import DeviceBrickStore
    from kangaroo_amd.pipeline import FramePipeline, SlabPipeline
    assert hasattr(_lib.load(), "kfx_brick_pool_spill")
    N, w, h = 32, 80, 60
    lo, hi = (-1.0, -1.0, 2.0), (0.9375, 0.9375, 3.9375)
    p = FramePipeline(roo, (N, N, N), lo, hi, w, h, track=True, color=True, follow=dict(quantum=8, spill=True))
    r = FramePipeline(roo, (N, N, N), lo, hi, w, h, track=True, color=True, follow=dict(quantum=8, spill="device"))
    small = FramePipeline(roo, (N, N, N), lo, hi, w, h, track=True, color=True, follow=dict(quantum=8, spill="device", pool_bricks=2))
    assert r.spill == "device" and isinstance(r.store, DeviceBrickStore) and isinstance(r.cstore, DeviceBrickStore)
    assert r.store.capacity == 64 == r.cstore.capacity and small.store.capacity == 2 and r.store.kind == "f32" and r.cstore.brick_bytes == 2048
    for i in range(3):
        T_wc = scenes.orbit_pose(i, 8)
        raw = T.upload_image(roo, scenes.render_depth("room", w, h, T_wc, p.K))
        rgb = roo.Image(w, h, "u8x3").MemcpyFromHost(scenes.render_rgb("room", w, h, T_wc, p.Kimg))
        for pipe in (p, r, small):
            pipe.step(T_wc, raw, rgb)
    torch.cuda.synchronize()
    assert p.shifts == [] and r.shifts == []
    host = lambda pipe: (pipe.vol.storage.cpu().numpy().copy(), pipe.cvol.storage.cpu().numpy().copy())
    sdf0, col0 = host(p)
    T_back = scenes.orbit_pose(0, 8)   # looks at where the volume was

    def same(what):
        torch.cuda.synchronize()
        (a, ac), (b, bc) = host(p), host(r)
        assert np.array_equal(a, b), "%s: the SDF volumes differ" % what
        assert np.array_equal(ac, bc), "%s: the colour volumes differ" % what
        for s, t in ((p.store, r.store), (p.cstore, r.cstore)):
            ks, kt = set(map(tuple, s.items()[0].tolist())), set(map(tuple, t.items()[0].tolist()))
            assert len(t) == len(s) == len(ks) and ks == kt, what
            assert t.nbytes == s.nbytes
            hs, ht = dict(zip(map(tuple, s.items()[0].tolist()), s.items()[1])), dict(zip(map(tuple, t.items()[0].tolist()), t.items()[1]))
            assert all(np.array_equal(hs[k], ht[k]) for k in ks), what

    away = 0
    for shift in ((8, 0, -8), (0, 8, 0), (0, -8, 0), (-8, 0, 8)):
        for pipe in (p, r, small):
            pipe.shift_volume(shift)
        same("after %s" % (shift,))
        assert r.origin == p.origin and r.restored == p.restored
        if len(p.store):
            away += 1
            assert len(r.store) > 0 and len(r.cstore) > 0
            for color in (False, True):
                assert _images_equal(p.RaycastWorld(T_back, color=color), r.RaycastWorld(T_back, color=color)), shift
            mp, mr = p.ExtractWorldMesh(with_index=True), r.ExtractWorldMesh(with_index=True)
            torch.cuda.synchronize()
            assert len(mp[0]) > 100
            for a, b in zip(mp, mr):
                raw_bytes = lambda x: (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).tobytes()
                assert (a is None and b is None) or raw_bytes(a) == raw_bytes(b), shift
    assert away == 3 and p.restored > 0
    got = host(r)
    assert np.array_equal(got[0], sdf0) and np.array_equal(got[1], col0), "the volumes did not come back"
    assert len(r.store) == 0 and len(r.cstore) == 0 and r.store.nbytes == 0 and r.store.dropped == 0 and r.cstore.dropped == 0
    # the summary was rebuilt after the restores: the table march renders the plain march's bits
    T_wc = scenes.orbit_pose(2, 8)
    a, b = (roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h)), (roo.Image(w, h), roo.Image(w, h, "f32x4"), roo.Image(w, h))
    roo.RaycastSdf(a[0], a[1], a[2], r.vol, T_wc, r.K, r.near, r.far, r.trunc, True, summary=r.summary)
    roo.RaycastSdf(b[0], b[1], b[2], r.vol, T_wc, r.K, r.near, r.far, r.trunc, True)
    torch.cuda.synchronize()
    assert int(np.isfinite(b[0].MemcpyToHost()).sum()) > w * h // 10 and _images_equal(a, b)
    # a pool of two bricks was too small: it says so, and the pipeline went on
    assert small.store.dropped > 0 and small.origin == (0, 0, 0) and len(small.store) == 0
    small.step(T_wc, raw, rgb)
    torch.cuda.synchronize()
    # reset() clears the pools
    r.shift_volume((8, 0, -8))
    assert len(r.store) > 0
    r.reset()
    assert len(r.store) == 0 and len(r.cstore) == 0 and r.store.stats() == dict(occupied=0, spilled=0, restored=0, dropped=0)
    with pytest.raises(ValueError, match="whole bricks"):
        r.shift_volume((4, 0, 0))
    with pytest.raises(ValueError, match="spill"):
        FramePipeline(roo, (N, N, N), lo, hi, w, h, follow=dict(quantum=8, spill="host"))
    with pytest.raises(ValueError, match="pool_bricks"):
        FramePipeline(roo, (N, N, N), lo, hi, w, h, follow=dict(quantum=8, spill=True, pool_bricks=4))
    with pytest.raises(ValueError, match="spill='device'"):
        SlabPipeline(roo, None, (N, N, N), lo, hi, w, h, follow=dict(spill="device"))
