"""The host side of the spilling volume (kangaroo_amd/bricks.py): which boxes of a shift leave and enter, against a brute-force
mask; the world keys of their bricks; the store; and what FramePipeline(follow=dict(spill=True)) refuses.  Pure numpy."""
import itertools

import numpy as np
import pytest

from kangaroo_amd import bricks
from kangaroo_amd.bricks import BrickStore, box_brick_ids, entering_boxes, leaving_boxes, world_keys
from kangaroo_amd.pipeline import FramePipeline

DIMS = (40, 24, 16)
STEPS = (-16, -8, 0, 8, 16, 24, 40)
SHIFTS = list(itertools.product(STEPS, STEPS, STEPS))


def _masks(dims, shift):
    """(leaving, entering) as (d, h, w) masks: old cells whose destination x - s is outside, new cells whose source x + s is"""
    axes = [np.arange(n) for n in dims]
    dst_in = [(a - s >= 0) & (a - s < n) for a, s, n in zip(axes, shift, dims)]
    src_in = [(a + s >= 0) & (a + s < n) for a, s, n in zip(axes, shift, dims)]
    cube = lambda m: m[2][:, None, None] & m[1][None, :, None] & m[0][None, None, :]
    return ~cube(dst_in), ~cube(src_in)


def _cover(dims, boxes):
    count = np.zeros(dims[::-1], np.int32)
    for (x, y, z), (w, h, d) in boxes:
        assert w > 0 and h > 0 and d > 0 and x >= 0 and y >= 0 and z >= 0 and x + w <= dims[0] and y + h <= dims[1] and z + d <= dims[2]
        count[z:z + d, y:y + h, x:x + w] += 1
    return count


@pytest.mark.parametrize("planner, which", [(leaving_boxes, 0), (entering_boxes, 1)])
def test_boxes_are_disjoint_at_most_three_and_cover_the_mask_exactly(planner, which):
    assert len(SHIFTS) == 343
    for shift in SHIFTS:
        boxes = planner(DIMS, shift)
        assert len(boxes) <= 3, (shift, boxes)
        count = _cover(DIMS, boxes)
        assert count.max(initial=0) <= 1, (shift, boxes)                       # disjoint
        assert np.array_equal(count == 1, _masks(DIMS, shift)[which]), (shift, boxes)
    assert planner(DIMS, (0, 0, 0)) == []
    for shift in ((40, 0, 0), (0, -24, 0), (8, 8, 16), (48, -8, 0)):           # at or beyond the extent: everything goes, in one box
        assert planner(DIMS, shift) == [((0, 0, 0), DIMS)]


def test_the_retained_cells_are_the_issues_interval():
    # new(x) = old(x + s): the old cells kept are [max(0, s), min(dim, dim + s)) per axis
    for shift in SHIFTS:
        leaving, _ = _masks(DIMS, shift)
        kept = np.zeros(DIMS[::-1], bool)
        lo = [max(0, s) for s in shift]
        hi = [min(n, n + s) for s, n in zip(shift, DIMS)]
        if all(a < b for a, b in zip(lo, hi)):
            kept[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = True
        assert np.array_equal(kept, ~leaving), shift


def test_world_keys_follow_the_boxs_brick_ids_and_invert():
    keys = world_keys((16, -8, 0), (8, 0, 8), (16, 24, 8))
    assert keys.shape == (2 * 3 * 1, 3) and keys.dtype == np.int64
    assert keys.tolist() == [[3, -1, 1], [4, -1, 1], [3, 0, 1], [4, 0, 1], [3, 1, 1], [4, 1, 1]]   # x fastest, then y, then z
    assert box_brick_ids((16, -8, 0), (8, 0, 8), (16, 24, 8), keys).tolist() == list(range(6))
    assert box_brick_ids((16, -8, 0), (8, 0, 8), (16, 24, 8), keys[[1, 4]]).tolist() == [1, 4]
    for bad in (((4, 0, 0), (0, 0, 0), (8, 8, 8)), ((0, 0, 0), (0, 2, 0), (8, 8, 8)), ((0, 0, 0), (0, 0, 0), (8, 8, 12))):
        with pytest.raises(ValueError, match="whole bricks"):
            world_keys(*bad)


def _as_set(keys):
    return set(map(tuple, np.asarray(keys).reshape(-1, 3).tolist()))


def test_keys_there_and_back_cancel():
    """What leaves under a shift s enters again under -s: the same world keys, so a store filled by the one is emptied by the other."""
    for origin in ((0, 0, 0), (-24, 8, 160)):
        for shift in SHIFTS:
            gone = set()
            for start, size in leaving_boxes(DIMS, shift):
                keys = _as_set(world_keys(origin, start, size))
                assert not keys & gone
                gone |= keys
            moved = tuple(o + s for o, s in zip(origin, shift))
            back_origin = tuple(o - s for o, s in zip(moved, shift))
            assert back_origin == origin
            back = set()
            for start, size in entering_boxes(DIMS, tuple(-s for s in shift)):
                back |= _as_set(world_keys(back_origin, start, size))
            assert back == gone, (origin, shift)
            # and what the shift itself exposes are other bricks, unless nothing is retained
            if all(abs(s) < n for s, n in zip(shift, DIMS)) and any(shift):
                exposed = set()
                for start, size in entering_boxes(DIMS, shift):
                    exposed |= _as_set(world_keys(moved, start, size))
                assert not exposed & gone, (origin, shift)


@pytest.mark.parametrize("kind, nbytes", [("f32", 4096), ("f16", 2048), ("c32", 2048)])
def test_brick_store_round_trip(kind, nbytes):
    rng = np.random.default_rng(3)
    store = BrickStore(kind)
    assert len(store) == 0 and store.nbytes == 0 and store.brick_bytes == nbytes
    keys = np.array([[0, 0, 0], [-1, 2, 7], [5, 5, 5], [1 << 40, 0, -3]], np.int64)
    cells = rng.integers(0, 256, (4, nbytes), dtype=np.uint8)
    store.put(keys, cells)
    cells_before = cells.copy()
    cells[:] = 0                                                    # the store keeps its own copy
    assert len(store) == 4 and store.nbytes == 4 * nbytes
    found, got = store.take(np.array([[9, 9, 9], [5, 5, 5], [0, 0, 0], [7, 7, 7]]))
    assert found.tolist() == [[5, 5, 5], [0, 0, 0]] and np.array_equal(got, cells_before[[2, 0]]) and got.dtype == np.uint8
    assert len(store) == 2 and store.nbytes == 2 * nbytes
    found, got = store.take(np.array([[5, 5, 5], [0, 0, 0]]))      # taken means gone
    assert found.shape == (0, 3) and got.shape == (0, nbytes)
    store.put(keys[1:2], cells_before[3:4])                          # a key already present is replaced
    found, got = store.take(keys)
    assert found.tolist() == keys[[1, 3]].tolist() and np.array_equal(got, cells_before[[3, 3]])
    assert len(store) == 0 and store.nbytes == 0
    store.put(keys, cells_before)
    store.clear()
    assert len(store) == 0


class _Ops:
    """an operator set that has the shift and the bricks, and nothing the constructor may reach before it refuses"""
    VolumeShift = BrickPack = BrickUnpack = staticmethod(lambda *a, **k: None)


LO, HI = (-1.0, -1.0, 2.0), (1.0, 1.0, 4.0)


def test_spill_is_refused_unless_shifts_and_dims_are_whole_bricks():
    with pytest.raises(ValueError, match="spill=True.*multiples of 8"):
        FramePipeline(_Ops(), (32, 32, 32), LO, HI, 80, 60, follow=dict(quantum=4, spill=True))
    with pytest.raises(ValueError, match="spill=True.*multiples of 8"):
        FramePipeline(_Ops(), (40, 24, 12), LO, HI, 80, 60, follow=dict(quantum=8, spill=True))
    with pytest.raises(ValueError, match="spill=True.*multiples of 8"):
        FramePipeline(_Ops(), (40, 24, 12), LO, HI, 80, 60, follow=dict(spill=True))
    with pytest.raises(ValueError, match="takes focus, quantum, slack and spill"):
        FramePipeline(_Ops(), (32, 32, 32), LO, HI, 80, 60, follow=dict(quantum=8, spil=True))

    class NoBricks:
        VolumeShift = staticmethod(lambda *a, **k: None)
    with pytest.raises(ValueError, match="spill=True.*BrickPack"):
        FramePipeline(NoBricks(), (32, 32, 32), LO, HI, 80, 60, follow=dict(quantum=8, spill=True))
    assert bricks.BRICK == 8
