"""bricks.world_frame: the frame a volume's live bricks and its store's bricks share, in numpy alone, on the lattice whose positions are
exact in fp32 (tests/test_follow_cpu.py, tests/test_gpu_bricks.py): box (-1, -1, 2) - (0.9375, 0.9375, 3.9375), 32^3, voxel 1/16.  And
BrickStore.items(), which looks without taking."""
import numpy as np
import pytest

from kangaroo_amd import bricks

N = 32
LO, HI = np.array([-1.0, -1.0, 2.0], np.float32), np.array([0.9375, 0.9375, 3.9375], np.float32)
VOXEL = 1.0 / 16


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def shifted_box(origin):
    """the box of the 32^3 volume after shifts that sum to `origin` (exact on this lattice)"""
    o = np.asarray(origin, np.float64)
    return (LO + o * VOXEL).astype(np.float32), (HI + o * VOXEL).astype(np.float32)


def test_an_empty_store_gives_the_volumes_own_frame():
    live = np.array([[0, 0, 0], [3, 1, 2], [1, 0, 0]])
    for origin in ((0, 0, 0), (8, 0, -8), (3, -5, 1)):   # (without stored bricks the origin need not be whole bricks)
        bmin, bmax = shifted_box(origin)
        lo, dims, fmin, fmax, ids, order = bricks.world_frame(np.empty((0, 3)), live, origin, (N, N, N), bmin, bmax)
        assert tuple(lo) == tuple(origin) and tuple(dims) == (N, N, N)
        assert np.array_equal(bits(fmin), bits(bmin)) and np.array_equal(bits(fmax), bits(bmax))
        assert ids.dtype == np.uint32 and ids.tolist() == [0, 1, (2 * 4 + 1) * 4 + 3] and order.tolist() == [0, 2, 1]
    # dimensions that are no multiple of 8, and a box that is not on the lattice: the volume's own bits all the same
    bmin, bmax = np.array([-0.3, 0.1, 1.7], np.float32), np.array([0.77, 1.3, 2.9], np.float32)
    lo, dims, fmin, fmax, ids, _ = bricks.world_frame(np.empty((0, 3)), [[5, 3, 4]], (0, 0, 0), (44, 29, 35), bmin, bmax)
    assert tuple(dims) == (44, 29, 35) and ids.tolist() == [(4 * 4 + 3) * 6 + 5]
    assert np.array_equal(bits(fmin), bits(bmin)) and np.array_equal(bits(fmax), bits(bmax))


def test_keys_on_both_sides_of_the_world_origin_give_the_bounding_frame_and_ascending_ids():
    # the volume has moved by (8, 0, -8): it covers world cells x 8..40, y 0..32, z -8..24; what it left lies at x 0..8 and z 24..32
    origin = (8, 0, -8)
    bmin, bmax = shifted_box(origin)
    store = np.array([[0, 2, 3], [0, 0, -1], [2, 3, 3], [4, 1, 3]])          # world keys, negative z among them
    live = np.array([[3, 3, 3], [0, 0, 0], [1, 2, 0]])                        # the volume's own brick coordinates
    lo, dims, fmin, fmax, ids, order = bricks.world_frame(store, live, origin, (N, N, N), bmin, bmax)
    assert tuple(lo) == (0, 0, -8) and tuple(dims) == (40, 32, 40)
    # by hand: boxmin = vol.boxmin + (lo - origin) / 16, boxmax = vol.boxmin + (lo + dims - 1 - origin) / 16
    assert np.array_equal(bits(fmin), bits([-1.0, -1.0, 1.5])) and np.array_equal(bits(fmax), bits([1.4375, 0.9375, 3.9375]))
    # ids in the frame's 5 x 4 x 5 grid: world key - lo / 8 = key - (0, 0, -1); live keys first add origin / 8 = (1, 0, -1)
    rel = np.concatenate([live + [1, 0, 0], store + [0, 0, 1]])
    want = (rel[:, 2] * 4 + rel[:, 1]) * 5 + rel[:, 0]
    assert np.all(np.diff(ids.astype(np.int64)) > 0) and np.array_equal(ids, np.sort(want)) and np.array_equal(want[order], ids)
    # a store further out, on the negative side of every axis
    lo, dims, fmin, fmax, ids, order = bricks.world_frame([[-3, -1, -2]], live, (0, 0, 0), (N, N, N), LO, HI)
    assert tuple(lo) == (-24, -8, -16) and tuple(dims) == (56, 40, 48)
    assert np.array_equal(bits(fmin), bits([-2.5, -1.5, 1.0])) and np.array_equal(bits(fmax), bits(HI))
    assert ids[0] == 0 and order[0] == 3 and ids.tolist() == sorted(ids.tolist())
    # `cover`: a second store's keys widen the frame without joining the list
    lo2, dims2, _, _, ids2, _ = bricks.world_frame(np.empty((0, 3)), live, (0, 0, 0), (N, N, N), LO, HI, cover=[[-3, -1, -2]])
    assert tuple(lo2) == (-24, -8, -16) and tuple(dims2) == (56, 40, 48) and len(ids2) == 3 and set(ids2.tolist()) < set(ids.tolist())


def test_a_brick_both_stored_and_live_is_refused_and_so_is_a_store_beside_a_volume_off_the_brick_lattice():
    with pytest.raises(ValueError, match="both in the store and live"):
        bricks.world_frame([[1, 0, -1], [0, 0, 3]], [[0, 0, 0]], (8, 0, -8), (N, N, N), *shifted_box((8, 0, -8)))
    with pytest.raises(ValueError, match="whole bricks"):
        bricks.world_frame([[0, 0, 3]], [[0, 0, 0]], (4, 0, 0), (N, N, N), *shifted_box((4, 0, 0)))
    with pytest.raises(ValueError, match="whole bricks"):
        bricks.world_frame([[0, 0, 9]], [[0, 0, 0]], (0, 0, 0), (44, 32, 32), LO, HI)


def test_store_items_looks_without_taking():
    s = bricks.BrickStore("c32")
    keys, cells = s.items()
    assert keys.shape == (0, 3) and cells.shape == (0, 2048)
    rng = np.random.default_rng(1)
    put = rng.integers(0, 256, (3, 2048), dtype=np.uint8)
    s.put([[0, 0, 3], [-1, 2, 0], [5, 5, 5]], put)
    keys, cells = s.items()
    assert keys.tolist() == [[0, 0, 3], [-1, 2, 0], [5, 5, 5]] and np.array_equal(cells, put)
    cells[:] = 0   # (copies)
    assert len(s) == 3 and s.nbytes == 3 * 2048 and np.array_equal(s.items()[1], put)
    taken, _ = s.take([[5, 5, 5]])
    assert len(taken) == 1 and len(s) == 2 and s.items()[0].tolist() == [[0, 0, 3], [-1, 2, 0]]
