"""Sparse brick snapshots (include/kfx_bricks.h underneath): where the bricks a moving volume loses are kept -- on the host
(BrickStore) or in a brick pool on the device (DeviceBrickStore, include/kfx_brick_pool.h) -- which boxes of a shift leave and enter, and
a whole volume as one file.

A brick is 8 x 8 x 8 cells.  A volume that follows the camera in steps of whole bricks keeps its cells on one world lattice: with
`origin` the running sum of its shifts (new(x) = old(x + s), so the view's cell 0 is world cell `origin`), the brick at view cell
(8 i, 8 j, 8 k) has the world key (origin / 8 + (i, j, k)).  world_frame puts a volume's live bricks and its store's on one frame,
the input of the brick mesh (mesh.ExtractBrickMesh).  Pure numpy up to world_bricks and SaveBricks / LoadBricks, which call the operators.
"""
import numpy as np

BRICK = 8


def _retained(dim, s):
    """[lo, hi) of the old cells of one axis a shift by s keeps: those whose destination x - s lies inside"""
    return max(0, s), min(dim, dim + s)


def leaving_boxes(dims, shift):
    """The cells a shift discards (those whose destination is outside the view), in the coordinates before the shift: up to three
    disjoint (start, size) boxes that cover them exactly.  The retained cells are a box, [max(0, s), min(dim, dim + s)) per axis;
    what is left of the view is peeled off axis by axis: the z-planes outside it, then the y-rows outside it within its z-range,
    then the x-cells outside it within its z- and y-range.  A shift has one sign per axis, so each peel is one box."""
    dims = [int(v) for v in dims]
    keep = [_retained(d, int(s)) for d, s in zip(dims, shift)]
    if any(lo >= hi for lo, hi in keep):
        return [((0, 0, 0), tuple(dims))]
    boxes = []
    lo, hi = [0, 0, 0], list(dims)   # the part of the view not yet peeled
    for axis in (2, 1, 0):
        klo, khi = keep[axis]
        for a, b in ((0, klo), (khi, dims[axis])):
            if a < b:
                start, size = list(lo), [hi[i] - lo[i] for i in range(3)]
                start[axis], size[axis] = a, b - a
                boxes.append((tuple(start), tuple(size)))
        lo[axis], hi[axis] = klo, khi
    return boxes


def entering_boxes(dims, shift):
    """The cells a shift fills (those whose source is outside the view), in the coordinates after the shift: the cells the
    opposite shift would discard."""
    return leaving_boxes(dims, tuple(-int(s) for s in shift))


def world_keys(origin_cells, start, size):
    """The world brick keys (n, 3) int64 = (bx, by, bz) of the bricks of the box (start, size) of a view whose cell 0 is world cell
    origin_cells, in the order of the box's own brick ids ((bz * nby + by) * nbx + bx).  Everything a multiple of 8."""
    o = np.asarray(origin_cells, np.int64) + np.asarray(start, np.int64)
    size = np.asarray(size, np.int64)
    if np.any(o % BRICK) or np.any(size % BRICK):
        raise ValueError("world_keys: origin %s + start %s and size %s must be whole bricks" % (tuple(origin_cells), tuple(start), tuple(size)))
    nb = size // BRICK
    bz, by, bx = np.meshgrid(np.arange(nb[2]), np.arange(nb[1]), np.arange(nb[0]), indexing="ij")
    return np.stack([bx.reshape(-1), by.reshape(-1), bz.reshape(-1)], 1).astype(np.int64) + o // BRICK


def box_brick_ids(origin_cells, start, size, keys):
    """the brick ids, within the box (start, size), of world keys that lie in it: the inverse of world_keys"""
    rel = np.asarray(keys, np.int64).reshape(-1, 3) - (np.asarray(origin_cells, np.int64) + np.asarray(start, np.int64)) // BRICK
    nb = np.asarray(size, np.int64) // BRICK
    return (rel[:, 2] * nb[1] + rel[:, 1]) * nb[0] + rel[:, 0]


class BrickStore:
    """Host memory for the bricks of one volume that are outside its box: world brick key (bx, by, bz) -> the brick's bytes
    (512 cells, x fastest).  No limit and no eviction.  spill() / restore() / all_items() are DeviceBrickStore's calls (ops: the
    operator set they pack and unpack with, default kangaroo_amd.roo); the rest is plain host memory."""

    def __init__(self, kind="f32", ops=None):
        self.kind, self.ops = kind, ops
        self.brick_bytes = BRICK ** 3 * {"f32": 8, "f16": 4, "c32": 4}[kind]
        self._bricks = {}

    def __len__(self):
        return len(self._bricks)

    @property
    def nbytes(self):
        return len(self._bricks) * self.brick_bytes

    def clear(self):
        self._bricks.clear()

    def put(self, keys, cells):
        """keys (n, 3) integers, cells n bricks of bytes; a key already present is replaced"""
        keys = np.asarray(keys, np.int64).reshape(-1, 3)
        cells = np.ascontiguousarray(cells).view(np.uint8).reshape(len(keys), self.brick_bytes)
        for k, c in zip(keys.tolist(), cells):
            self._bricks[tuple(k)] = c.copy()

    def keys(self):
        """every key (m, 3) int64"""
        return np.asarray(list(self._bricks.keys()), np.int64).reshape(-1, 3)

    def items(self):
        """(every key (m, 3) int64, their cells (m, brick bytes) uint8), copies; the store keeps them"""
        if not self._bricks:
            return np.empty((0, 3), np.int64), np.empty((0, self.brick_bytes), np.uint8)
        return np.asarray(list(self._bricks.keys()), np.int64).reshape(-1, 3), np.stack(list(self._bricks.values()))

    def take(self, keys):
        """(found keys (m, 3) int64, their cells (m, brick bytes) uint8), in the order of `keys`; what is found leaves the store"""
        keys = np.asarray(keys, np.int64).reshape(-1, 3)
        found, cells = [], []
        for k in keys.tolist():
            c = self._bricks.pop(tuple(k), None)
            if c is not None:
                found.append(k)
                cells.append(c)
        if not found:
            return np.empty((0, 3), np.int64), np.empty((0, self.brick_bytes), np.uint8)
        return np.asarray(found, np.int64), np.stack(cells)

    def _ops(self):
        if self.ops is None:
            from . import roo
            self.ops = roo
        return self.ops

    def spill(self, view, fill, key0):
        """the live bricks of `view` (ops.BrickPack) go to the host under the keys key0 + (bx, by, bz); a key already present is replaced"""
        ids, cells = self._ops().BrickPack(view, fill)
        if ids.numel():
            size = (view.w, view.h, view.d)
            self.put(world_keys(np.asarray(key0, np.int64) * BRICK, (0, 0, 0), size)[ids.cpu().numpy()], cells.cpu().numpy())

    def restore(self, view, key0):
        """the bricks the store holds of the key range of `view` go back into it (ops.BrickUnpack) and leave the store; returns how
        many.  An empty store has nothing to look up."""
        if not len(self):
            return 0
        origin, size = np.asarray(key0, np.int64) * BRICK, (view.w, view.h, view.d)
        keys, cells = self.take(world_keys(origin, (0, 0, 0), size))
        if len(keys):
            self._ops().BrickUnpack(view, box_brick_ids(origin, (0, 0, 0), size, keys), cells)
        return len(keys)

    def all_items(self):
        """what bricks.world_bricks asks either store for: (keys (m, 3) int64, cells (m, brick bytes) uint8), the cells where the
        store keeps them -- here on the host"""
        return self.items()


class DeviceBrickStore:
    """Device memory for the bricks of one volume that are outside its box: a brick pool (include/kfx_brick_pool.h) of `capacity`
    bricks in one uint8 tensor, and the scratch of its calls.  spill() and restore() enqueue launches on torch's current stream and
    never touch the host.  A spill that finds the pool full DROPS the bricks that do not fit -- they are lost, as every brick is
    without a store -- and counts them: `dropped` > 0 says that the pool was too small.  No eviction.
    What it shares with BrickStore: kind, brick_bytes, len() and nbytes (blocking: they read the pool's counters), clear(), items(),
    all_items(), spill() and restore()."""

    def __init__(self, kind, capacity, ops=None, device="cuda"):
        import torch
        if ops is None:
            from . import roo as ops
        self.ops, self.kind, self.capacity = ops, kind, int(capacity)
        self.brick_bytes = BRICK ** 3 * {"f32": 8, "f16": 4, "c32": 4}[kind]
        need = ops.BrickPoolBytes(kind, self.capacity)
        if not need:
            raise ValueError("DeviceBrickStore: a pool holds 1 .. 2^31 - 1 bricks, not %d" % self.capacity)
        self.pool = torch.empty(need, dtype=torch.uint8, device=device)
        self._scratch = None
        self.clear()

    def _scratch_for(self, view):
        import torch
        need = self.ops.BrickPoolScratchBytes(view, self.capacity)
        if self._scratch is None or self._scratch.numel() < need:   # (torch's memory: its reuse is ordered on torch's current stream)
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.pool.device)
        return self._scratch

    def clear(self):
        self.ops.BrickPoolInit(self.pool, self.kind, self.capacity)

    def stats(self):
        """dict(occupied=, spilled=, restored=, dropped=) -- blocking"""
        return self.ops.BrickPoolStats(self.pool, self.kind, self.capacity)

    def __len__(self):
        return self.stats()["occupied"]

    @property
    def nbytes(self):
        return len(self) * self.brick_bytes

    @property
    def dropped(self):
        return self.stats()["dropped"]

    @property
    def restored(self):
        return self.stats()["restored"]

    def spill(self, view, fill, key0):
        """the live bricks of `view` go into the pool under the keys key0 + (bx, by, bz); what the pool held of that range is replaced"""
        self.ops.BrickPoolSpill(self.pool, self.capacity, view, fill, key0, self._scratch_for(view))

    def restore(self, view, key0):
        """the bricks the pool holds of the key range of `view` go back into it and leave the pool; returns None: how many is not
        known on the host"""
        self.ops.BrickPoolRestore(self.pool, self.capacity, view, key0, self._scratch_for(view))

    def keys(self):
        """every key (m, 3) int64 -- blocking: a plain copy of the pool's keys block"""
        return self.ops.BrickPoolKeys(self.pool, self.capacity)[1]

    def device_items(self):
        """(every key (m, 3) int64 on the host, their cells (m, brick bytes) uint8 on the device, gathered); the store keeps them.
        Blocking: the keys block is copied to the host; the payload stays on the device."""
        slots, keys = self.ops.BrickPoolKeys(self.pool, self.capacity)
        return keys, self.ops.BrickPoolGather(self.pool, self.kind, self.capacity, slots)

    def all_items(self):
        """what bricks.world_bricks asks either store for: device_items(), the cells where the store keeps them -- on the device"""
        return self.device_items()

    def items(self):
        """(every key (m, 3) int64, their cells (m, brick bytes) uint8) on the host, copies: for checkpoints and tests"""
        keys, cells = self.device_items()
        return keys, cells.cpu().numpy()


def world_frame(store_keys, live_keys, origin, vol_dims, vol_boxmin, vol_boxmax, cover=None):
    """The frame of a volume's live bricks and its store's together (numpy only): the bounding box, in whole bricks, of the volume's
    own box (cells [origin, origin + vol_dims) of the world lattice), the store's keys and the keys of `cover` (a second store whose
    bricks are to share the frame: a colour store beside the SDF store).

    Returns (lo, dims, boxmin, boxmax, ids, order): lo the frame's first world cell, a multiple of 8; dims its cells; its box in float32
    from float64 arithmetic on the volume's lattice -- voxel = (vol_boxmax - vol_boxmin) / (vol_dims - 1), boxmin = vol_boxmin +
    (lo - origin) * voxel, boxmax = vol_boxmin + (lo + dims - 1 - origin) * voxel; ids (uint32, strictly ascending) the brick ids in
    the frame's grid of all bricks, and order the rows of concatenate([live_keys, store_keys]) they stand for.  store_keys are world
    keys, live_keys the volume's own brick coordinates (bx, by, bz).  With nothing stored there is no alignment to ask for: the frame
    is the volume (lo = origin, its dims and its box).  A brick in both lists is refused: the store holds what is OUTSIDE the box."""
    origin, vol_dims = np.asarray(origin, np.int64), np.asarray(vol_dims, np.int64)
    store_keys, live_keys = np.asarray(store_keys, np.int64).reshape(-1, 3), np.asarray(live_keys, np.int64).reshape(-1, 3)
    bmin64, bmax64 = np.asarray(vol_boxmin, np.float32).astype(np.float64), np.asarray(vol_boxmax, np.float32).astype(np.float64)
    bound = store_keys if cover is None else np.concatenate([store_keys, np.asarray(cover, np.int64).reshape(-1, 3)])
    if len(bound) == 0:
        lo, dims, first, vol_first = origin.copy(), vol_dims.copy(), np.zeros(3, np.int64), np.zeros(3, np.int64)
    else:
        if np.any(origin % BRICK) or np.any(vol_dims % BRICK):
            raise ValueError("world_frame: with stored bricks the volume's origin %s and dims %s must be whole bricks" % (tuple(origin), tuple(vol_dims)))
        first = np.minimum(origin // BRICK, bound.min(0))
        last = np.maximum((origin + vol_dims) // BRICK, bound.max(0) + 1)
        lo, dims, vol_first = first * BRICK, (last - first) * BRICK, origin // BRICK
    rel = np.concatenate([live_keys + vol_first, store_keys]) - first
    nb = (dims + BRICK - 1) // BRICK
    ids = (rel[:, 2] * nb[1] + rel[:, 1]) * nb[0] + rel[:, 0]
    order = np.argsort(ids, kind="stable")
    ids = ids[order]
    if np.any(np.diff(ids) == 0):
        raise ValueError("world_frame: a brick is both in the store and live in the volume")
    voxel = (bmax64 - bmin64) / (vol_dims - 1).astype(np.float64)
    boxmin = (bmin64 + (lo - origin).astype(np.float64) * voxel).astype(np.float32)
    boxmax = (bmin64 + (lo + dims - 1 - origin).astype(np.float64) * voxel).astype(np.float32)
    return lo, dims, boxmin, boxmax, ids.astype(np.uint32), order


def world_bricks(store, vol, origin, fill, ops=None, cover=None):
    """Everything a moving volume has seen as one brick list: the live bricks of `vol` (ops.BrickPack(vol, fill); its cell 0 is world
    cell `origin`) merged with the bricks of `store` (None: none) under world keys, on the frame world_frame() gives them (cover: world_frame's).
    Returns
    (lo, dims, boxmin, boxmax, ids, cells): ids uint32 (n,) ascending in the frame's grid, on the host; cells a uint8 device tensor
    (n, brick bytes) in that order -- the live bricks never leave the device.  What mesh.ExtractBrickMesh and ops.BrickUnpack take.
    The store is left as it is."""
    import torch
    if ops is None:
        from . import roo as ops
    live_ids, live_cells = ops.BrickPack(vol, fill)
    dims = (vol.w, vol.h, vol.d)
    nbx, nby = (vol.w + BRICK - 1) // BRICK, (vol.h + BRICK - 1) // BRICK
    lid = live_ids.cpu().numpy().view(np.uint32).astype(np.int64)
    live_keys = np.stack([lid % nbx, (lid // nbx) % nby, lid // (nbx * nby)], 1)
    if store is None:
        store_keys, store_cells = np.empty((0, 3), np.int64), None
    else:   # (a device store's payload is gathered where it is, never uploaded; a host store's is uploaded below)
        store_keys, store_cells = store.all_items()
    lo, fdims, boxmin, boxmax, ids, order = world_frame(store_keys, live_keys, origin, dims, vol.boxmin, vol.boxmax, cover)
    cells = live_cells
    if len(store_keys):
        cells = torch.cat([live_cells, store_cells if torch.is_tensor(store_cells) else torch.from_numpy(store_cells).to(live_cells.device)])
    cells = cells[torch.from_numpy(order).to(cells.device)].contiguous()
    return lo, fdims, boxmin, boxmax, ids, cells


def SaveBricks(path, vol, fill, ops=None):
    """A snapshot of a whole volume as one .npz: its dims, box, cell kind, the bits of `fill`, and the ids and cells of the bricks
    that differ from the fill cell (ops.BrickPack).  Returns the number of bricks written."""
    if ops is None:
        from . import roo as ops
    ids, cells = ops.BrickPack(vol, fill)
    with open(path, "wb") as f:
        np.savez(f, dims=np.array([vol.w, vol.h, vol.d], np.int64), boxmin=np.asarray(vol.boxmin, np.float32), boxmax=np.asarray(vol.boxmax, np.float32),
                 kind=np.array(vol.kind), fill_bits=np.array([fill], np.float32).view(np.uint32),
                 ids=ids.cpu().numpy().view(np.uint32), cells=cells.cpu().numpy())
    return int(ids.numel())


def LoadBricks(path, vol, ops=None):
    """Read a SaveBricks file into `vol`: refuses a volume of other dims or another cell kind; every cell becomes the file's fill
    cell, then the bricks are unpacked; vol takes the file's box.  Returns the number of bricks read."""
    if ops is None:
        from . import roo as ops
    with np.load(path) as z:
        dims, kind = tuple(int(v) for v in z["dims"]), str(z["kind"])
        if dims != (vol.w, vol.h, vol.d) or kind != vol.kind:
            raise ValueError("LoadBricks: the file holds a %s volume of %s, not a %s volume of %s" % (kind, dims, vol.kind, (vol.w, vol.h, vol.d)))
        fill = float(z["fill_bits"].view(np.float32)[0])
        ids, cells = z["ids"], z["cells"]
        vol.boxmin, vol.boxmax = z["boxmin"].astype(np.float32), z["boxmax"].astype(np.float32)
    ops.VolumeFill(vol, fill)
    if ids.size:
        ops.BrickUnpack(vol, ids, cells)
    return int(ids.size)
