// brick_pool_host.h -- what brick_pool.hip (include/kfx_brick_pool.h) decides on the host before it launches anything: how a pool
// and its scratch are carved -- from (cell, capacity) and the brick count of the view alone, never from what the pool holds -- and
// the refusals of both; and the three rules of the pool itself, written once for the kernels and for the host: which keys lie in a
// key box, which slot the r-th brick of a spill takes, and how the header changes after a spill and after a take.  No HIP in here:
// scripts/brick_pool_host_check.cpp drives it under the host sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/kfx_brick_pool.h"
#include "bricks_host.h"

#if defined(__HIPCC__)
#define KFX_BP_HD __host__ __device__
#else
#define KFX_BP_HD
#endif

namespace kfx {

constexpr unsigned BRICK_POOL_FREE = 0, BRICK_POOL_OCCUPIED = 1;   // the state word of a key

// the first 40 bytes of a pool's 256-byte header: four counters, then the record of what the pool was initialised as (written by
// kfx_brick_pool_init for whoever looks at the bytes; no call reads it back)
struct BrickPoolHeader {
    unsigned long long free_n;      // entries of the free stack
    unsigned long long spilled, restored, dropped;   // cumulative
    unsigned cell, capacity;
};
// one slot's key: the world brick key and the state
struct BrickPoolKey {
    int bx, by, bz;
    unsigned state;
};

// A pool of `capacity` bricks of cb-byte cells (offsets in bytes from its start; include/kfx_brick_pool.h states the sum):
//   hdr    256 bytes: BrickPoolHeader
//   keys   16 bytes per slot
//   free   uint32 per slot: the stack of free slot numbers, free[0 .. free_n)
//   cells  512 cells per slot
struct BrickPoolLayout {
    size_t hdr, keys, free, cells, bytes;
    size_t brick_bytes;
};
inline BrickPoolLayout brick_pool_layout(size_t cb, unsigned long long capacity)
{
    BrickPoolLayout p{};
    p.brick_bytes = (size_t)BRICK_CELLS * cb;
    p.hdr = 0;
    p.keys = 256;
    p.free = p.keys + brick_round256(16 * capacity);
    p.cells = p.free + brick_round256(4 * capacity);
    p.bytes = p.cells + brick_round256(p.brick_bytes * capacity);
    return p;
}

// The scratch of a spill, a restore or a discard over n entries (the bricks of the view or the slots of the pool, whichever are
// more; a discard: the slots):
//   hdr    256 bytes: word 0 (8 bytes) = the number of flagged entries of the scan in progress
//   flags  one byte per entry
//   part   uint32 per scan block of 256 entries: its flagged entries
//   base   uint32 per scan block: the flagged entries before it
//   list   uint32 per entry: the flagged entries in ascending order
struct BrickPoolScratch {
    size_t hdr, flags, part, base, list, bytes;
    unsigned long long n, nblk;
};
inline BrickPoolScratch brick_pool_scratch(unsigned long long view_bricks, unsigned long long capacity)
{
    BrickPoolScratch s{};
    s.n = view_bricks > capacity ? view_bricks : capacity;
    s.nblk = (s.n + BRICK_SCAN_BLOCK - 1) / BRICK_SCAN_BLOCK;
    s.hdr = 0;
    s.flags = 256;
    s.part = s.flags + brick_round256(s.n);
    s.base = s.part + brick_round256(4 * s.nblk);
    s.list = s.base + brick_round256(4 * s.nblk);
    s.bytes = s.list + brick_round256(4 * s.n);
    return s;
}

// the cell kind and the capacity -- in that order; cb = the cell's bytes
inline BrickRefusal brick_pool_check_kind(int cell, unsigned long long capacity, size_t& cb)
{
    cb = shift_cell_bytes(cell);
    if (!cb) return {KFX_E_RANGE, "unknown cell kind"};
    if (capacity == 0 || capacity > BRICK_MAX) return {KFX_E_RANGE, "capacity 0 or above 2^31 - 1"};
    return {0, nullptr};
}
// the pool and the scratch (bricks_host.h's rule)
inline BrickRefusal brick_pool_check_pool(const void* pool, size_t pool_bytes, size_t cb, unsigned long long capacity)
{
    return brick_check_block(pool, pool_bytes, brick_pool_layout(cb, capacity).bytes, "null pool", "pool smaller than kfx_brick_pool_bytes()",
                             "pool not aligned to 256 bytes");
}
inline BrickRefusal brick_pool_check_scratch(unsigned long long view_bricks, unsigned long long capacity, const void* scratch, size_t scratch_bytes)
{
    return brick_check_block(scratch, scratch_bytes, brick_pool_scratch(view_bricks, capacity).bytes, "null scratch",
                             "scratch smaller than kfx_brick_pool_scratch_bytes()", "scratch not aligned to 256 bytes");
}
// a key box of nb[a] >= 1 bricks from key0: its last key, key0 + nb - 1, is an int32 on every axis
inline BrickRefusal brick_pool_check_keys(const int key0[3], const int nb[3])
{
    for (int a = 0; a < 3; ++a)
        if ((long long)key0[a] + (long long)nb[a] - 1 > 0x7fffffffll) return {KFX_E_RANGE, "the key range leaves int32"};
    return {0, nullptr};
}

// ---- the rules of the pool, for the kernels and for the host ----
// A key box: nb bricks per axis from key0; brick (i, j, k) of it has the id (k * nb[1] + j) * nb[0] + i.
struct BrickPoolBox {
    int key0[3];
    int nb[3];
};

// Does the key lie in the box?  Then *id = its brick id in the box's grid: a coordinate is used only if it lies inside the grid,
// whatever the key holds.
KFX_BP_HD inline bool brick_pool_key_in_box(const BrickPoolBox& b, int bx, int by, int bz, unsigned* id)
{
    const long long i = (long long)bx - b.key0[0], j = (long long)by - b.key0[1], k = (long long)bz - b.key0[2];
    if (i < 0 || j < 0 || k < 0 || i >= b.nb[0] || j >= b.nb[1] || k >= b.nb[2]) return false;
    *id = (unsigned)((k * b.nb[1] + j) * b.nb[0] + i);
    return true;
}
// the key of brick `id` of the box
KFX_BP_HD inline BrickPoolKey brick_pool_key_of(const BrickPoolBox& b, unsigned id)
{
    const unsigned nxy = (unsigned)b.nb[0] * (unsigned)b.nb[1], r = id % nxy;
    return BrickPoolKey{b.key0[0] + (int)(r % (unsigned)b.nb[0]), b.key0[1] + (int)(r / (unsigned)b.nb[0]), b.key0[2] + (int)(id / nxy), BRICK_POOL_OCCUPIED};
}

// the header's free_n as the calls use it: never above the capacity, whatever the header holds
KFX_BP_HD inline unsigned long long brick_pool_free_n(unsigned long long free_n, unsigned long long capacity) { return free_n < capacity ? free_n : capacity; }

// The r-th live brick of a spill (ascending brick id, r from 0) takes the slot free[free_n - 1 - r]: the index into free[], or -1 where
// the brick is dropped (r >= free_n).
KFX_BP_HD inline long long brick_pool_spill_index(unsigned long long free_n, unsigned long long r) { return r < free_n ? (long long)(free_n - 1 - r) : -1; }
// The i-th slot a restore or a discard takes (ascending slot number, i from 0) is pushed to free[free_n + i]: the index, or -1 where
// the stack is full -- which a pool that holds a slot either in its keys or in its stack never is.
KFX_BP_HD inline long long brick_pool_push_index(unsigned long long free_n, unsigned long long i, unsigned long long capacity)
{
    return free_n + i < capacity ? (long long)(free_n + i) : -1;
}
// A slot number read from free[] or from a list is used only if it is below the capacity.
KFX_BP_HD inline bool brick_pool_slot_ok(unsigned slot, unsigned long long capacity) { return slot < capacity; }

// the header after a spill of `live` bricks ...
KFX_BP_HD inline void brick_pool_after_spill(BrickPoolHeader& h, unsigned long long live, unsigned long long capacity)
{
    const unsigned long long free_n = brick_pool_free_n(h.free_n, capacity), taken = live < free_n ? live : free_n;
    h.free_n = free_n - taken;
    h.spilled += taken;
    h.dropped += live - taken;
}
// ... and after `taken` slots left the pool: a restore counts them, a discard does not
KFX_BP_HD inline void brick_pool_after_take(BrickPoolHeader& h, unsigned long long taken, unsigned long long capacity, bool restore)
{
    const unsigned long long free_n = brick_pool_free_n(h.free_n, capacity), room = capacity - free_n, pushed = taken < room ? taken : room;
    h.free_n = free_n + pushed;
    if (restore) h.restored += taken;
}

} // namespace kfx
