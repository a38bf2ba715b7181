// raycast_bricks_host.h -- what raycast_bricks.hip (include/kfx_raycast_bricks.h) decides on the host before it launches anything: the
// capacity of a table and how the scratch is carved -- from the brick counts alone, never from the frame -- the refusals of a plan's
// id list and of a scratch (the frame, the counts and the lists: bricks_host.h), and the table itself: where an id hashes to, how it is
// inserted and how it is looked up, written once for the kernels and for the host.  No HIP in here:
// scripts/raycast_bricks_host_check.cpp drives it under the host sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/kfx_raycast_bricks.h"
#include "bricks_host.h"

#if defined(__HIPCC__)
#define KFX_RB_HD __host__ __device__
#else
#define KFX_RB_HD
#endif

namespace kfx {

constexpr unsigned BRICK_SLOT_EMPTY = 0xffffffffu;                   // no brick id: a frame has 2^31 - 1 bricks at the most

// the id list of a plan with n entries (n == 0: nothing is asked of it)
inline BrickRefusal brick_ray_check_ids(const void* ids, unsigned long long n)
{
    if (n == 0) return {0, nullptr};
    if (!ids) return {KFX_E_NULL, "null ids"};
    if ((uintptr_t)ids & 3) return {KFX_E_ALIGN, "ids not aligned to 4 bytes"};
    return {0, nullptr};
}

// A table of m entries' capacity: 0 for none, else the smallest power of two >= 2 m (at most 2^32: m <= 2^31 - 1) and its log2.  At
// least half of the slots stay empty, so every probe sequence ends.
struct BrickTable {
    unsigned long long cap;
    int log2cap;
};
inline BrickTable brick_table(unsigned long long m)
{
    BrickTable t{0, 0};
    if (m == 0) return t;
    t.cap = 2;
    t.log2cap = 1;
    while (t.cap < 2 * m) { t.cap <<= 1; ++t.log2cap; }
    return t;
}

// The scratch of a plan and its renders (offsets in bytes from its start; include/kfx_raycast_bricks.h states the sum):
//   hdr    256 bytes: {n, n_color} uint32, {cap(n), cap(n_color)} uint64 at byte 8 -- a record the plan's kernel writes
//   tab    8 bytes {id, position} per slot of the SDF list's table
//   ctab   the same for the colour list
struct BrickRayScratch {
    size_t hdr, tab, ctab, bytes;
    BrickTable t, ct;
};
inline BrickRayScratch brick_ray_scratch(unsigned long long n, unsigned long long n_color)
{
    BrickRayScratch s{};
    s.t = brick_table(n);
    s.ct = brick_table(n_color);
    s.hdr = 0;
    s.tab = 256;
    s.ctab = s.tab + brick_round256(8 * s.t.cap);
    s.bytes = s.ctab + brick_round256(8 * s.ct.cap);
    return s;
}
// the scratch (bricks_host.h's rule)
inline BrickRefusal brick_ray_check_scratch(unsigned long long n, unsigned long long n_color, const void* scratch, size_t scratch_bytes)
{
    return brick_check_block(scratch, scratch_bytes, brick_ray_scratch(n, n_color).bytes, "null scratch",
                             "scratch smaller than kfx_raycast_bricks_scratch_bytes()", "scratch not aligned to 256 bytes");
}

// ---- the table: slots of two words {id, position}, BRICK_SLOT_EMPTY in the id word of a free one ----
// How the kernels see one: its slots, cap - 1, 32 - log2(cap) and the entries of the list it indexes.  n == 0: no table, nothing is read.
struct BrickTableView {
    const unsigned* slots;
    unsigned mask;
    int shift;
    unsigned n;
};
inline BrickTableView brick_table_view(const void* slots, const BrickTable& t, unsigned long long n)
{
    return BrickTableView{(const unsigned*)slots, (unsigned)(t.cap - 1), 32 - t.log2cap, (unsigned)n};
}
// first slot of an id: the top log2(cap) bits of a multiplicative hash (neighbouring ids, which is what a brick list holds, spread out);
// cap >= 2, so the shift is at most 31
KFX_RB_HD inline unsigned brick_slot_of(unsigned id, int shift) { return (id * 2654435761u) >> shift; }

// Insert (id -> pos).  cas(word, expected, desired) returns the word's value before: the device's atomicCAS, or a plain host
// compare-and-swap.  At most cap probes, every one inside the table; false if the id is already there (a repeated id keeps one of
// its entries) or -- which a table of capacity >= 2 n never does -- no slot is free.
template <typename CAS>
KFX_RB_HD inline bool brick_table_insert(unsigned* slots, unsigned mask, int shift, unsigned id, unsigned pos, CAS cas)
{
    unsigned s = brick_slot_of(id, shift), k = 0;
    do {
        const unsigned was = cas(slots + 2 * (size_t)s, BRICK_SLOT_EMPTY, id);
        if (was == BRICK_SLOT_EMPTY) {
            slots[2 * (size_t)s + 1] = pos;
            return true;
        }
        if (was == id) return false;
        s = (s + 1) & mask;
    } while (k++ != mask);
    return false;
}

// The position of brick `id` in the list, -1 if it is not listed.  At most cap probes, every one inside the table; a position is
// returned only if it is below n, whatever the table holds.
KFX_RB_HD inline int brick_table_find(const BrickTableView& t, unsigned id)
{
    if (t.n == 0) return -1;
    unsigned s = brick_slot_of(id, t.shift), k = 0;
    do {
        const unsigned key = t.slots[2 * (size_t)s], pos = t.slots[2 * (size_t)s + 1];
        if (key == id) return pos < t.n ? (int)pos : -1;
        if (key == BRICK_SLOT_EMPTY) return -1;
        s = (s + 1) & t.mask;
    } while (k++ != t.mask);
    return -1;
}

} // namespace kfx
