// bricks_host.h -- what bricks.hip (include/kfx_bricks.h) decides on the host before it launches anything: the brick grid of a view,
// how the scratch is carved, and the refusals of a scratch, an id list and a payload; and the rules every brick operator shares
// (mesh_bricks_host.h, raycast_bricks_host.h, brick_pool_host.h): which frames are accepted, how many entries a list may have, and
// what is asked of a block of device memory a call is handed.  No HIP in here: scripts/bricks_host_check.cpp drives it under the
// host sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/kfx_bricks.h"
#include "shift_host.h"

namespace kfx {

constexpr int BRICK = 8, BRICK_CELLS = BRICK * BRICK * BRICK;
constexpr unsigned BRICK_SCAN_BLOCK = 256;                 // bricks per scan block: one per thread of a workgroup
constexpr unsigned long long BRICK_MAX = 0x7fffffffull;    // bricks of a view, entries of a list: ids are uint32, grids are int

struct BrickGeom {
    int w, h, d;            // cells of the view
    int nbx, nby, nbz;
    unsigned long long nb;  // bricks of the view
    unsigned long long nblk;   // scan blocks
};

// the brick grid of a view of w x h x d cells (every dimension >= 1)
inline BrickGeom brick_geom(size_t w, size_t h, size_t d)
{
    BrickGeom g{};
    g.w = (int)w; g.h = (int)h; g.d = (int)d;
    g.nbx = (int)((w + BRICK - 1) / BRICK); g.nby = (int)((h + BRICK - 1) / BRICK); g.nbz = (int)((d + BRICK - 1) / BRICK);
    g.nb = (unsigned long long)g.nbx * (unsigned long long)g.nby * (unsigned long long)g.nbz;
    g.nblk = (g.nb + BRICK_SCAN_BLOCK - 1) / BRICK_SCAN_BLOCK;
    return g;
}

inline size_t brick_round256(unsigned long long n) { return (size_t)((n + 255) / 256 * 256); }

// The scratch of a plan (offsets in bytes from its start; include/kfx_bricks.h states the sum):
//   hdr    256 bytes: word 0 (8 bytes) = the number of live bricks
//   flags  one byte per brick: 1 = live
//   part   uint32 per scan block: its live bricks
//   base   uint32 per scan block: the live bricks before it
struct BrickScratch {
    size_t hdr, flags, part, base, bytes;
};
inline BrickScratch brick_scratch(const BrickGeom& g)
{
    BrickScratch s{};
    s.hdr = 0;
    s.flags = 256;
    s.part = s.flags + brick_round256(g.nb);
    s.base = s.part + brick_round256(4 * g.nblk);
    s.bytes = s.base + brick_round256(4 * g.nblk);
    return s;
}

// a refusal: code 0 = accepted, else KFX_E_* and the rule that was broken
struct BrickRefusal {
    int code;
    const char* rule;
};

inline BrickRefusal brick_check_grid(const BrickGeom& g)
{
    if (g.nb > BRICK_MAX) return {KFX_E_RANGE, "more than 2^31 - 1 bricks"};
    return {0, nullptr};
}
// A block of device memory a call is handed -- a scratch, a pool: present, large enough, aligned to 256 bytes -- in that order.
inline BrickRefusal brick_check_block(const void* ptr, size_t have_bytes, size_t need_bytes, const char* null_rule, const char* small_rule,
                                      const char* align_rule)
{
    if (!ptr) return {KFX_E_NULL, null_rule};
    if (have_bytes < need_bytes) return {KFX_E_SHAPE, small_rule};
    if ((uintptr_t)ptr & 255) return {KFX_E_ALIGN, align_rule};
    return {0, nullptr};
}
// the scratch of a plan
inline BrickRefusal brick_check_scratch(const BrickGeom& g, const void* scratch, size_t scratch_bytes)
{
    return brick_check_block(scratch, scratch_bytes, brick_scratch(g).bytes, "null scratch",
                             "scratch smaller than kfx_bricks_scratch_bytes()", "scratch not aligned to 256 bytes");
}
// the id list and the payload of n entries (n == 0: nothing is asked of them)
inline BrickRefusal brick_check_lists(const void* ids, const void* cells, unsigned long long n)
{
    if (n == 0) return {0, nullptr};
    if (n > BRICK_MAX) return {KFX_E_RANGE, "more than 2^31 - 1 entries"};
    if (!ids || !cells) return {KFX_E_NULL, "null ids / cells"};
    if (((uintptr_t)ids & 3) || ((uintptr_t)cells & 15)) return {KFX_E_ALIGN, "ids not aligned to 4 bytes / cells not aligned to 16 bytes"};
    return {0, nullptr};
}

// ---- a FRAME (mesh_bricks.hip, raycast_bricks.hip): a virtual dense volume, of which only the dimensions and the box are read ----
constexpr size_t FRAME_MIN_DIM = 3, FRAME_MAX_DIM = 65535;   // the dimensions kfx_mesh_plan and kfx_raycast_sdf accept of a dense volume

// the frame; its brick grid in g
inline BrickRefusal brick_check_frame(const kfx_volume* frame, BrickGeom& g)
{
    if (!frame) return {KFX_E_NULL, "null frame"};
    if (frame->w < FRAME_MIN_DIM || frame->h < FRAME_MIN_DIM || frame->d < FRAME_MIN_DIM || frame->w > FRAME_MAX_DIM ||
        frame->h > FRAME_MAX_DIM || frame->d > FRAME_MAX_DIM)
        return {KFX_E_SHAPE, "frame dimensions"};
    g = brick_geom(frame->w, frame->h, frame->d);
    return brick_check_grid(g);
}
// ... and the kind of the SDF bricks, before the dimensions
inline BrickRefusal brick_check_frame(const kfx_volume* frame, int cell, BrickGeom& g)
{
    if (!frame) return {KFX_E_NULL, "null frame"};
    if (cell != KFX_CELL_F32 && cell != KFX_CELL_F16) return {KFX_E_RANGE, "unknown cell kind"};
    return brick_check_frame(frame, g);
}
// the entries of the SDF list and of the colour list
inline BrickRefusal brick_check_counts(unsigned long long n, unsigned long long n_color)
{
    if (n > BRICK_MAX || n_color > BRICK_MAX) return {KFX_E_RANGE, "more than 2^31 - 1 entries"};
    return {0, nullptr};
}

} // namespace kfx
